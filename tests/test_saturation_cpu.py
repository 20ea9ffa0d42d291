"""tests/saturation_cases.py without a GPU: that its dtype-taking restatements are, at float64, the references of the
existing suites; that every case and tensor meets 8 e32 <= bound (e32 = max|f32 - f64| of the same restatement on the same
float32 operands), so no bound of tests/test_saturation_gpu.py is wider than float32 itself needs; and that every profile
produces the regime it is named for, so a later edit of a helper cannot quietly turn a row back into unit-scale data.
Prints e32, the bound and their ratio per case and tensor."""
import math

import numpy as np
import pytest
import torch

from tests import saturation_cases as SAT

B, PAD = SAT.B, SAT.PAD


@pytest.fixture(scope="module")
def ops():
    from r3d_amd import ops as o          # (host-only queries: the split-key chunk)
    return o


def _att_cases():
    from r3d_amd import ops
    return SAT.att_cases(ops.mha_splitk_chunk)


ATT = _att_cases()
ATT_IDS = [c[0] for c in ATT]


def _condition(tag, pairs):
    """pairs [(name, f32, f64)] under SAT.rel_bound: prints, then asserts 8 e32 <= bound"""
    bad = []
    for name, f32, f64 in pairs:
        f64 = f64.double()
        assert bool(torch.isfinite(f64).all()) and bool(torch.isfinite(f32).all()), (tag, name)
        e32 = float((f32.double() - f64).abs().max())
        bound = SAT.rel_bound(name) * max(float(f64.abs().max()), 1e-5)
        print(f"[saturation] {tag} {name}: e32 {e32:.2e} bound {bound:.2e} ratio {SAT.MARGIN * e32 / bound:.3f}")
        if not SAT.MARGIN * e32 <= bound:
            bad.append((name, e32, bound))
    assert not bad, (tag, bad)


def _loss_condition(tag, pairs):
    """pairs [(name, f32, f64, kind)] under tests/loss_cases.py's margins (SAT.loss_bound)"""
    bad = []
    for name, f32, f64, kind in pairs:
        f64 = torch.as_tensor(f64).double()
        err = (torch.as_tensor(f32).double() - f64).abs()
        bound = SAT.loss_bound(f64, kind)
        ratio = float((SAT.MARGIN * err / bound).max())
        print(f"[saturation] {tag} {name}: e32 {float(err.max()):.2e} bound {float(bound.max()):.2e} ratio {ratio:.3f}")
        if not ratio <= 1.0:
            bad.append((name, float(err.max()), float(bound.max())))
    assert not bad, (tag, bad)


# ---------------------------------------------------------------------------------------------------------------------
# A
# ---------------------------------------------------------------------------------------------------------------------
def test_attention_table_is_the_issues():
    rows = {(r[0], r[1], r[2], r[3], r[4]) for r in SAT.ATT_ROWS}
    assert rows == {("core", 8, 21, 16, 8), ("core", 8, 64, 128, 1), ("core", 8, 130, 16, 8), ("core", 40, 70, 25, 4),
                    ("tiled", 70, 70, 16, 8), ("tiled", 8, 130, 25, 8), ("tiled", 16, 130, 128, 1),
                    ("splitk", 8, "C+1", 16, 8), ("splitk", 16, "2C+1", 16, 8), ("splitk", 8, "C+1", 128, 1)}
    from r3d_amd import ops
    assert ops.mha_core_supported(40, 70, 25, True) and not ops.mha_core_supported(41, 70, 25, True)    # (the issue's Lq = 70)
    for core in ("core", "tiled", "splitk"):
        masked = [r[5] for r in SAT.ATT_ROWS if r[0] == core]
        assert any(masked) and not all(masked), core
    by_row = {}
    for _, i, Lk, C, p in ATT:
        by_row.setdefault(i, []).append(p)
    for i, ps in by_row.items():
        core, Lq, lk, dh, heads, masked = SAT.ATT_ROWS[i]
        assert "sharp" in ps and "shift" in ps
        if lk not in (21, 64):
            assert sum(p.startswith("stair") for p in ps) == 1
            assert ({"cliff_up", "cliff_down"} <= set(ps)) == (dh == 16), (i, ps)
        if masked:                                   # the keep-mask's row stride is no multiple of 4 bytes
            assert next(c[2] for c in ATT if c[1] == i) % 4
    assert {p for ps in by_row.values() for p in ps} == {"sharp", "shift", "stair_up", "stair_down", "cliff_up", "cliff_down"}
    # the split-key row with a third chunk masks its whole first chunk under cliff_down, in every clip
    i, Lk, C = next((c[1], c[2], c[3]) for c in ATT if c[0].startswith("splitk-Lq16") and c[4] == "cliff_down")
    assert Lk == 2 * C + 1 and bool((SAT.att_problem(i, Lk, C, "cliff_down")["lab"][:, :C] == PAD).all())


@pytest.mark.parametrize("cid", [ATT_IDS[0], ATT_IDS[-1], next(c for c in ATT_IDS if "tiled" in c and "drop" in c)])
def test_attention_restatement_is_the_tiled_tests_reference(cid):
    from tests.test_tiled_attention_gpu import reference
    _, i, Lk, C, prof = ATT[ATT_IDS.index(cid)]
    _, Lq, _, dh, heads, _ = SAT.ATT_ROWS[i]
    H = heads * dh
    p = SAT.att_problem(i, Lk, C, prof)
    o, lse, dq, dk, dv = reference(p["q"], p["kv"][:, :H], p["kv"][:, H:], p["d_o"], p["lab"], p["keep"], p["dsc"], heads, dh, Lq, Lk)
    r = p["ref"]
    for a, b in ((o, r["o"]), (lse, r["lse"]), (dq, r["dq"]), (dk, r["dk"]), (dv, r["dv"])):
        assert a.dtype == torch.float64 and torch.equal(a, b), cid
    assert p["ref32"]["o"].dtype == torch.float32 and p["ref32"]["dq"].dtype == torch.float32


@pytest.mark.parametrize("cid", ATT_IDS)
def test_attention_case_meets_the_condition_and_its_regime(cid):
    _, i, Lk, C, prof = ATT[ATT_IDS.index(cid)]
    core, Lq, _, dh, heads, masked = SAT.ATT_ROWS[i]
    p = SAT.att_problem(i, Lk, C, prof)
    _condition(cid, SAT.att_pairs(p) + [("dq|dk|dv", SAT.joint(p["ref32"]), SAT.joint(p["ref"]))])
    zero = [n for n in ("dq", "dk", "dv") if SAT.negligible(p["ref"], n)]
    if zero:
        print(f"[saturation] {cid}: {zero} are 0 at float32's resolution of the joint gradient scale")
    assert "dv" not in zero
    if "cut" in p:                                   # the first tile or chunk alone gives the same rows, in float64 too
        _condition(cid, [("o vs the first tile alone", p["ref32"]["o"], p["cut"])])
    s = SAT.scores(p, i, Lk)
    if prof == "sharp":
        mp = float(s.softmax(-1).max(-1).values.mean())
        print(f"[saturation] {cid}: mean max-probability {mp:.3f}, score std {float(s.std()):.1f}")
        assert mp >= 0.9
        assert float((s - s.max(-1, keepdim=True).values).min()) < -100.0          # exp of -100 and below inside a row
    elif prof == "shift":
        flat = SAT.apply_profile("flat", p["q"], p["kv"][:, :heads * dh], heads, dh, p["step"])
        pf = dict(p, q=flat[0], kv=torch.cat([flat[1], p["kv"][:, heads * dh:]], 1))
        d = s - SAT.scores(pf, i, Lk)
        assert float((d - SAT.SHIFT).abs().max()) < 1e-5                            # every score moved by the shift
    else:
        step = p["step"]
        nt = -(-Lk // step)
        assert nt >= 2
        tm = torch.stack([s[..., t * step:(t + 1) * step].max(-1).values for t in range(nt)], -1)     # [B, heads, Lq, tiles]
        if prof.startswith("cliff"):
            d = (tm - tm.max(-1, keepdim=True).values).float()
            dominated = d < 0
            assert int(dominated.sum()) == d[..., 0].numel() * (nt - 1)
            e = torch.exp(d[dominated])
            print(f"[saturation] {cid}: largest float32 exp(m_tile - m_row) of a dominated tile {float(e.max()):.1e} "
                  f"(argument {float(d[dominated].max()):.1f})")
            assert e.dtype == torch.float32 and bool((e == 0).all())
            top = tm.argmax(-1)
            assert bool((top == (nt - 1 if prof == "cliff_up" else 0)).all())
        else:
            # consecutive tile maxima: 4 apart in the mean between full tiles (a row's own differ by the maxima of 64
            # unit-scale scores, +-2 at the extremes); a partial last tile's maximum lies lower, so its step is shorter
            # going up and longer going down, and never near 0
            df = ((tm[..., 1:] - tm[..., :-1]) * (1 if prof == "stair_up" else -1)).reshape(-1, nt - 1)
            mean = df.mean(0).tolist()
            print(f"[saturation] {cid}: mean step of the tile maxima {[round(m, 2) for m in mean]}")
            full = Lk // step
            assert all(3.0 <= m <= 5.0 for m in mean[:full - 1]), mean
            assert all(1.5 <= m <= 7.0 for m in mean), mean
            assert full < 2 or float(df[:, :full - 1].min()) > 0.0


@pytest.mark.parametrize("name", SAT.XCLIP_NAMES)
@pytest.mark.parametrize("profile", ["sharp", "shift"])
def test_xclip_case_meets_the_condition_and_its_regime(name, profile):
    p = SAT.xclip_problem(name, profile)
    _condition(f"xclip {name} {profile}", SAT.xclip_pairs(p))
    if profile == "sharp":
        mp = float(p["probs"].max(-1).values.mean())
        print(f"[saturation] xclip {name}: mean max-probability {mp:.3f}")
        assert mp >= 0.9


# ---------------------------------------------------------------------------------------------------------------------
# B
# ---------------------------------------------------------------------------------------------------------------------
def _confident(profile, loss_rows, grad_rows):
    """confident_right: float64 loss < 1e-15 and a gradient of nothing on the edited rows; confident_wrong: loss >= 50"""
    if profile == "confident_right":
        assert float(loss_rows.max()) < 1e-15 and float(grad_rows.abs().max()) < 1e-15
    elif profile == "confident_wrong":
        assert float(loss_rows.min()) >= SAT.CONFIDENT


@pytest.mark.parametrize("profile", SAT.LOGIT_PROFILES)
@pytest.mark.parametrize("name", SAT.LOSS_CASES)
def test_loss_launch_case_meets_the_condition_and_its_regime(name, profile):
    from tests import loss_cases as LC
    p = SAT.loss_problem(name, profile)
    c, t, ref = p["c"], p["t"], p["ref"]
    N, BQ, K = c["B"] * c["S"], c["B"] * c["Q"], c["K"]
    Ks = c["Kseg"] or K
    assert LC.in_oracle_subset(c) or c["Kseg"]
    # the restatement at float64 is losses64's cross-entropy terms
    for n, want in (("loss_seg", ref["loss"][0]), ("loss_act", ref["loss"][1]), ("d_seg", ref["d_seg"].reshape(N, Ks)),
                    ("d_act", ref["d_act"].reshape(BQ, K))):
        assert torch.allclose(p["r64"][n], want, rtol=1e-12, atol=1e-15), (name, profile, n)
    _loss_condition(f"losses {name} {profile}", SAT.loss_pairs(p))
    plain = LC.make(c)
    assert torch.equal(t["dur"], plain["dur"]) and torch.equal(t["past_label"], plain["past_label"])     # (the duration term: untouched)
    for key, C, gold, valid in (("seg", Ks, t["past_label"], ref["info"]["seg_valid"]), ("act", K, t["target"], ref["info"]["act_valid"])):
        x, x0, gold = t[key].reshape(-1, C), plain[key].reshape(-1, C), gold.reshape(-1)
        changed = (x != x0).any(1)
        ce, d = SAT.ce_rows(x, gold, valid, torch.float64)
        if profile in ("sharp", "shift"):
            assert bool(changed.all())
            continue
        assert bool((changed <= valid).all()) and int(changed.sum()) >= 1
        _confident(profile, ce[changed], d[changed] if profile == "confident_right" else None)
        # the ties the table built are still ties at the row maximum
        mx = x.max(1, keepdim=True).values
        assert int(((x == mx).sum(1) > 1).sum()) == int(((x0 == x0.max(1, keepdim=True).values).sum(1) > 1).sum())


@pytest.mark.parametrize("profile", SAT.LOGIT_PROFILES)
@pytest.mark.parametrize("rows,C,pad", SAT.CE_ROWS)
def test_ce_rows_case_meets_the_condition_and_its_regime(rows, C, pad, profile):
    p = SAT.ce_problem(rows, C, pad, profile)
    _loss_condition(f"ce_rows {rows}x{C} {profile}", SAT.ce_pairs(p))
    live = p["tgt"] != pad
    ce, d = SAT.ce_rows(p["x"], p["tgt"], live, torch.float64)
    _confident(profile, ce[live], d[live] if profile == "confident_right" else None)
    if profile == "confident_right":
        assert p["ref"]["counts"] == [int(live.sum()), int(live.sum())]
    if profile == "confident_wrong":
        assert p["ref"]["counts"][0] == 0


def test_focal_table_covers_gamma_and_alpha():
    assert {(c["gamma"], c["alpha"]) for c in SAT.FOCAL} == {(1.0, 1.0), (2.0, 1.0), (1.0, 0.25), (2.0, 0.25)}
    assert sorted(c["C"] for c in SAT.FOCAL) == [17, 64, 65, 122]


@pytest.mark.parametrize("profile", SAT.LOGIT_PROFILES)
@pytest.mark.parametrize("name", [c["name"] for c in SAT.FOCAL])
def test_focal_case_meets_the_condition_and_its_regime(name, profile):
    from tests import temporal_oracle as TO
    p = SAT.focal_problem(name, profile)
    case, ref = p["case"], p["ref"]
    loss, flags, nc, nl = TO.focal(p["pred"], p["gold"], case["pad"], case["exclude"], case["alpha"], case["gamma"], case["penalty"])
    assert torch.equal(loss, ref["loss"]) and torch.equal(flags, ref["flags"]) and [nc, nl] == ref["counts"]
    pairs = [("loss", p["ref32"]["loss"], ref["loss"], "loss"), ("d", p["ref32"]["d"], ref["d"], "grad")]
    if "flat" in p:
        pairs += [("loss vs unshifted", p["ref32"]["loss"], p["flat"]["loss"], "loss"), ("d vs unshifted", p["ref32"]["d"], p["flat"]["d"], "grad")]
    _loss_condition(f"focal {name} {profile}", pairs)
    assert torch.equal(p["ref32"]["flags"], ref["flags"])
    edited = p["live"] & ~p["skip"]
    assert int(p["skip"].sum()) >= 1 and int(edited.sum()) >= 8
    ce, d = SAT.ce_rows(p["pred"], p["gold"], p["live"], torch.float64)
    _confident(profile, ce[edited], d[edited] if profile == "confident_right" else None)
    if profile == "confident_right":                 # (1 - p)^gamma ce as p -> 1: nothing, gradient included
        assert float(ref["d"][edited].abs().max()) < 1e-15 and bool(ref["flags"][edited].all())
    if profile == "confident_wrong":                 # as p -> 0 the focal weight is 1: alpha ce / N per row
        assert not bool(ref["flags"][edited].any())


# ---------------------------------------------------------------------------------------------------------------------
# C
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SAT.SUPCON_NAMES)
def test_supcon_case_meets_the_condition_and_its_regime(name):
    from tests import supcon_cases as SC, supcon_oracle as SO
    p = SAT.supcon_problem(name)
    case, z, yo, kw, ref = p["case"], p["z"], p["yo"], p["kw"], p["ref"]
    assert case["T"] == case["Tb"] == 0.01 and case["unit"] and not case["normalize"]
    l64, g64, lse64, P64 = SO.supcon_with_grad(z, yo, **kw)
    assert torch.equal(l64, ref["loss"]) and torch.equal(g64, ref["d"]) and torch.equal(lse64, ref["lse"]) and torch.equal(P64, ref["P"])
    A = kw["A"]
    kept = torch.ones(A, dtype=torch.bool) if not case["ignore"] else (yo[:A] != SC.IGNORE)
    rows = kept & torch.isfinite(lse64)
    _condition(f"supcon {name}", [("loss", p["ref32"]["loss"].reshape(1), ref["loss"].reshape(1)),
                                  ("lse", p["ref32"]["lse"][rows], ref["lse"][rows]), ("d", p["ref32"]["d"], ref["d"])])
    s = (z.double() @ z.double().t()) / case["T"]
    off = s - torch.diag(torch.full((s.shape[0],), float("inf"), dtype=torch.float64))
    print(f"[saturation] supcon {name}: off-diagonal scores in [{float(off.min()):.1f}, {float(off[off > -1e300].max()):.1f}]")
    assert float(off.max()) - float(off.min()) > 100.0 and float(ref["loss"]) > 1.0
    if name == "sat_n65_d16":
        y = p["y"]
        assert torch.equal(z[0], z[1]) and int(y[0]) == int(y[1]) and abs(float(s[0, 1]) - 100.0) < 1e-4
        twin = [r for r in range(3, z.shape[0]) if torch.equal(z[r], z[2])]
        assert len(twin) == 1 and int(y[twin[0]]) != int(y[2])
    if case["ignore"]:
        assert 0 < int((yo == SC.IGNORE).sum()) < yo.numel() and case["V"] == 2 and case["mode"] == "all"


# ---------------------------------------------------------------------------------------------------------------------
# D
# ---------------------------------------------------------------------------------------------------------------------
def test_lstm_table_is_the_issues(ops):
    from r3d_amd.engine_rnn import lstm_route
    assert SAT.LSTM_CASES == [("registers", 8, 16, 128), ("registers", 13, 37, 136), ("steps", 1, 2, 264),
                              ("steps", 5, 3, 520), ("steps", 8, 16, 512), ("steps", 8, 16, 128)]
    for route, _, _, H in SAT.LSTM_CASES:           # by rule, or the steps route forced where the registers route exists
        assert lstm_route(H, True) == route or (route == "steps" and H == 128 and ops.lstm_steps_supported(H)), (route, H)


@pytest.mark.parametrize("Bc,S,H", sorted({c[1:] for c in SAT.LSTM_CASES}))
def test_lstm_case_meets_the_cap_and_sits_on_its_rails(Bc, S, H):
    from tests import rnn_wide_cases as WC
    ref, bounds, f32 = SAT.lstm_reference(Bc, S, H)
    bad = []
    for k in WC.TENSORS:
        bound, e32, scale = bounds[k]
        assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(f32[k]).all())
        print(f"[saturation] lstm B{Bc} S{S} H{H} {k}: e32 {e32:.2e} bound {bound:.2e} scale {scale:.2e} "
              f"cap ratio {WC.MARGIN * e32 / (WC.CAP * scale):.3f}")
        assert scale > 0.0
        if not WC.MARGIN * e32 <= WC.CAP * scale:
            bad.append((k, e32, scale))
    assert not bad, bad
    # the rails, on the float32 cast of the float64 gates: per direction [i | f | g | o], each h wide
    h = H // 2
    g = ref["gates"].float().reshape(Bc * S, 2, 4, h)
    q = SAT.quarters(h)
    one, half_ulp = torch.tensor(1.0), 2.0 ** -25
    frac = lambda t: float(t.float().mean())        # noqa: E731
    f0, i1, o2, g2 = g[:, :, 1, q[0]], g[:, :, 0, q[1]], g[:, :, 3, q[2]], g[:, :, 2, q[2]]
    print(f"[saturation] lstm B{Bc} S{S} H{H}: f == 1 on {frac(f0 == 1):.2f} of quarter 0, i < 2^-25 on {frac(i1 < half_ulp):.2f} "
          f"of quarter 1 (largest {float(i1.max()):.1e}), o == 1 on {frac(o2 == 1):.2f} and g == 1 on {frac(g2 == 1):.2f} of quarter 2")
    # quarter 0: f(1 - f) is exactly 0; quarter 2: o(1 - o) and 1 - g^2 are.  Quarter 1: sigmoid(-20) = 2e-9 is a normal
    # float32, not 0 -- its rail is 1 - i == 1 in float32 (i below half an ulp of 1), so i(1 - i) = i and nothing is left of
    # the input.  At least a quarter of each saturated gate's values must sit there (in fact all do).
    assert frac(f0 == one) >= 0.25 and frac(o2 == one) >= 0.25 and frac(g2 == one) >= 0.25 and frac(i1 < half_ulp) >= 0.25
    assert bool(((one - i1) == one).all())
    # quarter 3 is left in its linear region
    rest = g[:, :, :, q[3]]
    assert float(rest[:, :, [0, 1, 3]].min()) > 0.05 and float(rest[:, :, [0, 1, 3]].max()) < 0.95
    # and the unrailed inputs are rnn_wide_cases' own
    w0, x0, dy0 = WC.inputs(Bc, S, H)
    w, x, dy = SAT.lstm_inputs(Bc, S, H)
    assert torch.equal(x, x0) and torch.equal(dy, dy0)
    for k in w0:
        assert torch.equal(w[k], w0[k]) == (k[0] != "b_hh"), k
        assert torch.equal(w[k], w[k].float().double())


def test_values_in_use():
    assert (SAT.SHIFT, SAT.STAIR, SAT.SHARP, SAT.LOGIT_SHIFT, SAT.CONFIDENT, SAT.RAIL, SAT.RAIL_G) == (16.0, 4.0, 30.0, 100.0, 50.0, 20.0, 12.0)
    assert 100.0 <= SAT.CLIFF <= 116.0 and math.exp(-SAT.CLIFF + 8) < float(np.finfo(np.float32).smallest_subnormal) / 2
