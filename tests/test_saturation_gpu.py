"""The softmax, row cross-entropy, contrastive and LSTM gate kernels where their inputs saturate (tests/saturation_cases.py),
through r3d_amd.ops against the float64 references of their own suites: sharp softmaxes, running maxima that move by 4 per
tile, whole tiles and chunks that underflow, a shift that only max subtraction cancels, logits 50 past the row's extremes,
contrast scores of +-100, gates on their rails.  Every case prints err, scale and bound per tensor before it asserts; every
output is finite, the outside of every strided buffer untouched, a second run bit-equal.  Bounds: those of the kernels' own
suites (tests/saturation_cases.py; tests/test_saturation_cpu.py shows that float32 itself meets them 8 times over).
Needs an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from tests import saturation_cases as SAT  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402
from tests.test_query_kernels_gpu import strided, outside_untouched  # noqa: E402

B, PAD = SAT.B, SAT.PAD


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


def _att_cases():
    from r3d_amd import ops
    return SAT.att_cases(ops.mha_splitk_chunk)


ATT = _att_cases()


def held(tag, name, got, want, rtol):
    """print the figures, then close_rel"""
    a, b = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    scale = float(b.abs().max())
    finite = bool(torch.isfinite(a).all())
    err = float((a - b).abs().max()) if finite and a.shape == b.shape else float("inf")
    print(f"[saturation] {tag} {name}: err {err:.2e}, scale {scale:.2e}, bound {rtol * max(scale, 1e-5):.2e}")
    assert finite, f"{tag} {name}: not finite"
    close_rel(a, b, f"{tag} {name}", rtol=rtol)


# ---------------------------------------------------------------------------------------------------------------------
# A. attention cores
# ---------------------------------------------------------------------------------------------------------------------
def _run_attention(ops, core, p, Lq, Lk, dh, heads, aligned):
    """One forward + backward: q and d_o buffers of their own, k | v the halves of one buffer, dq a slice of [B*Lq, H + 9],
    dk | dv the halves of a slice of a wider buffer (16-byte aligned rows where the small path needs them), NaN outside."""
    H = heads * dh
    qd, kvd, dod, labd = p["q"].to(DEV), p["kv"].to(DEV), p["d_o"].to(DEV), p["lab"].to(DEV)
    keep = None if p["keep"] is None else p["keep"].to(DEV)
    dq, dqb = strided(torch.zeros(B * Lq, H), H + 9, 5)
    ld, c0 = (2 * H + 8, 4) if aligned else (2 * H + 7, 3)
    dkv, dkvb = strided(torch.zeros(B * Lk, 2 * H), ld, c0)
    k, v, dk, dv = kvd[:, :H], kvd[:, H:], dkv[:, :H], dkv[:, H:]
    out = {}
    if core == "core":
        assert ops.mha_core_supported(Lq, Lk, dh, True)
        probs = torch.full((B, heads, Lq, Lk), float("nan"), device=DEV)
        o = torch.full((B * Lq, H), float("nan"), device=DEV)
        ops.mha_core_fwd(qd, k, v, probs, o, B, heads, Lq, Lk, dh, key_labels=labd, pad_idx=PAD, drop_mask=keep, drop_scale=p["dsc"])
        ops.mha_core_bwd(qd, k, v, probs, dod, dq, dk, dv, B, heads, Lq, Lk, dh, drop_mask=keep, drop_scale=p["dsc"])
        out.update(o=o, probs=probs)
    elif core == "tiled":
        from tests.test_tiled_attention_gpu import run_tiled
        assert ops.mha_tiled_supported(Lq, Lk, dh, True)
        o, lse, delta = run_tiled(ops, qd, k, v, dod, heads, dh, Lq, Lk, dq, dk, dv, key_labels=labd, keep=keep, dsc=p["dsc"])
        out.update(o=o, lse=lse, delta=delta)
    else:
        from tests.test_attention_splitk_gpu import run_splitk
        assert ops.mha_splitk_supported(Lq, Lk, dh, True)
        o, lse, delta = run_splitk(ops, qd, k, v, dod, heads, dh, Lq, Lk, dq, dk, dv, key_labels=labd, keep=keep, dsc=p["dsc"])
        out.update(o=o, lse=lse, delta=delta)
    torch.cuda.synchronize()
    out.update(dq=dq, dk=dk, dv=dv)
    untouched = outside_untouched(dqb, 5, H) and outside_untouched(dkvb, c0, 2 * H)
    return out, untouched


@pytest.mark.parametrize("cid,i,Lk,C,prof", ATT, ids=[c[0] for c in ATT])
def test_attention_core_where_the_softmax_saturates(ops, cid, i, Lk, C, prof):
    core, Lq, _, dh, heads, masked = SAT.ATT_ROWS[i]
    p = SAT.att_problem(i, Lk, C, prof)
    small = core == "core" and Lq == 8 and Lk <= 64
    got, untouched = _run_attention(ops, core, p, Lq, Lk, dh, heads, aligned=small)
    again, _ = _run_attention(ops, core, p, Lq, Lk, dh, heads, aligned=small)
    for against, ref in (("", p["ref"]),) + (((" vs unshifted", p["flat"]),) if "flat" in p else ()):
        # (the shift cancels: the unshifted problem's reference, lse moved back)
        for n in SAT.ATT_TENSORS:
            if n not in got:
                continue
            if SAT.negligible(ref, n):              # an exact 0 (one key holds all the weight): the joint scale alone, below
                err = float((got[n].double().cpu() - ref[n]).abs().max())
                print(f"[saturation] {cid} {n}{against}: err {err:.2e}, scale {float(ref[n].abs().max()):.2e}, held to dq|dk|dv")
                assert bool(torch.isfinite(got[n]).all()), (cid, n)
                continue
            held(cid, n + against, got[n] - (SAT.SHIFT if against and n == "lse" else 0.0), ref[n], SAT.rel_bound(n))
        held(cid, "dq|dk|dv" + against, SAT.joint(got), SAT.joint(ref), 1e-3)
    if "cut" in p:                                  # what the dominated tiles or chunks add is exactly 0
        held(cid, "o vs the first tile alone", got["o"], p["cut"], SAT.rel_bound("o"))
    assert untouched, cid
    for n in got:
        assert torch.equal(got[n], again[n]), (cid, n)


def _run_xclip(ops, p):
    """q, d_o, o and d_qkv as 16-byte aligned column slices of wider NaN-filled buffers (tests/test_l3_gpu._xclip "strided")"""
    case = p["case"]
    Bc, S, H, heads = case["B"], case["S"], case["H"], case["heads"]
    N = Bc * S
    q, _ = strided(p["qkv"].reshape(N, 3 * H), 3 * H + 8, 4)
    g, _ = strided(p["d_o"].reshape(N, H), H + 8, 4)
    o, ob = strided(torch.zeros(N, H), H + 12, 4)
    d, db = strided(torch.zeros(N, 3 * H), 3 * H + 12, 4)
    o.fill_(float("nan")), d.fill_(float("nan"))
    ops.xclip_fwd(q, o, Bc, S, heads)
    ops.xclip_bwd(q, g, d, Bc, S, heads)
    torch.cuda.synchronize()
    return dict(o=o, d_qkv=d), outside_untouched(ob, 4, H) and outside_untouched(db, 4, 3 * H)


@pytest.mark.parametrize("profile", ["sharp", "shift"])
@pytest.mark.parametrize("name", SAT.XCLIP_NAMES)
def test_xclip_where_the_softmax_saturates(ops, name, profile):
    p = SAT.xclip_problem(name, profile)
    case = p["case"]
    N = case["B"] * case["S"]
    got, untouched = _run_xclip(ops, p)
    again, _ = _run_xclip(ops, p)
    tag = f"xclip {name} {profile}"
    for n in ("o", "d_qkv"):
        held(tag, n, got[n], p["ref"][n].reshape(N, -1), SAT.rel_bound(n))
        if "flat" in p:
            held(tag, n + " vs unshifted", got[n], p["flat"][n].reshape(N, -1), SAT.rel_bound(n))
        assert torch.equal(got[n], again[n]), (tag, n)
    assert untouched, tag


# ---------------------------------------------------------------------------------------------------------------------
# B. row cross-entropies
# ---------------------------------------------------------------------------------------------------------------------
def held_loss(tag, name, got, want):
    """tests/loss_cases.py's margin for a loss: rtol 1e-4, atol 1e-6, element-wise"""
    a, b = torch.as_tensor(got).double().cpu().reshape(-1), torch.as_tensor(want).double().cpu().reshape(-1)
    bound = SAT.loss_bound(b, "loss")
    j = int(((a - b).abs() / bound).nan_to_num(float("inf")).argmax())        # the element nearest its bound
    print(f"[saturation] {tag} {name}: err {float((a - b).abs()[j]):.2e}, scale {float(b[j].abs()):.2e}, bound {float(bound[j]):.2e}, "
          f"got {a.tolist()}")
    assert bool(torch.isfinite(a).all()), f"{tag} {name}: not finite"
    assert bool(((a - b).abs() <= SAT.loss_bound(b, "loss")).all()), (tag, name, a.tolist(), b.tolist())


@pytest.mark.parametrize("profile", SAT.LOGIT_PROFILES)
@pytest.mark.parametrize("name", SAT.LOSS_CASES)
def test_loss_launch_where_the_logits_saturate(ops, name, profile):
    from tests import loss_cases as LC
    from tests.test_loss_optim_gpu import _Bufs, _same_bits, i64, SENT
    p = SAT.loss_problem(name, profile)
    c, t, ref = p["c"], p["t"], p["ref"]
    Bc, S, Q, K = c["B"], c["S"], c["Q"], c["K"]
    bufs = _Bufs(c, t)
    Ks = bufs.Ks
    ws = torch.zeros(ops.losses_ws_floats(Bc, S, Q), device="cuda")
    ticks = i64(0, 0)
    one = bufs.launch(ops, ws, ticks, kseg=c["Kseg"])
    two = bufs.launch(ops, ws, ticks, kseg=c["Kseg"])
    tag = f"losses {name} {profile}"
    d_seg, d_act, d_dur = one["d_seg"][:, :Ks], one["d_act"][:, :K], one["d_act"][:, K]
    for against, r in (("", ref),) + ((((" vs unshifted"), p["flat"]),) if "flat" in p else ()):
        held_loss(tag, "losses" + against, one["loss"], r["loss"])
        held(tag, "d_seg" + against, d_seg, r["d_seg"].reshape(Bc * S, Ks), 1e-3)
        held(tag, "d_act" + against, d_act, r["d_act"].reshape(Bc * Q, K), 1e-3)
        held(tag, "d_dur" + against, d_dur, r["d_dur"].reshape(Bc * Q), 1e-3)
    assert one["counts"].tolist() == ref["counts"], f"{tag}: counters"
    assert bool((one["d_act"][:, K + 1:] == SENT).all()) and bool((one["d_seg"][:, Ks:] == SENT).all()), tag
    ignored = ~ref["info"]["seg_valid"]
    assert float(d_seg[ignored].abs().max() if bool(ignored.any()) else 0.0) == 0.0, tag
    _same_bits(one, two, f"{tag}: second launch")
    if profile == "confident_right":                # the edited rows: a loss of 0 (or of one ulp of 50) and no gradient
        x0 = LC.make(c)["seg"].reshape(-1, Ks)
        edited = (t["seg"].reshape(-1, Ks) != x0).any(1)
        assert float(d_seg[edited].abs().max()) <= 1e-3 * max(float(ref["d_seg"].abs().max()), 1e-5), tag


@pytest.mark.parametrize("profile", SAT.LOGIT_PROFILES)
@pytest.mark.parametrize("rows,C,pad", SAT.CE_ROWS)
def test_ce_rows_where_the_logits_saturate(ops, rows, C, pad, profile):
    p = SAT.ce_problem(rows, C, pad, profile)
    assert ops.ce_rows_supported(rows, C)

    def run():
        x, xb = strided(p["x"], C + 5, 2)
        dx, dxb = strided(torch.zeros(rows, C), C + 7, 3)
        loss, counts = torch.full((4,), float("nan"), device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
        ops.ce_rows_fwd_bwd(x, p["tgt"].to(DEV), pad, loss, counts, dx)
        torch.cuda.synchronize()
        return loss, counts, dx, dxb
    loss, counts, dx, dxb = run()
    loss2, counts2, dx2, _ = run()
    tag = f"ce_rows {rows}x{C} {profile}"
    for against, r in (("", p["ref"]),) + (((" vs unshifted", p["flat"]),) if "flat" in p else ()):
        held_loss(tag, "loss" + against, loss[3], r["loss"])
        held(tag, "d_logits" + against, dx, r["d"], 1e-3)
    assert float(loss[1]) == float(loss[3]) and counts.tolist() == [0, 0] + p["ref"]["counts"], tag
    assert outside_untouched(dxb, 3, C), tag
    assert torch.equal(loss, loss2) and torch.equal(counts, counts2) and torch.equal(dx, dx2), tag
    assert not bool(dx.cpu()[p["tgt"] == pad].any()), tag


@pytest.mark.parametrize("profile", SAT.LOGIT_PROFILES)
@pytest.mark.parametrize("name", [c["name"] for c in SAT.FOCAL])
def test_focal_rows_where_the_logits_saturate(ops, name, profile):
    p = SAT.focal_problem(name, profile)
    case, ref = p["case"], p["ref"]
    N, C = p["pred"].shape

    def run():
        pd, _ = strided(p["pred"], C + 7, 3)
        dp, dpb = strided(torch.zeros(N, C), C + 8, 4)
        ws, loss = torch.full((N,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
        flags, counts = torch.zeros(N, dtype=torch.bool, device=DEV), torch.full((2,), -1, dtype=torch.int64, device=DEV)
        ops.focal_rows(pd, p["gold"].to(DEV), case["pad"], ws=ws, loss_out=loss, flags=flags, counts=counts, d_pred=dp,
                       exclude_idx=case["exclude"], alpha=case["alpha"], gamma=case["gamma"], penalty_weight=case["penalty"])
        torch.cuda.synchronize()
        return loss, flags, counts, dp, dpb
    loss, flags, counts, dp, dpb = run()
    loss2, flags2, counts2, dp2, _ = run()
    tag = f"focal {name} gamma {case['gamma']} alpha {case['alpha']} {profile}"
    for against, r in (("", ref),) + (((" vs unshifted", p["flat"]),) if "flat" in p else ()):
        held_loss(tag, "loss" + against, loss, r["loss"])
        held(tag, "d_pred" + against, dp, r["d"], 1e-3)
    assert torch.equal(flags.cpu(), ref["flags"]) and counts.tolist() == ref["counts"], tag      # the counters stay exact
    assert outside_untouched(dpb, 4, C), tag
    assert torch.equal(loss, loss2) and torch.equal(dp, dp2) and torch.equal(flags, flags2) and torch.equal(counts, counts2), tag
    assert not bool(dp.cpu()[~p["live"]].any()), tag


# ---------------------------------------------------------------------------------------------------------------------
# C. supervised contrastive loss at T = Tb = 0.01
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SAT.SUPCON_NAMES)
def test_supcon_at_low_temperature(ops, name):
    from tests import supcon_cases as SC
    from tests.test_supcon_gpu import _run, _layout
    p = SAT.supcon_problem(name)
    case, z, y, yo, ref = p["case"], p["z"], p["y"], p["yo"], p["ref"]
    N, D = z.shape
    A = p["kw"]["A"]
    loss, ws, dx, dxb = _run(ops, case, z, y)
    loss2, ws2, dx2, _ = _run(ops, case, z, y)
    torch.cuda.synchronize()
    tag = f"supcon {name}"
    held(tag, "loss", loss, ref["loss"].reshape(1), 1e-4)
    kept = torch.ones(A, dtype=torch.bool) if not case["ignore"] else (yo[:A] != SC.IGNORE)
    rows = kept & torch.isfinite(ref["lse"])
    wsc = ws.cpu()
    held(tag, "lse", wsc[:A][rows], ref["lse"][rows], 1e-4)
    held(tag, "gradient", dx, ref["d"], 1e-3)
    assert torch.equal(wsc[2 * N:2 * N + A][kept], ref["P"][kept].float()), f"{tag} P"
    assert outside_untouched(dxb, _layout(D)[1] + 1, D), tag
    assert torch.equal(loss, loss2) and torch.equal(dx, dx2) and torch.equal(ws.view(torch.int32), ws2.view(torch.int32)), tag
    if case["ignore"]:
        assert not bool(dx.cpu()[yo == SC.IGNORE].any()), tag


# ---------------------------------------------------------------------------------------------------------------------
# D. LSTM gates on their rails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,Bc,S,H", SAT.LSTM_CASES, ids=[f"{c[0]}-B{c[1]}-S{c[2]}-H{c[3]}" for c in SAT.LSTM_CASES])
def test_lstm_layer_with_gates_on_their_rails(ops, route, Bc, S, H):
    from tests import rnn_wide_cases as WC
    w, x, dy = SAT.lstm_inputs(Bc, S, H)
    if route == "registers":
        from tests.test_rnn_gpu import _run_layer
        assert ops.lstm_supported(H)
        run = lambda: _run_layer(Bc, S, H, w, x, dy)          # noqa: E731
    else:
        from tests.test_rnn_wide_gpu import _run_layer_steps
        assert ops.lstm_steps_supported(H)
        run = lambda: _run_layer_steps(Bc, S, H, w, x, dy)    # noqa: E731

    def flat(r):
        if isinstance(r["dw_hh"], list):
            r["dw_hh"], r["db_hh"] = torch.cat(r["dw_hh"], 0), torch.cat(r["db_hh"])
        return r
    got, again = flat(run()), flat(run())
    SAT.lstm_check(got, Bc, S, H, route)
    for k in WC.TENSORS:
        t = got[k]
        assert bool(torch.isfinite(t).all()), (route, k)
        assert torch.equal(t, again[k]), (route, k)
        # no denormal storm: a saturated i(1 - i) or 1 - g^2 gives 0 or a normal float32, and what the gradients
        # accumulate from them stays normal
        tiny = (t != 0) & (t.abs() < torch.finfo(torch.float32).tiny)
        assert int(tiny.sum()) <= t.numel() // 100, (route, k, int(tiny.sum()))
