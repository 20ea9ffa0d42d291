"""The L3 query model's kernels on the GPU against the float64 restatement (tests/l3_oracle.py) over tests/l3_cases.py: the
cross-clip attention (csrc/attention_xclip.hip) forward and backward -- contiguous and strided rows, the same bits on a second
call, graph capture, the refusals -- and the loss mix (csrc/l3mix.hip): flags and m exactly, the weights, the total and the
scaled gradients.  Needs an MI355X.  Tolerances: tests/l3_cases.py (8 x the float32 restatement's error per case)."""
import numpy as np
import pytest
import torch

from r3d_amd import engine_l3, train_unsupervised  # noqa: F401  (the feature under test: without it nothing here is collected)
from tests import l3_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from tests.test_query_kernels_gpu import strided, outside_untouched  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


# ---------------------------------------------------------------------------------------------------------------------
# cross-clip attention
# ---------------------------------------------------------------------------------------------------------------------
def _xclip(ops, case, layout="dense"):
    """(o, d_qkv, buffers) of a case through the C ABI.  layout "strided": qkv, d_o, o and d_qkv are column slices of wider
    NaN-filled buffers -- 16-byte aligned where H % 4 == 0 (the 16-byte loads), an odd stride and offset otherwise."""
    qkv, d_o = LC.xclip_inputs(case)
    B, S, H, heads = case["B"], case["S"], case["H"], case["heads"]
    N = B * S
    if layout == "dense":
        q, g = qkv.reshape(N, 3 * H).to(DEV), d_o.reshape(N, H).to(DEV)
        o = torch.full((N, H), float("nan"), device=DEV)
        d = torch.full((N, 3 * H), float("nan"), device=DEV)
        bufs = None
    else:
        pad, c0 = (8, 4) if layout == "strided" else (7, 3)
        q, _ = strided(qkv.reshape(N, 3 * H), 3 * H + pad, c0)
        g, _ = strided(d_o.reshape(N, H), H + pad, c0)
        o, ob = strided(torch.zeros(N, H), H + pad + 4, c0)
        d, db = strided(torch.zeros(N, 3 * H), 3 * H + pad + 4, c0)
        o.fill_(float("nan")), d.fill_(float("nan"))
        bufs = (ob, db, c0)
    ops.xclip_fwd(q, o, B, S, heads)
    ops.xclip_bwd(q, g, d, B, S, heads)
    return o, d, bufs


def _check(case, o, d):
    ref = LC.xclip_reference(case["name"])
    N = case["B"] * case["S"]
    eo, ed = LC.rel_err(o.cpu().reshape(N, -1), ref["o"].reshape(N, -1)), LC.rel_err(d.cpu().reshape(N, -1), ref["d_qkv"].reshape(N, -1))
    print(f"{case['name']}: o err {eo:.3e} (tol {ref['tol_o']:.3e})  d_qkv err {ed:.3e} (tol {ref['tol_d']:.3e})")
    assert not torch.isnan(o).any() and not torch.isnan(d).any()       # (every element written)
    assert eo <= ref["tol_o"], (case["name"], "o", eo, ref["tol_o"])
    assert ed <= ref["tol_d"], (case["name"], "d_qkv", ed, ref["tol_d"])


@pytest.mark.parametrize("name", [c["name"] for c in LC.XCLIP])
def test_xclip_matches_float64(ops, name):
    case = LC.XCLIP_BY_NAME[name]
    o, d, _ = _xclip(ops, case)
    _check(case, o, d)
    o2, d2, _ = _xclip(ops, case)
    assert torch.equal(o, o2) and torch.equal(d, d2)                   # the same call, the same bits


STRIDED = [c["name"] for c in LC.XCLIP if (c["B"], c["S"]) in ((8, 5), (13, 64), (13, 200), (2, 64), (2, 200), (64, 1), (33, 5))]


@pytest.mark.parametrize("layout", ["strided", "odd"])
@pytest.mark.parametrize("name", STRIDED)
def test_xclip_strided_views(ops, name, layout):
    case = LC.XCLIP_BY_NAME[name]
    o, d, (ob, db, c0) = _xclip(ops, case, layout)
    _check(case, o, d)
    assert outside_untouched(ob, c0, case["H"]) and outside_untouched(db, c0, 3 * case["H"])
    dense_o, dense_d, _ = _xclip(ops, case)
    assert torch.equal(o, dense_o) and torch.equal(d, dense_d)        # (the layout changes no sum)


def test_xclip_reads_the_in_projection_columns_in_place(ops):
    """qkv as the engine holds it: the three parts of one [N, 3 H] GEMM output, and q / k / v taken from its columns"""
    case = LC.XCLIP_BY_NAME["B8_S5_H128_h8"] if "B8_S5_H128_h8" in LC.XCLIP_BY_NAME else LC.XCLIP_BY_NAME["B8_S1_H128_h8"]
    qkv, _ = LC.xclip_inputs(case)
    B, S, H, heads = case["B"], case["S"], case["H"], case["heads"]
    q = qkv.reshape(B * S, 3 * H).to(DEV)
    o = torch.empty(B * S, H, device=DEV)
    ops.xclip_fwd(q, o, B, S, heads)
    dh = H // heads
    x = q.view(B, S, 3, heads, dh).permute(1, 3, 2, 0, 4)               # [S, heads, 3, B, dh]
    p = torch.softmax((x[:, :, 0].double() @ x[:, :, 1].double().transpose(-1, -2)) / np.sqrt(dh), -1)
    want = (p @ x[:, :, 2].double()).permute(2, 0, 1, 3).reshape(B * S, H)
    assert LC.rel_err(o.cpu(), want.cpu()) <= LC.xclip_reference(case["name"])["tol_o"]


def test_xclip_graph_capture(ops):
    case = LC.XCLIP_BY_NAME["B13_S64_H136_h4"] if "B13_S64_H136_h4" in LC.XCLIP_BY_NAME else LC.XCLIP[-1]
    eager_o, eager_d, _ = _xclip(ops, case)
    qkv, d_o = LC.xclip_inputs(case)
    B, S, H, heads = case["B"], case["S"], case["H"], case["heads"]
    q, g = qkv.reshape(B * S, 3 * H).to(DEV), d_o.reshape(B * S, H).to(DEV)
    o, d = torch.zeros(B * S, H, device=DEV), torch.zeros(B * S, 3 * H, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.xclip_fwd(q, o, B, S, heads)                                # (warm-up outside the capture: function attributes)
        ops.xclip_bwd(q, g, d, B, S, heads)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.xclip_fwd(q, o, B, S, heads)
        ops.xclip_bwd(q, g, d, B, S, heads)
    for _ in range(2):
        o.zero_(), d.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager_o) and torch.equal(d, eager_d)


def test_xclip_refusals(ops):
    from r3d_amd._lib import R3DHipError
    assert not ops.xclip_supported(65, 16) and not ops.xclip_supported(8, 256)
    o = torch.full((65 * 2, 32), 3.0, device=DEV)
    with pytest.raises(ValueError, match="64"):
        ops.xclip_fwd(torch.zeros(65 * 2, 96, device=DEV), o, 65, 2, 2)
    with pytest.raises(ValueError, match="128"):
        ops.xclip_fwd(torch.zeros(4, 3 * 256, device=DEV), torch.zeros(4, 256, device=DEV), 2, 2, 1)
    with pytest.raises(ValueError, match="heads"):
        ops.xclip_fwd(torch.zeros(4, 3 * 10, device=DEV), torch.zeros(4, 10, device=DEV), 2, 2, 4)
    # the C entry point's own check, before anything is enqueued
    lib = ops._lib.load()
    rc = lib.r3d_xclip_fwd(o.data_ptr(), 96, o.data_ptr(), 32, 65, 2, 2, 16, None)
    assert rc == -1
    rc = lib.r3d_xclip_bwd(o.data_ptr(), 768, o.data_ptr(), 256, o.data_ptr(), 768, 2, 2, 1, 256, None)
    assert rc == -1
    # B S 3 H >= 2^31: the wrapper's check reads the shape alone (a storage-less tensor stands in for 8 GiB), the C entry point
    # returns before it touches a pointer or enqueues
    B, S, heads, dh = 64, 5462, 16, 128
    assert B * S * 3 * heads * dh >= 2 ** 31 > B * (S - 1) * 3 * heads * dh
    big = torch.empty(B * S, 3 * heads * dh, device="meta")
    with pytest.raises(ValueError, match="2\\^31"):
        ops.xclip_fwd(big, torch.empty(B * S, heads * dh, device="meta"), B, S, heads)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.xclip_bwd(big, torch.empty(B * S, heads * dh, device="meta"), big, B, S, heads)
    H = heads * dh
    assert lib.r3d_xclip_fwd(o.data_ptr(), 3 * H, o.data_ptr(), H, B, S, heads, dh, None) == -1
    assert lib.r3d_xclip_bwd(o.data_ptr(), 3 * H, o.data_ptr(), H, o.data_ptr(), 3 * H, B, S, heads, dh, None) == -1
    assert lib.r3d_xclip_fwd(o.data_ptr(), 96, o.data_ptr(), 32, 2, 0, 2, 16, None) == -1                # S = 0
    torch.cuda.synchronize()
    assert bool((o == 3.0).all())
    assert issubclass(R3DHipError, RuntimeError)


# ---------------------------------------------------------------------------------------------------------------------
# mix
# ---------------------------------------------------------------------------------------------------------------------
def _mix(ops, case, c):
    N, K = c["seg"].shape
    seg, _ = strided(torch.from_numpy(c["seg"]), K + 3, 1)
    d_seg, dsb = strided(torch.from_numpy(c["d_seg"]), K + 5, 2)
    d_ad, dab = strided(torch.from_numpy(c["d_actdur"]), c["d_actdur"].shape[1] + 1, 1)
    L3, Lc, Lseg, Lact, Ldur = (float(v) for v in c["losses"])
    t = lambda *v: torch.tensor(v, dtype=torch.float32, device=DEV)     # noqa: E731
    loss3 = t(Lseg, Lact, Ldur, Lseg + Lact + Ldur)
    out = torch.full((5,), float("nan"), device=DEV)
    l2 = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.full((ops.l3mix_ws_ints(N),), -12345, dtype=torch.int32, device=DEV)
    ops.l3mix(seg, torch.from_numpy(c["label"]).to(DEV), torch.from_numpy(c["l3"]).to(DEV), c["pad"], t(L3), t(Lc), loss3,
              t(case["wf"]), ws, out, d_seg=d_seg, d_actdur=d_ad, l2_flags=l2)
    return out.cpu().numpy(), l2.cpu().numpy().astype(bool), d_seg.cpu().numpy(), d_ad.cpu().numpy(), (dsb, dab)


@pytest.mark.parametrize("name", [c["name"] for c in LC.MIX])
def test_mix_matches_float64(ops, name):
    case = LC.MIX_BY_NAME[name]
    c, ref = LC.mix_reference(case)
    out, l2, d_seg, d_ad, (dsb, dab) = _mix(ops, case, c)
    print(name, "out", out, "ref", ref["m"], ref["a"], ref["b"], ref["c"], ref["total"])
    assert (l2 == ref["l2_correct"]).all()                                   # flags: exactly, every row
    assert out[0] == ref["m"]                                                # m: exactly
    for i, k in ((1, "a"), (2, "b"), (3, "c")):
        assert abs(float(out[i]) - float(ref[k])) <= LC.SCALAR_TOL, (k, out[i], ref[k])
    assert abs(float(out[4]) - float(ref["total"])) <= LC.SCALAR_TOL * float(np.abs(c["losses"]).sum())
    if case["kind"] == "all":
        assert out[0] == 1.0 and out[1] == 0.0 and out[2] == 0.0 and out[3] == 1.0
        assert (d_seg == c["d_seg"]).all() and (d_ad == c["d_actdur"]).all()
    if case["kind"] == "none":
        assert out[0] == 5.0
    for got, d in ((d_seg, c["d_seg"]), (d_ad, c["d_actdur"])):
        want = d.astype(np.float64) * float(ref["c"])
        assert (np.abs(got - want) <= LC.GRAD_TOL * np.abs(want) + 1e-45).all()
    K = case["Kseg"]
    assert outside_untouched(dsb, 2, K) and outside_untouched(dab, 1, c["d_actdur"].shape[1])
    again = _mix(ops, case, c)
    assert (again[0] == out).all() and (again[2] == d_seg).all() and (again[3] == d_ad).all()      # the same bits


def test_mix_weights_drive_the_loss_backward_launches(ops):
    """a and b are device scalars in the form focal_rows(d_pred=...) and tcluster_bwd(add=True) take as d_loss"""
    case = LC.MIX_BY_NAME["n65"]
    c, ref = LC.mix_reference(case)
    N, C = 65, 49
    out = torch.from_numpy(_mix(ops, case, c)[0]).to(DEV)
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(N, C, generator=g).to(DEV)
    gold = torch.randint(0, C - 2, (N,), generator=g).to(DEV)
    d_one, d_a = torch.empty(N, C, device=DEV), torch.empty(N, C, device=DEV)
    ops.focal_rows(pred, gold, 47, exclude_idx=48, d_pred=d_one)
    ops.focal_rows(pred, gold, 47, exclude_idx=48, d_pred=d_a, d_loss=out[1:2])
    want = d_one.double() * float(ref["a"])
    assert float((d_a.double() - want).abs().max()) <= 4 * LC.EPS32 * float(want.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# whole step: the engine against the float64 restatement and the fixtures made from the reference
# ---------------------------------------------------------------------------------------------------------------------
import argparse  # noqa: E402

from tests.helpers import load_fixture, fixture_params, stats  # noqa: E402

STEP_TAGS = [c["tag"] for c in LC.STEP_CASES]
LOSS_KEYS = ("L3", "Lc", "Lseg", "Lact", "Ldur", "total")


def step_batch(fx):
    c = LC.STEP_BY_TAG[fx["meta"]["tag"]]
    b = LC.batch(c, fx["meta"]["seed"])
    b[1], b[4] = torch.from_numpy(fx["past_label"]), torch.from_numpy(fx["query_label"])
    return c, b


def build_model(fx, dropout=False):
    from r3d_amd.model.futr_unsupervised_temp3 import FUTR
    m = fx["meta"]
    args = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    model = FUTR(m["n_class"], m["H"], m["pad_idx"], torch.device("cuda"), args, n_query=8, n_head=m["n_head"],
                 num_encoder_layers=2, num_decoder_layers=m["n_dec"], query_num=m["query_num"])
    missing = model.load_state_dict(fixture_params(fx), strict=False)
    assert not missing.unexpected_keys and all("pos_table" in k for k in missing.missing_keys)
    model.r3d_dropout_enabled = dropout
    return model.to("cuda")


def _rel(got, ref, tol, what):
    err = LC.rel_err(torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach())
    print(f"  {what}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("wi", [0, 1, 2])
@pytest.mark.parametrize("tag", STEP_TAGS)
def test_step_matches_float64_and_the_reference_fixture(tag, wi):
    fx = load_fixture(tag)
    m = fx["meta"]
    c, b = step_batch(fx)
    wf = LC.WFS[wi]
    p0 = fixture_params(fx)
    ref = LC.step_reference(c, b, p0, wf)
    tol, res = ref["tol"], ref["res"]
    model = build_model(fx).eval()
    eng = model.engine()
    d = [t.cuda() for t in b]
    eng.set_wf(wf)
    out = eng.forward(d[0], d[1], "train", training=False)
    mix, loss3, l_l3, l_lc, counts, l3_counts = eng.losses(d[1], d[3], d[2], d[4])
    eng.backward()
    torch.cuda.synchronize()
    w = eng.last["w"]
    B, S = m["B"], m["S"]
    # ---- outputs
    for k in ("action", "duration", "seg", "l3"):
        _rel(out[k], ref["out"][k], tol[k], f"{tag}/{k}")
        fk = fx["out_" + k]
        if fk.shape == tuple(out[k].shape):
            _rel(out[k], fk, tol[k] + 8 * LC.EPS32, f"{tag}/{k} vs fixture")          # (the fixture is the reference's float32)
        else:
            assert abs(stats(out[k])[0] - fk[0]) <= (tol[k] + 8 * LC.EPS32) * fk[0] * np.sqrt(out[k].numel()), k
    # ---- flags, counters and m: exactly, no row left out
    assert (w.l3_flags.cpu().numpy().astype(bool) == fx["l3_correct"]).all()
    assert (w.l2_flags.cpu().numpy().astype(bool) == fx["l2_correct"]).all()
    assert counts.cpu().tolist() + l3_counts.cpu().tolist() == fx["counts"].tolist()
    mixc = mix.cpu().numpy()
    assert mixc[0] == fx["m"] == np.float32(float(res["m"]))
    assert 1.0 < mixc[0] < 5.0
    # ---- the five losses and the total
    got = dict(L3=l_l3[0], Lc=l_lc[0], Lseg=loss3[0], Lact=loss3[1], Ldur=loss3[2], total=mix[4])
    for i, k in enumerate(LOSS_KEYS):
        _rel(got[k], res[k], tol[k], f"{tag}/wf{wi}/{k}")
        assert abs(float(got[k]) - fx[f"losses_wf{wi}"][i]) <= (tol[k] + 8 * LC.EPS32) * abs(fx[f"losses_wf{wi}"][i]), k
    for i, k in ((1, "a"), (2, "b"), (3, "c")):
        assert abs(float(mixc[i]) - float(res[k])) <= LC.SCALAR_TOL, k
    # ---- gradients of every live parameter; dead parameters have none
    live = fx["live_names"]
    assert sorted(live) == sorted(n for n in fx["param_names"] if eng.arena.is_live(n)) == sorted(ref["live"])
    for n in live:
        g = eng.arena.g(n)
        gref = ref["grads"][n]
        if n == "pos_embedding":
            assert float(g[:, S:].abs().max()) == 0.0
            g, gref = g[:, :S], gref[:, :S]
        _rel(g, gref, tol["grad::" + n], f"{tag}/wf{wi}/grad {n}")
        full = fx.get(f"grad_wf{wi}::" + n)
        if full is not None and n != LC.ZERO_GRAD:
            _rel(g.reshape(full.shape), full, tol["grad::" + n] + 8 * LC.EPS32, f"{tag}/wf{wi}/grad {n} vs fixture")
    gs = np.stack([stats(eng.arena.g(n)) for n in live])
    fref = fx[f"grad_stats_wf{wi}"]
    gt = np.array([tol["grad::" + n] for n in live])
    numel = np.array([eng.arena.g(n).numel() for n in live])
    # |(|g| - |g_ref|)| <= |g - g_ref| <= sqrt(numel) max|g - g_ref|, and max|g_ref| <= |g_ref|
    keep = np.array([n != LC.ZERO_GRAD for n in live])         # (fc_len.bias: true gradient 0, rounding noise on both sides)
    assert bool((np.abs(gs[:, 0] - fref[:, 0]) <= (gt + 8 * LC.EPS32) * np.sqrt(numel) * fref[:, 0] + 1e-30)[keep].all()), "grad norms vs fixture"
    # ---- one AdamW step (the fixture's is taken at wf = 1/30)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    n_moved = 0
    eng.adamw(m["lr"], m["wd"])
    torch.cuda.synchronize()
    for n in live:
        p = eng.arena.p(n)
        if n == "pos_embedding":
            p = p[:, :S]
        over = (p.detach().cpu().double() - ref["post"][n]).abs() - tol["post::" + n]       # (element-wise: LC.post_tolerance)
        assert float(over.max()) <= 0.0, (n, float(over.max()))
        moved = (p.detach().cpu().double() - p0[n][:, :S].double() if n == "pos_embedding" else p.detach().cpu().double() - p0[n].double()).abs()
        n_moved += float(moved.max()) > 0.5 * m["lr"]
    assert n_moved >= len(live) - 2      # (the step was taken; fc_len.bias has a zero true gradient: the duration is normalised)
    for n in fx["param_names"]:
        if n not in live:
            assert torch.equal(dict(model.named_parameters())[n], before[n]) and torch.equal(before[n].cpu(), p0[n]), n
    assert bool(fx["dead_unchanged"].all())
    assert int(eng.step_t.item()) == 1


@pytest.mark.parametrize("tag", STEP_TAGS)
def test_graphed_step_equals_eager_bit_for_bit(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    c, b = step_batch(fx)
    d = [t.cuda() for t in b]
    wf = LC.WFS[1]

    def run(graphed, steps):
        model = build_model(fx).eval()
        eng = model.engine()
        outs = []
        for i in range(steps):
            fn = eng.train_step_graphed if graphed else eng.train_step
            mix = fn(d[0], d[1], d[2], d[3], d[4], m["lr"], m["wd"], wf if i == 0 else LC.WFS[2], training=False)[0]
            outs.append(mix.clone())
        torch.cuda.synchronize()
        return eng, outs

    e_eng, e_out = run(False, 2)
    g_eng, g_out = run(True, 2)
    for a, bb in zip(e_out, g_out):
        assert torch.equal(a, bb)
    n = e_eng.arena.n_live
    assert torch.equal(e_eng.arena.params, g_eng.arena.params) and torch.equal(e_eng.arena.grads[:n], g_eng.arena.grads[:n])
    assert torch.equal(e_eng.arena.exp_avg, g_eng.arena.exp_avg) and torch.equal(e_eng.arena.exp_avg_sq, g_eng.arena.exp_avg_sq)
    assert int(g_eng.step_t.item()) == 2 and len(g_eng.graphs) == 1          # (wf changed between the steps: no new capture)
    # a replay equals itself: the same state and batch give the same bits
    g2, g2_out = run(True, 2)
    assert torch.equal(g2.arena.params, g_eng.arena.params) and torch.equal(g2_out[1], g_out[1])


@pytest.mark.parametrize("tag", STEP_TAGS)
def test_test_mode_forward_matches_the_fixture(tag):
    fx = load_fixture(tag)
    c, b = step_batch(fx)
    p0 = fixture_params(fx)
    from tests import l3_oracle as LO
    o64, _ = LO.forward({n: v.double() for n, v in p0.items()}, b[0], "test", fx["meta"]["pad_idx"], c["n_head"], c["n_dec"], 8)
    o32, _ = LO.forward({n: v.float() for n, v in p0.items()}, b[0], "test", fx["meta"]["pad_idx"], c["n_head"], c["n_dec"], 8)
    model = build_model(fx).eval()
    with torch.no_grad():
        out = model(b[0].cuda(), b[4].cuda(), mode="test")
    assert set(out) == {"action", "duration", "seg", "l3"}
    for k in out:
        tol = LC.MARGIN * LC.rel_err(o32[k], o64[k])
        _rel(out[k], o64[k], tol, f"{tag}/test/{k}")
        fk = fx["test_" + k]
        if fk.shape == tuple(out[k].shape):
            _rel(out[k], fk, tol + 8 * LC.EPS32, f"{tag}/test/{k} vs fixture")


def test_autograd_bridge():
    fx = load_fixture("l3_tiny")
    c, b = step_batch(fx)
    p0 = fixture_params(fx)
    from tests import l3_oracle as LO
    model = build_model(fx).eval()
    d = [t.cuda() for t in b]
    out = model((d[0], d[1]), d[4])
    f = lambda o: (o["seg"] ** 2).mean() + o["action"].sum() * 0.01 + (o["duration"] * 0.1).exp().mean() + (o["l3"] ** 2).mean()   # noqa: E731
    f(out).backward()
    torch.cuda.synchronize()
    p = {n: v.double().requires_grad_(True) for n, v in p0.items()}
    oo, _ = LO.forward(p, (b[0], b[1]), "train", fx["meta"]["pad_idx"], c["n_head"], c["n_dec"], 8)
    f(oo).backward()
    for n, q in model.named_parameters():
        if p[n].grad is None:
            assert q.grad is None, n
        else:
            g, gr = (q.grad[:, :c["S"]], p[n].grad[:, :c["S"]]) if n == "pos_embedding" else (q.grad, p[n].grad)
            assert LC.rel_err(g.cpu(), gr) <= 1e-4, n


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_engine_refusals():
    from r3d_amd import engine_l3 as E
    fx = load_fixture("l3_tiny")
    model = build_model(fx).eval()
    eng = model.engine()
    H, D = fx["meta"]["H"], 2048
    z = lambda B, S: (torch.zeros(B, S, D, device=DEV), torch.zeros(B, S, dtype=torch.int64, device=DEV))     # noqa: E731
    with pytest.raises(ValueError, match="1 to 64"):
        eng.forward(*z(65, 2), "train")
    with pytest.raises(ValueError, match="max_pos_len"):
        eng.forward(*z(2, 2001), "train")
    with pytest.raises(ValueError, match="at least one frame"):
        eng.forward(*z(2, 0), "train")
    with pytest.raises(ValueError, match="1 to 64"):
        eng.forward(*z(0, 3), "train")
    with pytest.raises(ValueError, match="2\\^31"):
        E.check_l3_batch(64, 5462, 2048, 16, 8, 10 ** 6, True)
    E_ok = 64 * 5461 * 3 * 2048
    assert E_ok < 2 ** 31
    for bad, pat in (((132, 8, 8, 49, 17), "hidden % 8"), ((120, 7, 8, 49, 17), "n_head"), ((2056, 8, 8, 49, 17), "2048"),
                     ((1032, 8, 8, 49, 17), "128"), ((1024, 8, 16, 49, 17), "1024"), ((128, 8, 8, 257, 17), "256"),
                     ((128, 8, 8, 49, 1024), "1023")):
        with pytest.raises(ValueError, match=pat):
            E.check_l3_shape(*bad)
    E.check_l3_shape(128, 8, 8, 49, 17)
    longest = E.max_clip_len(128, 8, 8, 2000, True)
    with pytest.raises(ValueError, match="scores"):
        E.check_l3_batch(8, longest + 1, 128, 8, 8, 10 ** 6, True)
    E.check_l3_batch(8, longest, 128, 8, 8, 2000, True)
    assert not eng.shapes or all(k[0] <= 64 for k in eng.shapes)                 # (nothing was allocated for a refused batch)


# ---------------------------------------------------------------------------------------------------------------------
# train() / validate() against the reference's own run (tests/golden/l3_train_loop.npz)
# ---------------------------------------------------------------------------------------------------------------------
import contextlib  # noqa: E402
import io  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402
import re  # noqa: E402

_NUM = re.compile(r"-?\d+\.\d+(?:e-?\d+)?|-?\d+")


def _loop_args(epochs):
    return argparse.Namespace(epochs=epochs, seg=True, anticipate=True, task="long", input_type="i3d_transcript", graph_steps=True)


class _NoSched:
    def step(self):
        pass


def _loop_data(fx):
    train, val = LC.loop_data(LC.STEP_BY_TAG["l3_tiny"], fx["meta"]["seed"])
    val[0][3] = torch.from_numpy(fx["val_target"])               # (the future labels the fixture's generator chose)
    return train, val


@pytest.mark.parametrize("flat", [True, False])
def test_train_loop_matches_the_reference_run(tmp_path, flat):
    from r3d_amd import train_unsupervised as TU
    from r3d_amd.optim import FlatAdamW
    fx = load_fixture("l3_train_loop")
    m = fx["meta"]
    model = build_model(fx)                                       # (dropout off, as in the fixture's run)
    train, val = _loop_data(fx)
    opt = (FlatAdamW if flat else torch.optim.AdamW)(model.parameters(), m["lr"], weight_decay=m["wd"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TU.train(_loop_args(m["epochs"]), model, train, opt, _NoSched(), torch.nn.MSELoss(reduction="none"), str(tmp_path),
                 m["pad_idx"], torch.device(DEV), val, m["seed"])
    got, want = buf.getvalue().splitlines(), json.loads(str(fx["stdout"])).splitlines()
    print("\n".join(got))
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert _NUM.sub("#", g) == _NUM.sub("#", w), (g, w)
        for a, b in zip([float(x) for x in _NUM.findall(g)], [float(x) for x in _NUM.findall(w)]):
            assert abs(a - b) <= 2e-3 * max(1.0, abs(b)) + 1e-3, (g, w)          # (the printed digits: test_cnn_gpu's bound)
    assert sorted(os.listdir(tmp_path)) == fx["ckpt_files"] and fx["ckpt_files"]
    keys = list(torch.load(os.path.join(tmp_path, fx["ckpt_files"][0]), weights_only=True).keys())
    assert keys == fx["ckpt_keys"]
    with contextlib.redirect_stdout(io.StringIO()):
        vres = TU.validate(model, val, torch.nn.MSELoss(reduction="none"), m["pad_idx"], torch.device(DEV))
    assert np.abs(np.array(vres) - fx["val_result"]).max() <= 2e-3 * max(1.0, float(np.abs(fx["val_result"]).max()))
    assert not model.training                                     # (validate leaves the model in eval(); train never switches back)
    eng = model.engine()
    if flat:
        assert len(eng.graphs) == 1          # (dropout off throughout: one capture served the three epochs' warm-up factors)
    for j, n in enumerate(fx["live_names"]):
        if n == "fc_len.bias":
            continue
        ps, want = stats(eng.arena.p(n)), fx["post_stats"][j]
        assert abs(ps[0] - want[0]) <= 2e-3 * max(1.0, float(want[0])), (n, ps[0], want[0])


def test_loop_refusals(tmp_path, monkeypatch):
    from r3d_amd import train_unsupervised as TU
    fx = load_fixture("l3_train_loop")
    m = fx["meta"]
    model = build_model(fx)
    train, val = _loop_data(fx)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    for kw, pat in ((dict(seg=False), "NameError"), (dict(anticipate=False), "NameError"), (dict(erank_weight=0.1), "erank_weight"),
                    (dict(measure_rank=True), "measure_rank"), (dict(erank_report=True), "erank_report"),
                    (dict(supcon_weight=0.5), "supcon_weight")):
        args = _loop_args(1)
        for k, v in kw.items():
            setattr(args, k, v)
        with pytest.raises(ValueError, match=pat):
            TU.train(args, model, train, torch.optim.AdamW(model.parameters(), 1e-3), _NoSched(), None, str(tmp_path), m["pad_idx"],
                     torch.device(DEV), val, 1)
    # a data-parallel run: the process group's size is all the check reads
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(ValueError, match="one GPU"):
        TU.train(_loop_args(1), model, train, torch.optim.AdamW(model.parameters(), 1e-3), _NoSched(), None, str(tmp_path),
                 m["pad_idx"], torch.device(DEV), val, 1)
    monkeypatch.undo()
    with pytest.raises(TypeError, match="futr_unsupervised_temp3"):
        TU.train(_loop_args(1), torch.nn.Linear(2, 2), train, None, _NoSched(), None, str(tmp_path), m["pad_idx"], torch.device(DEV), val, 1)
    assert not os.listdir(tmp_path)
    assert all(torch.equal(p.detach().cpu(), before[n].cpu()) for n, p in model.named_parameters())      # nothing ran


# ---------------------------------------------------------------------------------------------------------------------
# the dropout-on step: what every run takes for its first epoch (model.train() holds until validate() switches to eval())
# ---------------------------------------------------------------------------------------------------------------------
def test_dropout_on_step_and_training_epoch(tmp_path):
    from r3d_amd import train_unsupervised as TU
    from r3d_amd.optim import FlatAdamW
    from r3d_amd.engine import DROP_P
    fx = load_fixture("l3_cfg")
    m = fx["meta"]
    c, b = step_batch(fx)
    d = [t.cuda() for t in b]
    # ---- the masks: Philox keep rate on the encoding's dropout, and what it leaves of the memory
    model = build_model(fx, dropout=True).train()
    eng = model.engine()
    eng.forward(d[0], d[1], "train", training=True)
    torch.cuda.synchronize()
    w = eng.last["w"]
    assert eng.last["drop"]
    n = w.drop["pe_rgb"].numel()
    sd = (DROP_P * (1 - DROP_P) / n) ** 0.5
    assert abs(float(w.drop["pe_rgb"].float().mean()) - (1 - DROP_P)) < 6 * sd           # (six standard deviations of the rate)
    # (+ the exact zeros the encoding itself leaves: sin(0) = 0 on frame 0's even columns wherever the ReLU is shut, under 2 %)
    assert -6 * sd < float((w.mem == 0).float().mean()) - DROP_P < 6 * sd + 0.02
    for k, v in w.drop.items():
        assert abs(float(v.float().mean()) - (1 - DROP_P)) < 6 * (DROP_P * (1 - DROP_P) / v.numel()) ** 0.5 + 1e-9, k
    kept = w.mem != 0
    eng.forward(d[0], d[1], "train", training=False)                                       # the same model without the masks
    torch.cuda.synchronize()
    assert not eng.last["drop"] and float((w.mem == 0).float().mean()) < 0.02
    # ---- eager and graphed steps at the same seed and offset: the same bits; the offset advances once per step
    def run(graphed):
        mod = build_model(fx, dropout=True).train()
        e = mod.engine()
        offs, outs = [int(e.drop_offset.item())], []
        for i in range(3):
            fn = e.train_step_graphed if graphed else e.train_step
            outs.append(fn(d[0], d[1], d[2], d[3], d[4], m["lr"], m["wd"], LC.WFS[1], training=True)[0].clone())
            offs.append(int(e.drop_offset.item()))
        torch.cuda.synchronize()
        return e, offs, outs
    e_eng, e_off, e_out = run(False)
    g_eng, g_off, g_out = run(True)
    assert e_off == g_off == [0, 1, 2, 3]
    assert all(torch.equal(a, bb) for a, bb in zip(e_out, g_out))
    assert torch.equal(e_eng.arena.params, g_eng.arena.params) and torch.equal(e_eng.arena.exp_avg_sq, g_eng.arena.exp_avg_sq)
    assert torch.equal(e_eng.last["w"].drop_pool, g_eng.shapes[(m["B"], m["S"], True)].drop_pool)
    assert not torch.equal(e_out[0], e_out[1])                                             # (another offset: other masks)
    assert len(g_eng.graphs) == 1 and next(iter(g_eng.graphs))[5] is True                  # the dropout-on graph key
    assert all(torch.isfinite(o).all() for o in e_out)
    # the masked step differs from the unmasked one on the same state (the masks reach the loss)
    clean = build_model(fx, dropout=True).train().engine()
    ref = clean.train_step(d[0], d[1], d[2], d[3], d[4], m["lr"], m["wd"], LC.WFS[1], training=False)[0]
    assert not torch.equal(ref, e_out[0]) and int(clean.drop_offset.item()) == 0           # (no tick of the offset without masks)
    assert bool(kept.any())
    # ---- train(): epoch 1 with model.training True and dropout on, epoch 2 after validate() left the model in eval()
    lfx = load_fixture("l3_train_loop")
    model = build_model(lfx, dropout=True)
    train, val = _loop_data(lfx)
    opt = FlatAdamW(model.parameters(), lfx["meta"]["lr"], weight_decay=lfx["meta"]["wd"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TU.train(_loop_args(2), model, train, opt, _NoSched(), torch.nn.MSELoss(reduction="none"), str(tmp_path),
                 lfx["meta"]["pad_idx"], torch.device(DEV), val, 1)
    log = buf.getvalue()
    leng = model.engine()
    assert "Epoch [ 1 / 2 ]" in log and "Epoch [ 2 / 2 ]" in log and log.count("Validation Loss") == 2 and "nan" not in log
    assert sorted(k[5] for k in leng.graphs) == [False, True]       # one capture with dropout, one after eval()
    assert int(leng.drop_offset.item()) == 2 and int(leng.step_t.item()) == 4              # 2 masked steps, 4 steps in all
    ref_lines = json.loads(str(lfx["stdout"])).splitlines()
    assert _NUM.findall(log.splitlines()[1])[-1] != _NUM.findall(ref_lines[1])[-1]         # (epoch 1 is not the dropout-free run)
