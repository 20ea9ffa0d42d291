"""The temporal auxiliary loss kernels (csrc/temporal.hip) against the float64 restatement (tests/temporal_oracle.py) over
tests/temporal_cases.py: run structures (one run, all singletons, boundaries at the tile edges, a length-1 run at a start > 0,
the in-run diagonal, different structures per clip, n_last from an earlier clip, M = 0), tile edges and widths, temperatures,
the all-zero cluster input, the focal loss's masks; label_runs against the oracle and the reference's fixture lists; strided
rows, the accumulating backward, a non-unit upstream gradient, bitwise reproducibility, graph capture; then both losses through
the label-query model.  Needs an MI355X.

Tolerances are the supervised contrastive tests' own (max abs error over the reference's max abs, close_rel): 1e-4 for losses
and row statistics, 1e-3 for gradients."""
import argparse
import os

import numpy as np
import pytest
import torch

from oracle import synth
from tests import temporal_cases as TC, temporal_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from tests.test_engine_gpu import close_rel  # noqa: E402
from tests.test_query_kernels_gpu import strided, outside_untouched  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


@pytest.fixture(scope="module")
def TL():
    from r3d_amd.loss import temporal
    return temporal


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "temporal_cases.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


_ORACLE = {}


def oracle(name):
    """the float64 restatement of a case, computed once: dict(loss, grad[, lse, Q])"""
    if name not in _ORACLE:
        case = TC.BY_NAME[name]
        if case["kind"] == "focal":
            pred, gold = TC.make(case)
            loss, grad = TO.with_grad(lambda p: TO.focal(p, gold, case["pad"], case["exclude"], case["alpha"], case["gamma"],
                                                         case["penalty"])[0], pred)
            _, flags, n_correct, n_word = TO.focal(pred, gold, case["pad"], case["exclude"])
            _ORACLE[name] = dict(loss=loss, grad=grad, flags=flags, counts=[n_correct, n_word])
        elif case["kind"] == "cluster":
            x, iv = TC.make(case)
            loss, grad = TO.with_grad(TO.cluster, x, iv)
            _ORACLE[name] = dict(loss=loss, grad=grad)
        else:
            x, iv = TC.make(case)
            loss, grad = TO.with_grad(TO.contrastive, x, iv, case["temperature"])
            _, lse, Q = TO.contrastive(x, iv, case["temperature"], stats=True)
            _ORACLE[name] = dict(loss=loss, grad=grad, lse=lse, Q=Q)
    return _ORACLE[name]


def _layout(W):
    """(row stride, first column) of the wider buffer a case's rows live in: 16-byte aligned rows where W allows the staging's
    float4 path, an odd stride and offset otherwise."""
    return (W + 8, 4) if W % 8 == 0 else (W + 7, 3)


def _device_runs(TL, case, iv):
    return TL.label_runs(TC.labels_of(iv, case["T"]).to(DEV))


def _run(ops, TL, case, *, add=False, d_loss=None, gscale=1.0, prefill=float("nan")):
    """forward + backward of a cluster / contrast case through the C ABI on rows staged in a wider buffer, the runs found on the
    device from the case's labels; returns loss, ws, dx slice, dx buffer"""
    x, iv = TC.make(case)
    B, T, W = x.shape
    ld, c0 = _layout(W)
    xd, _ = strided(x.reshape(B * T, W), ld, c0)
    dx, dxb = strided(torch.zeros(B * T, W), ld + 1, c0 + 1, fill=prefill)
    if add:
        dx.fill_(prefill)
    r = _device_runs(TL, case, iv)
    loss = torch.full((1,), float("nan"), device=DEV)
    if case["kind"] == "cluster":
        ws = torch.full((ops.tcluster_ws_floats(B, T, W),), float("nan"), device=DEV)
        ops.tcluster_fwd(xd, B, T, r.starts, r.last, r.count, ws, loss)
        ops.tcluster_bwd(xd, B, T, r.starts, r.last, r.count, ws, dx, d_loss=d_loss, gscale=gscale, add=add)
    else:
        ws = torch.full((ops.tcontrast_ws_floats(B, T),), float("nan"), device=DEV)
        ops.tcontrast_fwd(xd, B, T, r.first, r.last, ws, loss, temperature=case["temperature"])
        ops.tcontrast_bwd(xd, B, T, r.first, r.last, ws, dx, temperature=case["temperature"], d_loss=d_loss, gscale=gscale,
                          add=add)
    return loss, ws, dx, dxb


# ---------------------------------------------------------------------------------------------------------------------
# runs
# ---------------------------------------------------------------------------------------------------------------------
def test_label_runs_equal_the_oracle_and_the_fixture_lists(TL, golden):
    for case in TC.CONTRAST + TC.CLUSTER:
        x, iv = TC.make(case)
        B, T = case["B"], case["T"]
        lab = TC.labels_of(iv, T)
        r = TL.label_runs(lab.to(DEV))
        first, last, count = TO.frame_runs(TO.intervals(lab), T)
        assert torch.equal(r.first.cpu().long(), first) and torch.equal(r.last.cpu().long(), last), case["name"]
        assert torch.equal(r.count.cpu().long(), count), case["name"]
        up = TL.runs_from_intervals(iv, T, DEV)
        assert torch.equal(r.buf, up.buf), case["name"]          # (starts past the last run included)
        want = [[] for _ in range(B)]
        for b, s, e in golden[f"iv_{case['name']}"].tolist():
            want[b].append((s, e))
        assert TL.get_cluster_intervals(lab.to(DEV)) == want, case["name"]
    lab32 = TC.labels_of([TC.structure("r", 1142, seed=9)], 1142).to(torch.int32)       # chunks of 5 frames per thread
    assert TL.get_cluster_intervals(lab32.to(DEV)) == TO.intervals(lab32)


# ---------------------------------------------------------------------------------------------------------------------
# contrastive and cluster
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in TC.CONTRAST])
def test_contrastive_kernels_against_float64(ops, TL, name):
    case = TC.BY_NAME[name]
    o = oracle(name)
    B, T, W = case["B"], case["T"], case["W"]
    loss, ws, dx, dxb = _run(ops, TL, case)
    loss2, ws2, dx2, _ = _run(ops, TL, case)                     # the same call again: the same bits
    torch.cuda.synchronize()
    print(f"{name}: loss {float(loss):.7f} oracle {float(o['loss']):.7f}")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dx).all())
    close_rel(loss, o["loss"].reshape(1), f"{name} loss", rtol=1e-4)
    wsc = ws.cpu().view(5, B, T)
    close_rel(wsc[0], o["lse"], f"{name} lse", rtol=1e-4)
    close_rel(wsc[1], o["Q"], f"{name} Q", rtol=1e-4)
    x, _ = TC.make(case)
    close_rel(wsc[2], 1.0 / x.double().norm(dim=2).clamp_min(1e-12), f"{name} 1/|x|", rtol=1e-4)
    close_rel(dx, o["grad"].reshape(B * T, W), f"{name} gradient", rtol=1e-3)
    assert outside_untouched(dxb, _layout(W)[1] + 1, W)
    assert torch.equal(loss, loss2) and torch.equal(dx, dx2) and torch.equal(ws, ws2)


@pytest.mark.parametrize("name", [c["name"] for c in TC.CLUSTER])
def test_cluster_kernels_against_float64(ops, TL, name):
    case = TC.BY_NAME[name]
    o = oracle(name)
    B, T, W = case["B"], case["T"], case["W"]
    loss, ws, dx, dxb = _run(ops, TL, case)
    loss2, _, dx2, _ = _run(ops, TL, case)
    torch.cuda.synchronize()
    print(f"{name}: loss {float(loss):.7f} oracle {float(o['loss']):.7f}")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dx).all())
    close_rel(loss, o["loss"].reshape(1), f"{name} loss", rtol=1e-4)
    close_rel(dx, o["grad"].reshape(B * T, W), f"{name} gradient", rtol=1e-3)
    assert outside_untouched(dxb, _layout(W)[1] + 1, W)
    assert torch.equal(loss, loss2) and torch.equal(dx, dx2)
    x, iv = TC.make(case)
    means = torch.cat([torch.stack([x[b, s:e + 1].double().mean(0) for s, e in clip] +
                                   [torch.zeros(W, dtype=torch.float64)] * (T - len(clip))) for b, clip in enumerate(iv)])
    live = torch.cat([torch.arange(T) < len(clip) for clip in iv])
    close_rel(ws[:B * T * W].view(B * T, W).cpu()[live], means[live], f"{name} run means", rtol=1e-4)
    if case["zero"]:                                             # every pair at distance 0: 1 / 1e-5 each, no gradient
        pairs = len(iv[0]) * (len(iv[0]) - 1) // 2
        assert abs(float(loss) - pairs * 1e5 / (len(iv[0]) - 1)) <= 1e-4 * float(loss) and not bool(dx.any())
    if all(len(clip) == 1 for clip in iv):                       # M = 0: the inter scale is exactly 0
        assert float(ws[-3]) == 0.0


@pytest.mark.parametrize("name", ["n_t200_d48_f", "n_t65_d16_g", "c_t200_c122_f", "c_t65_c48_g"])
def test_backward_add_mode_accumulates_with_a_device_scalar_upstream(ops, TL, name):
    case = TC.BY_NAME[name]
    g64 = oracle(name)["grad"].reshape(-1, case["W"])
    up = torch.tensor([3.0], device=DEV)
    _, _, dx, dxb = _run(ops, TL, case, add=True, d_loss=up, gscale=0.5, prefill=1.0)
    _, _, dw, _ = _run(ops, TL, case, add=False, d_loss=up, gscale=0.5)
    torch.cuda.synchronize()
    close_rel(dw, 1.5 * g64, f"{name} written", rtol=1e-3)
    assert torch.equal(dx, 1.0 + dw)                            # one rounding of the same sum
    assert outside_untouched(dxb, _layout(case["W"])[1] + 1, case["W"], fill_value=1.0)


@pytest.mark.parametrize("name,runs_as", [("n_t200_d48_f", "labels"), ("n_t65_d16_g", "list"), ("n_t65_d48_tau05", "runs"),
                                          ("c_t200_c122_f", "labels"), ("c_t65_c48_g", "list"), ("c_t130_c256_r", "runs")])
def test_public_functions_are_differentiable_and_match_float64(TL, name, runs_as):
    case = TC.BY_NAME[name]
    o = oracle(name)
    x, iv = TC.make(case)
    lab = TC.labels_of(iv, case["T"]).to(DEV)
    runs = {"labels": lab, "list": iv, "runs": TL.label_runs(lab)}[runs_as]
    W = case["W"]
    buf = torch.full((case["B"], case["T"], W + 5), float("nan"), device=DEV)
    buf[:, :, 2:2 + W] = x.to(DEV)
    xd = buf.requires_grad_(True)
    view = xd[:, :, 2:2 + W]                                     # a strided view: row stride W + 5, no copy
    if case["kind"] == "cluster":
        loss = TL.temporal_cluster_loss(view, runs)
    else:
        loss = TL.temporal_contrastive_loss(view, runs, temperature=case["temperature"])
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    assert loss.shape == () and bool(torch.isfinite(loss))
    close_rel(loss.detach().reshape(1), o["loss"].reshape(1), f"{name} loss", rtol=1e-4)
    close_rel(xd.grad[:, :, 2:2 + W], 3.0 * o["grad"], f"{name} gradient", rtol=1e-3)
    assert not bool(xd.grad[:, :, :2].any()) and not bool(xd.grad[:, :, 2 + W:].any())


def test_refused_shapes_raise_and_write_nothing(ops, TL):
    from r3d_amd._lib import R3DHipError
    B, T, W = 2, 8, 257
    x = torch.randn(B * T, W, device=DEV)
    r = TL.label_runs(torch.zeros(B, T, dtype=torch.int64, device=DEV))
    ws, loss, dx = torch.zeros(B * T * W + 64, device=DEV), torch.zeros(1, device=DEV), torch.zeros(B * T, W, device=DEV)
    with pytest.raises(R3DHipError):
        ops.tcluster_fwd(x, B, T, r.starts, r.last, r.count, ws, loss)
    with pytest.raises(R3DHipError):
        ops.tcluster_bwd(x, B, T, r.starts, r.last, r.count, ws, dx)
    with pytest.raises(R3DHipError):
        ops.tcontrast_fwd(x, B, T, r.first, r.last, ws, loss)
    with pytest.raises(R3DHipError):
        ops.tcontrast_bwd(x, B, T, r.first, r.last, ws, dx)
    with pytest.raises(R3DHipError):
        ops.tcontrast_fwd(x[:, :16], B, T, r.first, r.last, ws, loss, temperature=0.0)
    with pytest.raises(R3DHipError):
        ops.focal_rows(x, torch.zeros(B * T, dtype=torch.int64, device=DEV), 5, gamma=0.5, d_pred=dx)
    torch.cuda.synchronize()
    for t in (ws, loss, dx):
        assert not bool(t.any())
    with pytest.raises(ValueError, match="256"):
        TL.temporal_contrastive_loss(x.view(B, T, W), r)
    with pytest.raises(ValueError, match="the runs describe"):
        TL.temporal_cluster_loss(x.view(B, T, W)[:, :4, :16], r)


# ---------------------------------------------------------------------------------------------------------------------
# focal
# ---------------------------------------------------------------------------------------------------------------------
def _focal_kw(case):
    return dict(exclude_idx=case["exclude"], alpha=case["alpha"], gamma=case["gamma"], penalty_weight=case["penalty"])


def _run_focal(ops, case, *, add=False, d_loss=None, gscale=1.0, prefill=float("nan")):
    pred, gold = TC.make(case)
    N, C = pred.shape
    ld, c0 = _layout(C)
    pd, _ = strided(pred, ld, c0)
    dp, dpb = strided(torch.zeros(N, C), ld + 1, c0 + 1, fill=prefill)
    if add:
        dp.fill_(prefill)
    ws, loss = torch.full((N,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
    flags, counts = torch.zeros(N, dtype=torch.bool, device=DEV), torch.full((2,), -1, dtype=torch.int64, device=DEV)
    ops.focal_rows(pd, gold.to(DEV), case["pad"], ws=ws, loss_out=loss, flags=flags, counts=counts, d_pred=dp, d_loss=d_loss,
                   gscale=gscale, add=add, **_focal_kw(case))
    return loss, flags, counts, dp, dpb


@pytest.mark.parametrize("name", [c["name"] for c in TC.FOCAL])
def test_focal_kernel_against_float64(ops, TL, golden, name):
    case = TC.BY_NAME[name]
    o = oracle(name)
    pred, gold = TC.make(case)
    loss, flags, counts, dp, dpb = _run_focal(ops, case)
    loss2, flags2, counts2, dp2, _ = _run_focal(ops, case)
    torch.cuda.synchronize()
    print(f"{name}: loss {float(loss):.7f} oracle {float(o['loss']):.7f} counts {counts.tolist()}")
    close_rel(loss, o["loss"].reshape(1), f"{name} loss", rtol=1e-4)
    close_rel(dp, o["grad"], f"{name} gradient", rtol=1e-3)
    assert outside_untouched(dpb, _layout(case["C"])[1] + 1, case["C"])
    assert np.array_equal(flags.cpu().numpy(), golden[f"flags_{name}"]) and torch.equal(flags.cpu(), o["flags"])
    assert counts.tolist() == golden[f"counts_{name}"].tolist() == o["counts"]
    assert torch.equal(loss, loss2) and torch.equal(dp, dp2) and torch.equal(flags, flags2) and torch.equal(counts, counts2)
    if case["oob"] is not None:                                  # the out-of-range label: a masked row
        row = int(((gold < 0) | (gold >= case["C"])).nonzero()[0])
        assert not bool(dp[row].any()) and not bool(flags[row])
    if case["argmax_pad"]:
        assert bool(((pred.argmax(1) == case["pad"]) & (gold != case["pad"])).any())
    # the public functions: autograd with a non-unit upstream gradient, and the counters of cal_performance_focal
    pd = pred.to(DEV).requires_grad_(True)
    l, fl = TL.focal_loss(pd, gold.to(DEV), case["pad"], case["exclude"], case["alpha"], case["gamma"], case["penalty"])
    (3.0 * l).backward()
    torch.cuda.synchronize()
    assert l.shape == () and fl.dtype == torch.bool and torch.equal(fl, flags) and torch.equal(l.detach().reshape(1), loss)
    close_rel(pd.grad, 3.0 * o["grad"], f"{name} autograd gradient", rtol=1e-3)
    if (case["alpha"], case["gamma"], case["penalty"]) == (1.0, 2.0, 0.0):
        l4, n_correct, n_word, fl4 = TL.cal_performance_focal(pred.to(DEV), gold.to(DEV), case["pad"], case["exclude"])
        assert [n_correct, n_word] == o["counts"] and torch.equal(fl4, flags) and torch.equal(l4.reshape(1), loss)
        assert isinstance(n_correct, int) and isinstance(n_word, int)


def test_focal_add_mode_accumulates(ops):
    case = TC.BY_NAME["f_n65_c122"]
    up = torch.tensor([3.0], device=DEV)
    _, _, _, dp, dpb = _run_focal(ops, case, add=True, d_loss=up, gscale=0.5, prefill=1.0)
    _, _, _, dw, _ = _run_focal(ops, case, add=False, d_loss=up, gscale=0.5)
    torch.cuda.synchronize()
    close_rel(dw, 1.5 * oracle(case["name"])["grad"], "written", rtol=1e-3)
    assert torch.equal(dp, 1.0 + dw)
    assert outside_untouched(dpb, _layout(case["C"])[1] + 1, case["C"], fill_value=1.0)


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n_t200_d48_f", "c_t200_c122_f", "f_n65_c122"])
def test_forward_and_backward_replay_from_a_graph_with_the_same_bits(TL, name):
    case = TC.BY_NAME[name]
    if case["kind"] == "focal":
        pred, gold = TC.make(case)
        x, gd = pred.to(DEV).requires_grad_(True), gold.to(DEV)
        fn = lambda: TL.focal_loss(x, gd, case["pad"], case["exclude"], case["alpha"], case["gamma"], case["penalty"])[0]  # noqa: E731
    else:
        xc, iv = TC.make(case)
        x, lab = xc.to(DEV).requires_grad_(True), TC.labels_of(iv, case["T"]).to(DEV)
        if case["kind"] == "cluster":
            fn = lambda: TL.temporal_cluster_loss(x, lab)                                    # noqa: E731  (run detection inside)
        else:
            fn = lambda: TL.temporal_contrastive_loss(x, lab, temperature=case["temperature"])   # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loss = fn()
        (grad,) = torch.autograd.grad(loss, x)
        loss, grad = loss.clone(), grad.clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_loss = fn()
        (g_grad,) = torch.autograd.grad(g_loss, x)
    for _ in range(2):
        g_loss.detach().fill_(float("nan"))                      # (the graph's static outputs, outside autograd)
        g_grad.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_loss, loss) and torch.equal(g_grad, grad)


# ---------------------------------------------------------------------------------------------------------------------
# through the label-query model
# ---------------------------------------------------------------------------------------------------------------------
def test_cluster_and_focal_losses_train_the_label_query_model(TL):
    from r3d_amd.model.futr_proposed import FUTR
    B, S, H, K, heads, query_num = 2, 12, 32, 17, 4, 48
    pad = K + 1
    args = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    model = FUTR(K, H, pad, torch.device(DEV), args, n_query=8, n_head=heads, num_encoder_layers=2, num_decoder_layers=1,
                 query_num=query_num)
    names = [(n, tuple(q.shape)) for n, q in model.named_parameters()]
    with torch.no_grad():
        for j, (n, s) in enumerate(names):
            if not n.startswith("transformer.encoder."):
                dict(model.named_parameters())[n].copy_(torch.from_numpy(synth.fill_value(n, s, j)))
    model = model.to(DEV).eval()
    feats, _, lab, _, _ = [torch.from_numpy(t) for t in synth.make_batch(B, S, K, pad, 5, depth_hw=(2, 2))]
    query = torch.from_numpy(synth.randint(B * S, query_num, 991).reshape(B, S))
    query[:, 4:7] = query[:, 4:5]                                # a run of three frames per clip
    gold = lab.reshape(-1).long()
    inputs = (feats.to(DEV), lab.to(DEV))

    def grads():
        out = {n: dict(model.named_parameters())[n].grad.clone() for n in ("fc_seg.weight", "input_embed.weight")}
        model.zero_grad(set_to_none=True)
        return out

    seg = model(inputs, query.to(DEV))["seg"]
    assert tuple(seg.shape) == (B, S, K - 1)
    loss = TL.temporal_cluster_loss(seg, query.to(DEV)) + TL.focal_loss(seg.view(-1, K - 1), gold.to(DEV), pad)[0]
    loss.backward()
    torch.cuda.synchronize()
    got = grads()
    seg64 = seg.detach().cpu().double().requires_grad_(True)
    l64 = TO.cluster(seg64, TO.intervals(query)) + TO.focal(seg64.view(-1, K - 1), gold, pad)[0]
    l64.backward()
    assert abs(float(loss.detach()) - float(l64.detach())) <= 1e-4 * abs(float(l64.detach()))
    seg2 = model(inputs, query.to(DEV))["seg"]
    seg2.backward(seg64.grad.float().to(DEV))
    torch.cuda.synchronize()
    want = grads()
    for n in got:
        assert bool(want[n].any())
        close_rel(got[n], want[n], n, rtol=1e-3)
