"""The supervised contrastive loss kernels (csrc/supcon.hip) against the float64 restatement (tests/supcon_oracle.py) over
tests/supcon_cases.py: tile edges and widths, label structures, temperatures, views and modes, ignored rows, in-kernel
normalisation, the input on which the reference is nan; bitwise reproducibility, the accumulating backward, refusal, the
memory bound; then the RNN engine's step and loop with --supcon_weight.  Needs an MI355X.

Tolerances are the tiled attention tests' own (max abs error over the reference's max abs, close_rel): 1e-4 for the loss
and lse, 1e-3 for gradients."""
import argparse
import contextlib
import io
import re

import pytest
import torch

from oracle import synth
from tests import rnn_oracle as RO, supcon_cases as SC, supcon_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from tests.test_engine_gpu import close_rel  # noqa: E402
from tests.test_query_kernels_gpu import strided, outside_untouched  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


def _kernel_kwargs(case):
    kw = SC.oracle_kwargs(case)
    kw.pop("A")
    return kw


def _layout(D):
    """(row stride, first column) of the wider buffer a case's rows live in: 16-byte aligned rows where D allows the
    staging's float4 path, an odd stride and offset otherwise."""
    return (D + 8, 4) if D % 8 == 0 else (D + 7, 3)


def _run(ops, case, z, y, *, add=False, d_loss=None, gscale=1.0, prefill=float("nan")):
    """forward + backward through the C ABI on rows staged in a wider buffer; returns loss, ws, dx slice, dx buffer"""
    N, D = z.shape
    A = SC.oracle_kwargs(case)["A"]
    ld, c0 = _layout(D)
    zd, _ = strided(z, ld, c0)
    dx, dxb = strided(torch.zeros(N, D), ld + 1, c0 + 1, fill=prefill)
    if add:
        dx.fill_(prefill)
    ws = torch.full((ops.supcon_ws_floats(N),), float("nan"), device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    yd = None if y is None else y.to(DEV)
    kw = _kernel_kwargs(case)
    ops.supcon_fwd(zd, yd, case["bsz"], A, ws, loss, **kw)
    ops.supcon_bwd(zd, yd, case["bsz"], A, ws, dx, d_loss=d_loss, gscale=gscale, add=add, **kw)
    return loss, ws, dx, dxb


@pytest.mark.parametrize("name", [c["name"] for c in SC.CASES])
def test_kernels_against_float64(ops, name):
    case = SC.BY_NAME[name]
    x, y = SC.make(case)
    z = SO.contrast_rows(x)
    N, D = z.shape
    yo = SC.oracle_labels(case, y)
    kw = SC.oracle_kwargs(case)
    A = kw["A"]
    l64, g64, lse64, P64 = SO.supcon_with_grad(z, yo, **kw)
    loss, ws, dx, dxb = _run(ops, case, z, y)
    loss2, ws2, dx2, _ = _run(ops, case, z, y)                   # the same call again: the same bits
    torch.cuda.synchronize()
    close_rel(loss, l64.reshape(1), f"{name} loss", rtol=1e-4)
    kept = torch.ones(A, dtype=torch.bool) if not case["ignore"] else (yo[:A] != SC.IGNORE)
    rows = kept & torch.isfinite(lse64)
    wsc = ws.cpu()
    if bool(rows.any()):
        close_rel(wsc[:A][rows], lse64[rows], f"{name} lse", rtol=1e-4)
    assert torch.equal(wsc[2 * N:2 * N + A][kept], P64[kept].float()), f"{name} P"
    assert not bool(wsc[2 * N:2 * N + A][~kept].any())
    assert float(wsc[4 * N]) == max(1, int(kept.sum()))
    close_rel(dx, g64, f"{name} gradient", rtol=1e-3)
    ld, c0 = _layout(D)
    assert outside_untouched(dxb, c0 + 1, D)
    assert torch.equal(loss, loss2) and torch.equal(dx, dx2)
    assert torch.equal(ws.view(torch.int32), ws2.view(torch.int32))       # (bits: rows past A keep the NaN fill)
    if case["labels"] == "distinct" or case["ignore"] == "all" or N == 1:
        assert float(loss) == 0.0 and not bool(dx.any())         # no positive pair / no anchor / no contrast: exactly 0
    if case["ignore"]:
        assert not bool(dx.cpu()[yo == SC.IGNORE].any())


@pytest.mark.parametrize("name", ["k17", "v2_one", "normalize_raw_d20_ign"])
def test_backward_add_mode_accumulates_with_a_device_scalar_upstream(ops, name):
    case = SC.BY_NAME[name]
    x, y = SC.make(case)
    z = SO.contrast_rows(x)
    _, g64, _, _ = SO.supcon_with_grad(z, SC.oracle_labels(case, y), **SC.oracle_kwargs(case))
    up = torch.tensor([2.0], device=DEV)
    _, _, dx, dxb = _run(ops, case, z, y, add=True, d_loss=up, gscale=0.25, prefill=1.0)
    _, _, dw, _ = _run(ops, case, z, y, add=False, d_loss=up, gscale=0.25)
    torch.cuda.synchronize()
    close_rel(dw, 0.5 * g64, f"{name} written", rtol=1e-3)
    assert torch.equal(dx, 1.0 + dw)                            # one rounding of the same sum
    assert outside_untouched(dxb, _layout(z.shape[1])[1] + 1, z.shape[1], fill_value=1.0)


@pytest.mark.parametrize("name", ["v2_all", "v2_one", "simclr", "ign_tile1_row3", "normalize_raw", "raw_03_randn", "t05_tb007"])
def test_module_is_differentiable_and_matches_float64(name):
    from r3d_amd.loss import SupConLoss
    case = SC.BY_NAME[name]
    x, y = SC.make(case)
    l64, g64, _, _ = SO.supcon_with_grad(SO.contrast_rows(x), SC.oracle_labels(case, y), **SC.oracle_kwargs(case))
    crit = SupConLoss(**SC.module_kwargs(case), ignore_index=SC.IGNORE if case["ignore"] else None, normalize=case["normalize"])
    xd = x.to(DEV).requires_grad_(True)
    loss = crit(xd, None if y is None else y.to(DEV))
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    assert loss.shape == () and bool(torch.isfinite(loss))
    close_rel(loss.detach().reshape(1), l64.reshape(1), f"{name} loss", rtol=1e-4)
    close_rel(xd.grad, 3.0 * torch.stack(g64.split(case["bsz"]), 1), f"{name} gradient", rtol=1e-3)


def test_module_flattens_trailing_dimensions():
    from r3d_amd.loss import SupConLoss
    case = SC.BY_NAME["v2_all"]
    x, y = SC.make(case)
    a = SupConLoss()(x.to(DEV), y.to(DEV))
    b = SupConLoss()(x.view(case["bsz"], 2, 4, 5).to(DEV), y.to(DEV))
    assert torch.equal(a, b)


def test_refused_width_raises_and_writes_nothing(ops):
    from r3d_amd._lib import R3DHipError
    N, D = 8, 257
    z = torch.randn(N, D, device=DEV)
    y = torch.arange(N, device=DEV) % 2
    ws, loss, dx = torch.zeros(ops.supcon_ws_floats(N), device=DEV), torch.zeros(1, device=DEV), torch.zeros(N, D, device=DEV)
    assert not ops.supcon_supported(D)
    with pytest.raises(R3DHipError):
        ops.supcon_fwd(z, y, N, N, ws, loss)
    with pytest.raises(R3DHipError):
        ops.supcon_bwd(z, y, N, N, ws, dx)
    with pytest.raises(R3DHipError):                            # more anchors than rows
        ops.supcon_fwd(z[:, :16], y, N, N + 1, ws, loss)
    torch.cuda.synchronize()
    for t in (ws, loss, dx):
        assert not bool(t.any())


def test_no_score_matrix_is_allocated():
    """N = 4096, D = 128: forward + backward grow the allocator's peak by less than one eighth of the 4 N^2 bytes of one
    score matrix (8.4 MB); the gradient, autograd's copy of it and the workspace are about 4.3 MB."""
    from r3d_amd.loss import SupConLoss
    N, D = 4096, 128
    g = torch.Generator().manual_seed(11)
    x = torch.nn.functional.normalize(torch.randn(N, 1, D, generator=g), dim=2).to(DEV).requires_grad_(True)
    y = torch.randint(0, 122, (N,), generator=g).to(DEV)
    crit = SupConLoss()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = crit(x, y)
    loss.backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"peak growth {grown} bytes, bound {4 * N * N // 8}")
    assert grown < 4 * N * N // 8, grown
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())


# ---------------------------------------------------------------------------------------------------------------------
# the RNN engine's step with --supcon_weight
# ---------------------------------------------------------------------------------------------------------------------
W = 0.5


def _args(H, **kw):
    a = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript",
                           hidden_dim=H, n_query=8, n_head=8, epochs=1, task="long", erank_weight=0.0, temperature=0.07)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rnn(B, S, H, K, ragged, seed=3):
    """(model on the GPU with the analytic parameter fill, its parameters, the 5-tuple)"""
    from r3d_amd.model.rnn import FUTR
    pad = K + 1
    model = FUTR(K, H, pad, torch.device(DEV), _args(H), n_query=8, n_head=8, num_encoder_layers=2, num_decoder_layers=1)
    state = synth.fill_state([(n, tuple(p.shape)) for n, p in model.named_parameters()])
    params = {n: torch.from_numpy(v) for n, v in state.items()}
    with torch.no_grad():
        for n, q in model.named_parameters():
            q.copy_(params[n])
    b = synth.make_batch(B, S, K, pad, seed, depth_hw=(2, 2))
    if ragged:
        for r in range(B):
            b[2][r, S - (5 * r) % 11:] = pad                     # tails of 0 .. 10 padded frames
    return model.to(DEV), params, [torch.from_numpy(x) for x in b]


def _dev(batch):
    f, _d, lab, dur, tgt = batch
    return f.to(DEV).contiguous(), lab.to(DEV).contiguous(), dur.to(DEV).contiguous(), tgt.to(DEV).contiguous()


_ORACLE = {}


def _oracle_step(key, params, batch, pad, weight=W):
    """float64 autograd of the three losses + weight * the contrastive term: (losses dict, supcon loss, gradients)"""
    if (key, weight) not in _ORACLE:
        feats, _d, lab, dur, tgt = batch
        p = {n: t.double().requires_grad_(RO.is_live(n)) for n, t in params.items()}
        out = RO.forward(p, feats.double())
        res = RO.losses(out, lab, dur.double(), tgt, pad)
        H = out["supcon"].shape[-1]
        sc, _, _ = SO.supcon(out["supcon"].reshape(-1, H), lab.reshape(-1), temperature=0.07, base_temperature=0.07,
                             ignore_index=pad, normalize=True)
        (res["loss"] + weight * sc).backward()
        _ORACLE[(key, weight)] = ({k: float(res[k]) for k in ("loss_seg", "loss_action", "loss_dur", "loss")}, float(sc),
                                  {n: q.grad for n, q in p.items() if q.grad is not None})
    return _ORACLE[(key, weight)]


SHAPES = [(8, 16, 128, 122, False), (13, 37, 136, 17, True)]


@pytest.mark.parametrize("B,S,H,K,ragged", SHAPES)
def test_rnn_step_with_supcon_matches_float64(B, S, H, K, ragged):
    model, params, batch = _rnn(B, S, H, K, ragged)
    pad = K + 1
    res, sc, grads = _oracle_step((B, S, H, K), params, batch, pad)
    eng = model.engine()
    eng.supcon_weight, eng.supcon_temperature = W, 0.07
    feats, lab, dur, tgt = _dev(batch)
    eng.forward(feats, None, lab, "train", training=True)
    loss, _ = eng.losses(lab, tgt, dur, tick=True)
    eng.backward()
    torch.cuda.synchronize()
    w = eng.last["w"]
    got = loss.cpu().double()
    want = [res["loss_seg"], res["loss_action"], res["loss_dur"], res["loss"] + W * sc]
    print(f"losses {got.tolist()} oracle {want}; supcon {float(w.sc_loss)} oracle {sc}")
    for g, r in zip(got.tolist(), want):
        assert abs(g - r) <= 1e-3 * max(abs(r), 1e-5), (got.tolist(), want)
    assert abs(float(w.sc_loss) - sc) <= 1e-3 * abs(sc)
    assert sorted(grads) == sorted(eng.arena.live_names)
    worst = {n: float((eng.arena.g(n).cpu().double() - r).abs().max() / max(float(r.abs().max()), 1e-5)) for n, r in grads.items()}
    print("gradient rel errors:", {n: f"{e:.2e}" for n, e in worst.items()})
    for n, r in grads.items():
        close_rel(eng.arena.g(n), r, n, rtol=1e-3)


def test_supcon_term_changes_the_gradient_it_should():
    """the contrastive term reaches rnn_fc and everything below it, and leaves the heads' own gradients alone"""
    B, S, H, K, _ = SHAPES[0]
    out = []
    for weight in (0.0, W):
        model, _, batch = _rnn(B, S, H, K, False)
        eng = model.engine()
        eng.supcon_weight = weight
        feats, lab, dur, tgt = _dev(batch)
        eng.forward(feats, None, lab, "train", training=True)
        eng.losses(lab, tgt, dur, tick=True)
        eng.backward()
        torch.cuda.synchronize()
        out.append({n: eng.arena.g(n).clone() for n in eng.arena.live_names})
    for n in out[0]:
        same = torch.equal(out[0][n], out[1][n])
        assert same == n.startswith(("fc.", "fc_len.", "fc_seg.")), n


def test_graphed_and_eager_steps_end_in_identical_parameters():
    from r3d_amd.train_unimodal import _UnimodalSteps
    B, S, H, K, _ = SHAPES[0]
    hyper = (5e-3, (0.9, 0.999), 1e-8)
    runs = []
    for graphed in (False, True):
        model, _, batch = _rnn(B, S, H, K, False)
        eng = model.engine()
        eng.supcon_weight = W
        feats, lab, dur, tgt = _dev(batch)
        acc_l = torch.zeros(4, dtype=torch.float64, device=DEV)
        acc_c = torch.zeros(4, dtype=torch.int64, device=DEV)
        acc_s = torch.zeros(1, dtype=torch.float64, device=DEV)
        gs = _UnimodalSteps(eng, acc_l, acc_c, acc_s)
        for _ in range(3):
            if graphed:
                gs.step([feats, lab, dur, tgt], 1e-3, hyper, True)
            else:
                gs._enqueue([feats, lab, dur, tgt], 1e-3, hyper, True)
        torch.cuda.synchronize()
        if graphed:
            assert next(iter(gs.shapes.values()))["graph"] is not None       # steps 2 and 3 ran as a captured graph
        assert float(acc_s) > 0.0
        runs.append((eng.arena.params.clone(), eng.arena.exp_avg.clone(), acc_l.clone(), acc_c.clone(), acc_s.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_zero_weight_leaves_every_buffer_as_without_the_flag():
    B, S, H, K, _ = SHAPES[0]
    runs = []
    for explicit in (False, True):
        model, _, batch = _rnn(B, S, H, K, False)
        eng = model.engine()
        if explicit:
            eng.supcon_weight, eng.supcon_temperature = 0.0, 0.5
        feats, lab, dur, tgt = _dev(batch)
        eng._shape(B, S, True).sc_ws.fill_(float("nan"))
        loss, counts = eng.train_step(feats, None, lab, dur, tgt, 1e-3, 5e-3)
        torch.cuda.synchronize()
        w = eng.last["w"]
        assert bool(torch.isnan(w.sc_ws).all()) and float(w.sc_loss) == 0.0     # nothing of the term was launched
        runs.append((loss.clone(), counts.clone(), eng.arena.params.clone(), eng.arena.grads.clone(), eng.arena.exp_avg.clone(),
                     w.d_tgt.clone(), w.tgt.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


_NUM = re.compile(r"-?\d+\.\d+")


def test_train_two_epochs_prints_the_supcon_line(tmp_path):
    from r3d_amd import train_unimodal as TU
    from r3d_amd.optim import FlatAdamW
    B, S, H, K = 8, 12, 16, 17
    pad = K + 1
    model, _, _ = _rnn(B, S, H, K, False)
    batches = [[torch.from_numpy(x) for x in synth.make_batch(B, S, K, pad, 20 + i, depth_hw=(2, 2))] for i in range(3)]
    val = [[torch.from_numpy(x) for x in synth.make_batch(1, 9, K, pad, 40, pad_tail=False, depth_hw=(2, 2))]]
    opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)

    class NoSched:
        def step(self):
            pass
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TU.train(_args(H, epochs=2, supcon_weight=W), model, batches, opt, NoSched(), torch.nn.MSELoss(reduction="none"),
                 str(tmp_path), pad, torch.device(DEV), val, 1)
    lines = buf.getvalue().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("supcon loss :")]
    assert len(at) == 2 and all(lines[i - 1].startswith("seg loss :") for i in at), lines
    for i in at:                                                 # Loss = seg + CE + dur + w * supcon, each printed rounded
        total = float(_NUM.findall(lines[i - 4])[-1])
        ce, dur = float(_NUM.findall(lines[i - 3])[-1]), float(_NUM.findall(lines[i - 2])[-1])
        seg, sc = float(_NUM.findall(lines[i - 1])[0]), float(_NUM.findall(lines[i])[0])
        assert sc > 0.0 and abs(total - (seg + ce + dur + W * sc)) <= 3e-3, lines[i - 4:i + 1]
