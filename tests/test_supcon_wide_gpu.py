"""The supervised contrastive loss's wide route (csrc/supcon.hip, 257 <= D <= 2048; ops wide=True, SupConLoss(wide=True),
--wide_supcon) against the float64 restatement (tests/supcon_oracle.py) over tests/supcon_wide_cases.py: row-tile edges
crossed with chunk edges, in-kernel normalisation across chunks, views and modes, ignored rows, the inputs on which the
reference is nan, one clustered case; bitwise reproducibility, the accumulating backward, equality with the narrow launches
up to 256 columns, refusal, the memory bound; then the RNN and CNN engines' steps and the loop with --wide_supcon.  Needs an
MI355X.

Tolerances are tests/test_supcon_gpu.py's own (close_rel: max abs error over the reference's max abs): 1e-4 for the loss and
lse, 1e-3 for gradients; P and the anchor count exactly.  tests/test_supcon_wide_cpu.py shows float32 arithmetic alone within
one eighth of each on every case."""
import contextlib
import io

import pytest
import torch

from oracle import synth
from tests import cnn_oracle as CO, supcon_cases as SC, supcon_oracle as SO, supcon_wide_cases as WC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from tests.test_engine_gpu import close_rel  # noqa: E402
from tests.test_query_kernels_gpu import strided, outside_untouched  # noqa: E402
from tests.test_supcon_gpu import W, _NUM, _args, _dev, _layout, _oracle_step  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


def _kernel_kwargs(case):
    kw = WC.oracle_kwargs(case)
    kw.pop("A")
    return kw


def _run(ops, case, z, y, *, wide=True, add=False, d_loss=None, gscale=1.0, prefill=float("nan")):
    """forward + backward through the C ABI on rows staged in a wider buffer (tests.test_supcon_gpu._layout: 16-byte aligned
    rows where D allows the staging's float4 path, an odd stride and offset otherwise); loss, ws, dx slice, dx buffer"""
    N, D = z.shape
    A = WC.oracle_kwargs(case)["A"]
    ld, c0 = _layout(D)
    zd, _ = strided(z, ld, c0)
    dx, dxb = strided(torch.zeros(N, D), ld + 1, c0 + 1, fill=prefill)
    if add:
        dx.fill_(prefill)
    kw = _kernel_kwargs(case)
    ws = torch.full((ops.supcon_ws_floats(N, D, kw["normalize"], wide=wide),), float("nan"), device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    yd = None if y is None else y.to(DEV)
    ops.supcon_fwd(zd, yd, case["bsz"], A, ws, loss, wide=wide, **kw)
    ops.supcon_bwd(zd, yd, case["bsz"], A, ws, dx, d_loss=d_loss, gscale=gscale, add=add, wide=wide, **kw)
    return loss, ws, dx, dxb


_REF = {}


def _reference(name):
    """(z, y, oracle labels, float64 loss, gradient, lse, P) of a case, computed once"""
    if name not in _REF:
        case = WC.BY_NAME[name]
        x, y = WC.make(case)
        z = SO.contrast_rows(x)
        yo = WC.oracle_labels(case, y)
        _REF[name] = (x, z, y, yo) + tuple(SO.supcon_with_grad(z, yo, **WC.oracle_kwargs(case)))
    return _REF[name]


@pytest.mark.parametrize("name", [c["name"] for c in WC.CASES])
def test_wide_kernels_against_float64(ops, name):
    case = WC.BY_NAME[name]
    _, z, y, yo, l64, g64, lse64, P64 = _reference(name)
    N, D = z.shape
    A = WC.oracle_kwargs(case)["A"]
    loss, ws, dx, dxb = _run(ops, case, z, y)
    loss2, ws2, dx2, _ = _run(ops, case, z, y)                   # the same call again: the same bits
    torch.cuda.synchronize()
    kept = torch.ones(A, dtype=torch.bool) if not case["ignore"] else (yo[:A] != WC.IGNORE)
    rows = kept & torch.isfinite(lse64)
    wsc = ws.cpu()
    rel = lambda a, b: float((a.double().cpu() - b).abs().max()) / max(float(b.abs().max()), 1e-5)      # noqa: E731
    print(f"{name}: loss rel {rel(loss, l64.reshape(1)):.2e}, gradient rel {rel(dx, g64):.2e}, lse rel "
          f"{rel(wsc[:A][rows], lse64[rows]) if bool(rows.any()) else 0.0:.2e}")
    close_rel(loss, l64.reshape(1), f"{name} loss", rtol=1e-4)
    if bool(rows.any()):
        close_rel(wsc[:A][rows], lse64[rows], f"{name} lse", rtol=1e-4)
    assert torch.equal(wsc[2 * N:2 * N + A][kept], P64[kept].float()), f"{name} P"
    assert not bool(wsc[2 * N:2 * N + A][~kept].any())
    assert float(wsc[4 * N]) == max(1, int(kept.sum()))
    close_rel(dx, g64, f"{name} gradient", rtol=1e-3)
    assert outside_untouched(dxb, _layout(D)[1] + 1, D)
    assert torch.equal(loss, loss2) and torch.equal(dx, dx2)
    assert torch.equal(ws.view(torch.int32), ws2.view(torch.int32))       # (bits: rows past A keep the NaN fill)
    if case["labels"] == "distinct" or case["ignore"] == "all" or N == 1:
        assert float(loss) == 0.0 and not bool(dx.any())         # no positive pair / no anchor / no contrast: exactly 0
    if case["ignore"]:
        assert not bool(dx.cpu()[yo == WC.IGNORE].any())


@pytest.mark.parametrize("name", WC.ADD_CASES)
def test_wide_backward_add_mode_accumulates_with_a_device_scalar_upstream(ops, name):
    case = WC.BY_NAME[name]
    _, z, y, _, _, g64, _, _ = _reference(name)
    up = torch.tensor([2.0], device=DEV)
    _, _, dx, dxb = _run(ops, case, z, y, add=True, d_loss=up, gscale=0.25, prefill=1.0)
    _, _, dw, _ = _run(ops, case, z, y, add=False, d_loss=up, gscale=0.25)
    torch.cuda.synchronize()
    close_rel(dw, 0.5 * g64, f"{name} written", rtol=1e-3)
    assert torch.equal(dx, 1.0 + dw)                            # prefill + written: one rounding of the same sum
    assert outside_untouched(dxb, _layout(z.shape[1])[1] + 1, z.shape[1], fill_value=1.0)


@pytest.mark.parametrize("name", ["n200_d16", "n200_d136", "n130_d256", "normalize_raw"])
def test_wide_entries_make_the_narrow_launches_up_to_256_columns(ops, name):
    case = SC.BY_NAME[name]
    x, y = SC.make(case)
    z = SO.contrast_rows(x)
    N = z.shape[0]
    up = torch.tensor([0.75], device=DEV)
    a = _run(ops, case, z, y, wide=False, d_loss=up)
    b = _run(ops, case, z, y, wide=True, d_loss=up)
    torch.cuda.synchronize()
    assert a[1].numel() == b[1].numel() == 4 * N + 4
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert bool(torch.isfinite(a[0]).all()) and bool(a[2].any())


@pytest.mark.parametrize("name", WC.MODULE_CASES)
def test_wide_module_is_differentiable_and_matches_float64(name):
    from r3d_amd.loss import SupConLoss
    case = WC.BY_NAME[name]
    x, _, y, _, l64, g64, _, _ = _reference(name)
    crit = SupConLoss(**WC.module_kwargs(case), ignore_index=WC.IGNORE if case["ignore"] else None, normalize=case["normalize"],
                      wide=True)
    xd = x.to(DEV).requires_grad_(True)
    loss = crit(xd, None if y is None else y.to(DEV))
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    assert loss.shape == () and bool(torch.isfinite(loss))
    close_rel(loss.detach().reshape(1), l64.reshape(1), f"{name} loss", rtol=1e-4)
    close_rel(xd.grad, 3.0 * torch.stack(g64.split(case["bsz"]), 1), f"{name} gradient", rtol=1e-3)


def test_wide_module_flattens_trailing_dimensions_to_300_columns():
    from r3d_amd.loss import SupConLoss
    case = WC.BY_NAME["w_t05_d300"]
    x, y = WC.make(case)
    kw = WC.module_kwargs(case)
    a = SupConLoss(**kw, wide=True)(x.to(DEV), y.to(DEV))
    b = SupConLoss(**kw, wide=True)(x.view(case["bsz"], 1, 3, 100).to(DEV), y.to(DEV))
    assert torch.equal(a, b) and bool(torch.isfinite(a))
    with pytest.raises(ValueError, match="256"):                # without the keyword the same input is refused as before
        SupConLoss(**kw)(x.view(case["bsz"], 1, 3, 100).to(DEV), y.to(DEV))


def test_wide_refusals_raise_and_write_nothing(ops):
    from r3d_amd._lib import R3DHipError
    N, D = 8, 2049
    z = torch.randn(N, D, device=DEV)
    y = torch.arange(N, device=DEV) % 2
    ws, loss, dx = torch.zeros(4 * N + 4 + N * D, device=DEV), torch.zeros(1, device=DEV), torch.zeros(N, D, device=DEV)
    assert not ops.supcon_supported(D, wide=True)
    with pytest.raises(R3DHipError):
        ops.supcon_fwd(z, y, N, N, ws, loss, wide=True)
    with pytest.raises(R3DHipError):
        ops.supcon_bwd(z, y, N, N, ws, dx, wide=True)
    with pytest.raises(R3DHipError):                            # more anchors than rows
        ops.supcon_fwd(z[:, :512], y, N, N + 1, ws, loss, normalize=True, wide=True)
    with pytest.raises(R3DHipError):
        ops.supcon_bwd(z[:, :512], y, N, N + 1, ws, dx[:, :512], normalize=True, wide=True)
    with pytest.raises(ValueError, match="ws has"):             # the wide workspace is checked on the host
        ops.supcon_bwd(z[:, :512], y, N, N, ws[:4 * N + 4], dx[:, :512], normalize=True, wide=True)
    torch.cuda.synchronize()
    for t in (ws, loss, dx):
        assert not bool(t.any())


@pytest.mark.parametrize("normalize", [False, True])
def test_wide_route_allocates_no_score_matrix(normalize):
    """N = 4096, D = 512: forward + backward grow the allocator's peak by less than one eighth of the 4 N^2 bytes of one score
    matrix (8.4 MB) plus, without normalize, twice the gradient's size (8.4 MB each: the gradient and autograd's copy of it; the
    workspace is 4 N + 4 floats); with normalize three times (the wide workspace adds dz [N, D] to the 4 N + 4 floats, which the eighth
    covers)."""
    from r3d_amd.loss import SupConLoss
    N, D = 4096, 512
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, 1, D, generator=g)
    x = (x if normalize else torch.nn.functional.normalize(x, dim=2)).to(DEV).requires_grad_(True)
    y = torch.randint(0, 122, (N,), generator=g).to(DEV)
    crit = SupConLoss(normalize=normalize, wide=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = crit(x, y)
    loss.backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    grad_bytes = 4 * N * D
    bound = 4 * N * N // 8 + (3 if normalize else 2) * grad_bytes       # 33 554 432 with normalize, 25 165 824 without
    print(f"normalize {normalize}: peak growth {grown} bytes, bound {bound}")
    assert grown < bound, (grown, bound)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())


# ---------------------------------------------------------------------------------------------------------------------
# the RNN engine's step with --wide_rnn --wide_supcon --supcon_weight
# ---------------------------------------------------------------------------------------------------------------------
def _rnn(B, S, H, K, ragged, seed=3):
    """tests.test_supcon_gpu._rnn with --wide_rnn: (model on the GPU with the analytic parameter fill, its parameters, the
    5-tuple); ragged: clip r ends in (2 r + 1) mod 4 padded frames"""
    from r3d_amd.model.rnn import FUTR
    pad = K + 1
    model = FUTR(K, H, pad, torch.device(DEV), _args(H, wide_rnn=True), n_query=8, n_head=8, num_encoder_layers=2,
                 num_decoder_layers=1)
    state = synth.fill_state([(n, tuple(p.shape)) for n, p in model.named_parameters()])
    params = {n: torch.from_numpy(v) for n, v in state.items()}
    with torch.no_grad():
        for n, q in model.named_parameters():
            q.copy_(params[n])
    b = synth.make_batch(B, S, K, pad, seed, depth_hw=(2, 2))
    if ragged:
        for r in range(B):
            b[2][r, S - (2 * r + 1) % 4:] = pad
    return model.to(DEV), params, [torch.from_numpy(x) for x in b]


def _wide_engine(model, weight=W):
    eng = model.engine()
    assert eng.steps and eng.H > 256
    eng.wide_supcon = True
    eng.supcon_weight, eng.supcon_temperature = weight, 0.07
    return eng


RNN_SHAPES = [(2, 5, 264, 17, True), (3, 37, 512, 17, False)]


@pytest.mark.parametrize("B,S,H,K,ragged", RNN_SHAPES)
def test_wide_rnn_step_with_supcon_matches_float64(B, S, H, K, ragged):
    """composed as tests/test_supcon_gpu.py::test_rnn_step_with_supcon_matches_float64, at its tolerances"""
    model, params, batch = _rnn(B, S, H, K, ragged)
    pad = K + 1
    if ragged:
        assert bool((batch[2] == pad).any())
    res, sc, grads = _oracle_step(("wide", B, S, H, K), params, batch, pad)
    eng = _wide_engine(model)
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


def test_wide_graphed_and_eager_steps_end_in_identical_parameters():
    from r3d_amd.train_unimodal import _UnimodalSteps
    B, S, H, K, ragged = RNN_SHAPES[0]
    hyper = (5e-3, (0.9, 0.999), 1e-8)
    runs = []
    for graphed in (False, True):
        model, _, batch = _rnn(B, S, H, K, ragged)
        eng = _wide_engine(model)
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


def test_wide_supcon_with_zero_weight_launches_nothing_of_the_term():
    B, S, H, K, ragged = RNN_SHAPES[0]
    runs = []
    for flag in (False, True):
        model, _, batch = _rnn(B, S, H, K, ragged)
        eng = model.engine()
        eng.wide_supcon = flag
        eng.supcon_weight = 0.0
        feats, lab, dur, tgt = _dev(batch)
        eng._shape(B, S, True).sc_ws.fill_(float("nan"))
        loss, counts = eng.train_step(feats, None, lab, dur, tgt, 1e-3, 5e-3)
        torch.cuda.synchronize()
        w = eng.last["w"]
        assert bool(torch.isnan(w.sc_ws).all()) and float(w.sc_loss) == 0.0     # the buffers are there, as without the flag, untouched
        runs.append((loss.clone(), counts.clone(), eng.arena.params.clone(), eng.arena.grads.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    eng.wide_supcon = False
    with pytest.raises(ValueError, match=r"256 columns.*--wide_supcon"):      # without the flag the weight is refused, and says how
        eng.supcon_weight = W
    assert eng.supcon_weight == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the CNN engine at hidden 264 (the composed route), and the loop
# ---------------------------------------------------------------------------------------------------------------------
def test_wide_cnn_step_with_supcon_matches_float64():
    """composed as tests/test_cnn_gpu.py::test_step_with_supcon_matches_float64, at its tolerances"""
    from r3d_amd.model.cnn import FUTR
    B, S, H, K = 2, 5, 264, 17
    pad = K + 1
    model = FUTR(K, H, pad, torch.device(DEV), _args(H), n_query=8, n_head=8, num_encoder_layers=1, num_decoder_layers=1)
    state = synth.fill_state([(n, tuple(p.shape)) for n, p in model.named_parameters()])
    params = {n: torch.from_numpy(v) for n, v in state.items()}
    with torch.no_grad():
        for n, q in model.named_parameters():
            q.copy_(params[n])
    model = model.to(DEV)
    b = synth.make_batch(B, S, K, pad, 3, depth_hw=(2, 2))
    b[2][1, S - 2:] = pad
    batch = [torch.from_numpy(x) for x in b]

    def term(out, bt):
        return W * SO.supcon(out["supcon"].reshape(-1, H), bt[2].reshape(-1), temperature=0.07, base_temperature=0.07,
                             ignore_index=pad, normalize=True)[0]
    tr = CO.Trainer(params, pad, extra=term)
    res, _, _ = tr.step(batch, apply=False)
    eng = model.engine()
    eng.supcon_weight, eng.supcon_temperature = W, 0.07
    feats, lab, dur, tgt = _dev(batch)
    eng.forward(feats, None, lab, "train", training=True)
    assert not eng.last["chain"]                                # hidden 264: the composed route
    with pytest.raises(ValueError, match="wide_supcon"):        # without the flag: refused before anything is enqueued
        eng.losses(lab, tgt, dur, tick=True)
    assert eng.last["w"].sc_ws is None and eng.last["w"].sc_loss is None     # (not even allocated)
    eng.wide_supcon = True
    loss, _ = eng.losses(lab, tgt, dur, tick=True)
    eng.backward()
    grads = {n: eng.arena.g(n).detach().cpu().clone() for n in eng.arena.live_names}
    torch.cuda.synchronize()
    want = [float(res["loss_seg"]), float(res["loss_action"]), float(res["loss_dur"]), float(res["loss"] + res["extra"])]
    print(f"losses {loss.tolist()} oracle {want}")
    for g, r in zip(loss.cpu().double().tolist(), want):
        assert abs(g - r) <= 1e-3 * max(abs(r), 1e-5), (loss.tolist(), want)
    assert abs(W * float(eng.last["w"].sc_loss) - float(res["extra"])) <= 1e-3 * abs(float(res["extra"]))
    for n, g in grads.items():
        if n == "fc_len.bias":              # (zero up to rounding in the oracle: the duration normalisation is shift-invariant)
            continue
        close_rel(g, tr.p[n].grad, n, rtol=1e-3)


def test_train_two_epochs_at_hidden_264_prints_the_supcon_line(tmp_path):
    from r3d_amd import train_unimodal as TU
    from r3d_amd.optim import FlatAdamW
    B, S, H, K = 8, 12, 264, 17
    pad = K + 1
    model, _, _ = _rnn(B, S, H, K, False)
    batches = [[torch.from_numpy(x) for x in synth.make_batch(B, S, K, pad, 20 + i, depth_hw=(2, 2))] for i in range(3)]
    val = [[torch.from_numpy(x) for x in synth.make_batch(1, 9, K, pad, 40, pad_tail=False, depth_hw=(2, 2))]]
    opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)

    class NoSched:
        def step(self):
            pass
    args = _args(H, epochs=2, supcon_weight=W, wide_rnn=True)
    with pytest.raises(ValueError, match=r"256 columns.*--wide_supcon"):      # one flag short
        TU.train(args, model, batches, opt, NoSched(), torch.nn.MSELoss(reduction="none"), str(tmp_path), pad,
                 torch.device(DEV), val, 1)
    args.wide_supcon = True
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TU.train(args, model, batches, opt, NoSched(), torch.nn.MSELoss(reduction="none"), str(tmp_path), pad,
                 torch.device(DEV), val, 1)
    assert model.engine().wide_supcon is True
    lines = buf.getvalue().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("supcon loss :")]
    assert len(at) == 2 and all(lines[i - 1].startswith("seg loss :") for i in at), lines
    for i in at:                                                 # Loss = seg + CE + dur + w * supcon, each printed rounded
        total = float(_NUM.findall(lines[i - 4])[-1])
        ce, dur = float(_NUM.findall(lines[i - 3])[-1]), float(_NUM.findall(lines[i - 2])[-1])
        seg, sc = float(_NUM.findall(lines[i - 1])[0]), float(_NUM.findall(lines[i])[0])
        assert sc > 0.0 and abs(total - (seg + ce + dur + W * sc)) <= 3e-3, lines[i - 4:i + 1]
