"""The tall rank route on the GPU (tests/erank_tall_cases.py): the blocked fold kernel alone against float64, ErankTall
against float64 autograd through svdvals with both folds, rank-penalised training steps on the route (eager and
graphed), a train() run with --erank_route tall, and every refusal before a launch."""
import argparse
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import erank_cases as EC  # noqa: E402
from tests import erank_tall_cases as TC  # noqa: E402
from tests import erank_tall_oracle as TO  # noqa: E402
from tests import width_cases as WC  # noqa: E402
from tests.test_erank_shapes_gpu import _device_batch, _grad_err, _model, erank64, make_matrix  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from r3d_amd import ops
    return ops


def _widest(ops):
    return max(H for H in range(16, 2049, 16) if ops.qr_fold_wy_supported(H))


def _fold(ops, x, lanes, H):
    """x: fp32 device [n, H] view -> merged R [H, H] (cpu, float64) and the accumulators as the fold left them."""
    R = torch.zeros(lanes, H, H, device="cuda")
    ops.qr_fold_wy(x, R)
    lanes_out = R.clone()
    ops.qr_merge(R)
    torch.cuda.synchronize()
    return R[0].cpu().double().numpy(), lanes_out


def _check_fold(R, x, lanes, tag):
    """R [H, H] float64 (merged) against the float64 Gram matrix and singular values of x (numpy fp32 [n, H])."""
    n, H = x.shape
    x64 = x.astype(np.float64)
    assert np.isfinite(R).all(), tag
    assert not np.tril(R, -1).any(), f"{tag}: R is not upper triangular"
    G = x64.T @ x64
    e_gram = np.linalg.norm(R.T @ R - G) / np.linalg.norm(G)
    sv = np.linalg.svd(x64, compute_uv=False)
    sv = np.concatenate([sv, np.zeros(H - sv.size)])
    smax = sv[0]
    got = np.sort(np.linalg.svd(R, compute_uv=False))[::-1]
    e_sig = np.abs(got - sv).max() / smax
    ref32 = TO.merge(TO.fold(x, lanes, np.float32)).astype(np.float64)
    e_ref = np.abs(np.sort(np.linalg.svd(ref32, compute_uv=False))[::-1] - sv).max() / smax
    print(f"[fold wy {tag}] sigma err/max {e_sig:.2e} (fp32 restatement {e_ref:.2e}), gram err {e_gram:.2e} "
          f"(bound {TC.gram_tol(n, H):.2e})")
    assert e_gram <= TC.gram_tol(n, H), f"{tag}: ||R^T R - X^T X|| / ||X^T X|| = {e_gram:.2e}"
    assert e_sig <= max(TC.SIGMA_FACTOR * e_ref, TC.SIGMA_FLOOR), f"{tag}: sigma error {e_sig:.2e}, fp32 restatement {e_ref:.2e}"


# ------------------------------------------------------------------------------------------------------------------
# the fold kernel alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", TC.FOLD_H + ["widest"])
def test_fold_kernel_against_fp64(ops, H):
    H = _widest(ops) if H == "widest" else H
    T = ops.qr_fold_wy_tile_rows(H)
    assert T >= 32 and T % 16 == 0
    for n in TC.FOLD_N + [2 * T + 7]:
        x = TC.fold_input(n, H, seed=n + 13 * H)
        xd = torch.from_numpy(x).cuda()
        for lanes in TC.FOLD_LANES:
            R, per_lane = _fold(ops, xd, lanes, H)
            _check_fold(R, x, lanes, f"H{H} n{n} lanes{lanes}")
            per = -(-n // lanes)
            for g in range(lanes):                       # a lane without rows is left as it was
                if g * per >= n:
                    assert not per_lane[g].any(), (H, n, lanes, g)


@pytest.mark.parametrize("H", [48, 128])
def test_fold_kernel_zero_column_zero_rows_strided_and_repeatable(ops, H):
    T = ops.qr_fold_wy_tile_rows(H)
    n = 2 * T + 7
    x = TC.fold_input(n, H, seed=5 + H, kind="zeros")
    xd = torch.from_numpy(x).cuda()
    R, lanes1 = _fold(ops, xd, 3, H)
    _check_fold(R, x, 3, f"H{H} zero column / zero rows")
    assert not R[:, H // 3].any(), "the all-zero column of X must stay an all-zero column of R"
    # the same call twice: the same bits
    _, lanes2 = _fold(ops, xd, 3, H)
    assert torch.equal(lanes1, lanes2)
    # a row-strided input (ldx > H), NaN in the padding
    big = torch.full((n, H + 9), float("nan"), device="cuda")
    big[:, :H] = xd
    _, lanes3 = _fold(ops, big[:, :H], 3, H)
    assert torch.equal(lanes1, lanes3)
    # folding on top of what is there: two halves in sequence give the Gram matrix of the whole
    Racc = torch.zeros(2, H, H, device="cuda")
    ops.qr_fold_wy(xd[:T + 3], Racc)
    ops.qr_fold_wy(xd[T + 3:], Racc)
    ops.qr_merge(Racc)
    torch.cuda.synchronize()
    _check_fold(Racc[0].cpu().double().numpy(), x, 2, f"H{H} two calls")


def test_fold_kernel_refusals_before_any_launch(ops):
    from r3d_amd._lib import R3DHipError
    widest = _widest(ops)
    for H in (8, 24, 100, widest + 16, 2048):
        assert not ops.qr_fold_wy_supported(H) and ops.qr_fold_wy_tile_rows(H) == 0
        R = torch.full((2, H, H), float("nan"), device="cuda")
        x = torch.ones(40, H, device="cuda")
        with pytest.raises(R3DHipError, match="R3D_EINVAL"):
            ops.qr_fold_wy(x, R)
        torch.cuda.synchronize()
        assert torch.isnan(R).all()
    R = torch.full((2, 64, 64), float("nan"), device="cuda")
    with pytest.raises(ValueError):
        ops.qr_fold_wy(torch.ones(40, 48, device="cuda"), R)
    with pytest.raises(R3DHipError, match="R3D_EINVAL"):
        ops.qr_fold_wy(torch.ones(40, 64, device="cuda"), torch.zeros(65, 64, 64, device="cuda"))
    ops.qr_fold_wy(torch.ones(0, 64, device="cuda"), R)                   # n = 0: a no-op
    torch.cuda.synchronize()
    assert torch.isnan(R).all()


# ------------------------------------------------------------------------------------------------------------------
# the route: ErankTall against float64
# ------------------------------------------------------------------------------------------------------------------
_REF = {}


def _route_ref(N, H, kind):
    """(fp32 matrix, float64 effective rank, float64 gradient), computed once per (N, H, spectrum) and left unchanged."""
    key = (N, H, kind)
    if key not in _REF:
        x = make_matrix(N, H, kind, seed=N + 7 * H).float()
        er, g = erank64(x)
        _REF[key] = (x, er, g)
    return _REF[key]


@pytest.mark.parametrize("fold", TC.FOLDS)
@pytest.mark.parametrize("kind", TC.SPECTRA)
@pytest.mark.parametrize("N,H", TC.ROUTE)
def test_route_against_fp64(ops, N, H, kind, fold):
    from r3d_amd.erank import ErankTall, effective_rank
    t0 = time.time()
    x, er_ref, g_ref = _route_ref(N, H, kind)
    xd = x.cuda()
    tall = ErankTall(N, H, "cuda", fold=fold)
    assert tall.fold == fold and (tall.blk is None) == ops.erank_fits(2 * H, H)
    sigma, stats = tall.forward(xd)
    dx = torch.full_like(xd, float("nan"))
    tall.backward(xd, torch.ones(1, device="cuda"), dx, False, ops.GemmWorkspace("cuda"))
    torch.cuda.synchronize()
    er = float(stats[0, 0])
    assert float(stats[0, 3]) < tall.max_sweeps, "the sweep on R did not converge"
    assert abs(er - er_ref) < TC.ER_TOL * max(1.0, er_ref / 50), (er, er_ref)
    sv = torch.linalg.svdvals(x.double())
    got = torch.sort(sigma[0].cpu().double(), descending=True)[0]
    assert float((got - sv).abs().max()) <= 1e-4 * float(sv[0])
    e = _grad_err(dx, g_ref)
    # accumulate: out += gout * gradient, and a second backward over one forward gives the same bits
    acc = dx.clone()
    tall.backward(xd, torch.full((1,), -0.5, device="cuda"), acc, True, ops.GemmWorkspace("cuda"))
    dx2 = torch.empty_like(xd)
    tall.backward(xd, torch.ones(1, device="cuda"), dx2, False, ops.GemmWorkspace("cuda"))
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)
    assert float((acc - 0.5 * dx).abs().max()) <= 1e-5 * float(dx.abs().max())
    # and through the differentiable op
    xg = xd.clone().requires_grad_(True)
    effective_rank(xg, route="tall", fold=fold).backward()
    torch.cuda.synchronize()
    e_op = _grad_err(xg.grad, g_ref)
    print(f"[tall route {N}x{H} {kind} {fold} lanes {tall.lanes}] erank {er:.5f} vs {er_ref:.5f}, sweeps {float(stats[0, 3]):.0f}, "
          f"gradient err/scale {e:.2e} (op {e_op:.2e}) ({time.time() - t0:.1f} s)")
    assert e <= TC.GRAD_TOL_KERNEL, f"gradient error / scale {e:.2e}"
    assert e_op <= TC.GRAD_TOL_KERNEL, f"effective_rank(route='tall') gradient error / scale {e_op:.2e}"


def test_effective_rank_tall_refusals(ops):
    from r3d_amd.erank import ErankTall, effective_rank
    with pytest.raises(ValueError, match="N >= H"):
        effective_rank(torch.zeros(63, 64, device="cuda"), route="tall")
    with pytest.raises(ValueError, match="2048"):
        effective_rank(torch.zeros(2100, 2064, device="cuda"), route="tall")
    with pytest.raises(ValueError, match="wy"):
        ErankTall(4096, 1024, "cuda", fold="wy")
    with pytest.raises(ValueError, match="lanes"):
        ErankTall(4096, 128, "cuda", lanes=65)


# ------------------------------------------------------------------------------------------------------------------
# training steps on the tall route
# ------------------------------------------------------------------------------------------------------------------
def _estep(s):
    return EC._s(s.B, s.S, s.H, s.heads, pad="tail" if isinstance(s.pad, str) else "none")


def _batch(s):
    if isinstance(s.pad, str):
        return _device_batch(_estep(s))
    return [t.cuda() for t in WC.make_batch(WC._c(s.B, s.S, s.H, s.heads, pad=s.pad))]


def _engine(s, route, fold=None):
    model, _ = _model(_estep(s))
    eng = model.engine()
    eng.erank_weight = TC.LAM
    eng.erank_route = route
    eng.erank_fold = fold
    return eng


def _run_step(eng, d):
    eng.forward(d[0], d[1], d[2], "train", training=False)
    eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("s", TC.STEPS, ids=TC.step_id)
def test_step_on_the_tall_route_against_fp64(ops, s, monkeypatch):
    t0 = time.time()
    N, H = s.B * s.S, s.H
    d = _batch(s)
    calls = []
    for nm in ("erank_jacobi", "erank_jacobi_warm", "erank_blocked_into", "qr_fold_wy", "qr_append", "qr_merge"):
        fn = getattr(ops, nm)
        monkeypatch.setattr(ops, nm, lambda *a, _fn=fn, _nm=nm, **kw: (calls.append(_nm), _fn(*a, **kw))[1])
    got = {}
    for fold in TC.FOLDS:
        eng = _engine(s, "tall", fold)
        eng.erank_warm_start = True                      # ignored on the tall route
        del calls[:]
        _run_step(eng, d)
        w = eng.last["w"]
        sweep = "erank_jacobi" if ops.erank_fits(2 * H, H) else "erank_blocked_into"
        assert calls == [{"wy": "qr_fold_wy", "column": "qr_append"}[fold], "qr_merge", sweep], calls
        assert w.er_tall.max_sweeps == (30 if sweep == "erank_jacobi" else eng.erank_max_sweeps)
        assert w.er_tall.fold == fold and (w.er_tall.N, w.er_tall.H) == (N, H)
        chain = any(isinstance(k, tuple) and k[0] == "bwd_chain" for k in w.tables)
        assert s.chain is None or chain == s.chain, sorted(map(str, w.tables))
        assert float(w.er_tall.stats[0, 3]) < w.er_tall.max_sweeps
        fused = w.fused.reshape(N, H)
        er_ref, g_ref = erank64(fused)
        er = float(eng.erank_value())
        assert abs(er - er_ref) < TC.ER_TOL * max(1.0, er_ref / 50), (er, er_ref)
        buf = torch.empty_like(fused)
        eng._erank_backward(w, ops.GemmWorkspace("cuda"), dst=buf)
        torch.cuda.synchronize()
        e = _grad_err(buf, -TC.LAM * g_ref)
        sg = w.er_tall.sigma[0]
        print(f"[tall step {TC.step_id(s)} {N}x{H} {fold}] sigma min/max {float(sg.min() / sg.max()):.1e}, "
              f"erank {er:.4f} vs {er_ref:.4f}, d fused err/scale {e:.2e} "
              f"({time.time() - t0:.1f} s)")
        assert e <= TC.GRAD_TOL_STEP, f"{TC.step_id(s)} {fold}: penalty gradient w.r.t. the fused tokens {e:.2e}"
        got[fold] = (er, eng.arena.grads.clone())
    monkeypatch.undo()
    if (s.B, s.S, s.H) == TC.JACOBI_REFUSES:
        with pytest.raises(ValueError, match="--erank_route tall admits it"):
            _run_step(_engine(s, "jacobi"), d)
    if (s.B, s.S, s.H) == TC.BOTH_ROUTES:
        # the two routes on one batch: the same effective rank and the same parameter gradients to the routes' precision
        eng = _engine(s, "jacobi")
        _run_step(eng, d)
        er_j, g_j = float(eng.erank_value()), eng.arena.grads
        for fold, (er, g) in got.items():
            assert abs(er - er_j) < TC.ER_TOL, (fold, er, er_j)
            assert float((g - g_j).abs().max()) <= TC.GRAD_TOL_STEP * float(g_j.abs().max()), fold


@pytest.mark.parametrize("s", TC.STEPS, ids=TC.step_id)
def test_graphed_step_on_the_tall_route_equals_eager_bit_for_bit(ops, s):
    """train()'s graphed step (eager, then captured + replayed, then replayed) against the same steps enqueued eagerly."""
    from r3d_amd.train_proposed_depth import _GraphedSteps
    d = _batch(s)
    hyper = (5e-3, (0.9, 0.999), 1e-8)
    runs = []
    for graphed in (False, True):
        eng = _engine(s, "tall")
        acc_loss = torch.zeros(4, dtype=torch.float64, device="cuda")
        acc_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        gs = _GraphedSteps(eng, acc_loss, acc_cnt)
        trace = []
        for _ in range(3):
            if graphed:
                gs.step(d, 1e-3, hyper, False)
            else:
                eng.set_lr(1e-3)
                gs._enqueue(d, 1e-3, hyper, False)
            torch.cuda.synchronize()
            trace.append((acc_loss.clone(), eng.arena.params.clone(), eng.last["w"].er_tall.stats.clone()))
        if graphed:
            st = next(iter(gs.shapes.values()))
            assert st["graph"] is not None, "the step was not captured"
        runs.append(trace)
    for i, ((l0, p0, s0), (l1, p1, s1)) in enumerate(zip(*runs)):
        assert torch.equal(s0, s1), (i, s0, s1)
        assert torch.equal(l0, l1), (i, l0, l1)
        assert torch.equal(p0, p1), (i, float((p0 - p1).abs().max()))
    assert not torch.equal(runs[0][0][1], runs[0][2][1]), "the steps changed no parameter"


def test_jacobi_route_gives_the_bits_recorded_before_the_flag_existed(ops, monkeypatch):
    """erank_route = "jacobi" (the default) at (4, 80, 128): none of the tall route's kernels is launched, and the step's
    fused tokens, singular values, rank statistics and parameter gradients are bit for bit what the build before this
    route existed gave on an MI355X (tests/golden/erank_jacobi_4x80x128.json: float hex and SHA-256 of the buffers' bytes,
    recorded from that build with this batch)."""
    import hashlib
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "erank_jacobi_4x80x128.json")))
    s = next(r for r in TC.STEPS if (r.B, r.S, r.H) == TC.BOTH_ROUTES)
    d = _batch(s)
    calls = []
    for nm in ("qr_fold_wy", "qr_append", "qr_merge"):
        fn = getattr(ops, nm)
        monkeypatch.setattr(ops, nm, lambda *a, _fn=fn, _nm=nm, **kw: (calls.append(_nm), _fn(*a, **kw))[1])
    model, _ = _model(_estep(s))
    eng = model.engine()
    assert eng.erank_route == "jacobi"
    eng.erank_weight = TC.LAM
    _run_step(eng, d)
    w = eng.last["w"]
    assert not calls and (w.er_blk is not None) == gold["blocked"] and not hasattr(w, "er_tall")

    def sha(t):
        return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()
    assert sha(w.fused) == gold["fused_sha256"], "the fused tokens moved: not the penalty's doing"
    assert [float(v).hex() for v in w.er_stats[0].cpu()] == gold["er_stats"]
    assert sha(w.er_sigma) == gold["sigma_sha256"]
    assert sha(eng.arena.grads) == gold["grads_sha256"]


def test_refusals_raise_before_any_launch(ops, monkeypatch):
    from tests.test_width_shapes_gpu import Recorder
    s = EC._s(1, 63, 64, 4, pad="none")
    model, _ = _model(s)
    eng = model.engine()
    eng.erank_weight = TC.LAM
    eng.erank_route = "tall"
    feats = torch.zeros(1, 63, 2048, device="cuda")
    depth = torch.zeros(1, 63, 224 * 224, device="cuda")
    lab = torch.full((1, 63), EC.K + 1, dtype=torch.int64, device="cuda")
    rec = Recorder(monkeypatch)
    calls = []
    for nm in ("erank_jacobi", "erank_blocked_into", "qr_fold_wy", "qr_append", "qr_merge", "gemm"):
        fn = getattr(ops, nm)
        monkeypatch.setattr(ops, nm, lambda *a, _fn=fn, _nm=nm, **kw: (calls.append(_nm), _fn(*a, **kw))[1])
    with pytest.raises(ValueError, match="N >= H"):
        eng.forward(feats, depth, lab, "train", training=False)
    eng.grad_hook = lambda stage: None                   # what a data-parallel wrapper installs
    with pytest.raises(ValueError, match="one GPU"):
        eng.forward(feats, depth, lab, "train", training=False)
    eng.grad_hook = None
    eng.erank_route = "gram"
    with pytest.raises(ValueError, match="erank_route"):
        eng.forward(feats, depth, lab, "train", training=False)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert not rec.calls and not calls and not eng.shapes, (rec.names(), calls)
    from r3d_amd.parallel import DataParallelStep
    eng.erank_route = "tall"
    with pytest.raises(ValueError, match="one GPU"):
        DataParallelStep(eng)


# ------------------------------------------------------------------------------------------------------------------
# train() with --erank_route tall
# ------------------------------------------------------------------------------------------------------------------
def test_train_two_epochs_on_the_tall_route(tmp_path):
    """train() with --erank_weight 0.05 --erank_route tall on synthetic clips: graphed steps, two epochs, finite losses,
    and the engine took the tall route."""
    import contextlib
    import io
    import math
    import re
    from r3d_amd.optim import FlatAdamW
    from r3d_amd.opts import parser
    from r3d_amd.train_proposed_depth import train
    s = EC._s(8, 40, 128)
    model, _ = _model(s)
    batches = [_device_batch(s, seed=300 + i) for i in range(2)]
    val = [[t[:1] for t in _device_batch(EC._s(2, 40, 128), seed=999)]]
    opt = parser.parse_args(["--erank_weight", "0.05", "--erank_route", "tall"])
    args = argparse.Namespace(epochs=2, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=1,
                              erank_weight=opt.erank_weight, erank_route=opt.erank_route)

    class NoSched:
        def step(self):
            pass
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train(args, model, batches, FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3), NoSched(), None, str(tmp_path),
              EC.K + 1, torch.device("cuda"), val, seed=0)
    torch.cuda.synchronize()
    losses = [float(x) for x in re.findall(r"Loss : (-?[0-9.]+|nan|inf)", buf.getvalue())]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses), buf.getvalue()
    eng = model.engine()
    assert eng.erank_route == "tall" and any(hasattr(v, "er_tall") for v in eng.shapes.values()), list(eng.shapes)
