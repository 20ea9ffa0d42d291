"""The effective-rank Jacobi over every shape the rank penalty admits (tests/erank_cases.py), against float64.

MATRICES rows, kernel level: sigma against svdvals, the effective rank, the rotated columns (orthogonal, norms sigma; with
the basis carried, X V reconstructs them and V is orthogonal), the zero padding of the blocked kernel's af_t, convergence
before the sweeps enqueued, and the gradient of the effective rank against float64 autograd through svdvals.
STEPS rows: one rank-penalised training step at the row's shape takes the row's route, converges, reports the effective
rank of its fused tokens and hands the penalty's gradient to the backward (against float64 autograd through svdvals of the
step's own fused tokens; "model" rows: every parameter gradient against the CPU oracle); refused rows raise before any
launch.  Plus: the penalised step replayed as a hipGraph equals the eager step, and a second backward over one sweep
gives the first one's gradient bit for bit."""
import argparse
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import futr_oracle as O, synth  # noqa: E402
from tests import erank_cases as EC  # noqa: E402
from tests import width_cases as WC  # noqa: E402
from tests.helpers import assert_close  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

ARGS = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
SWEEPS = 30                     # sweeps enqueued by the kernel-level rows (ops.erank_jacobi / erank_blocked's default)


@pytest.fixture(scope="module")
def ops():
    from r3d_amd import ops
    return ops


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def spectrum(k, kind):
    if kind == "sep":
        return torch.linspace(0.2, 2.0, k, dtype=torch.float64).flip(0)
    base = torch.logspace(0, -4, k // 4, dtype=torch.float64)                   # sigma_max / sigma_min = 1e4
    sv = (base[:, None] * (1.0 + 1e-3 * torch.arange(4, dtype=torch.float64))[None, :]).reshape(-1)
    sv = torch.sort(sv, descending=True)[0] * 50.0
    if sv.numel() < k:
        sv = torch.cat([sv, sv[-1:].repeat(k - sv.numel()) * 0.5])
    return sv


def make_matrix(R, C, kind, seed):
    """fp64 [R, C] with the prescribed singular values (rank min(R, C))."""
    k = min(R, C)
    q1 = torch.linalg.qr(_rnd(R, k, seed=seed))[0]
    q2 = torch.linalg.qr(_rnd(C, k, seed=seed + 1))[0]
    return q1 @ torch.diag(spectrum(k, kind)) @ q2.t()


def erank64(x):
    """float64 effective rank and its gradient (autograd through svdvals)."""
    xr = x.detach().double().cpu().clone().requires_grad_(True)
    er = O.effective_rank_torch(xr)
    er.backward()
    return float(er.detach()), xr.grad


def _grad_err(got, want):
    return float((got.double().cpu() - want).abs().max()) / float(want.abs().max())


def _launch(ops, m, xs):
    """Runs the row's kernel on the fp32 matrices xs (one, or the batch).  Returns per matrix (sigma [C], stats [4],
    A [C, R] rotated columns, vt or None) and, for the blocked route, its buffers."""
    R, C = m.R, m.C
    dev = "cuda"
    if m.route == "blocked":
        bufs = ops.ErankBlockedBufs(R, C, dev, max_sweeps=SWEEPS)
        bufs.af_full.fill_(float("nan"))                # the kernel must write every element of it, padding included
        x = xs[0]
        if m.layout == "xt":
            ops.erank_blocked_into(x.t().contiguous().cuda(), bufs, transposed=True)
        elif m.layout == "ld":
            big = torch.full((R, C + 9), float("nan"), device=dev)
            big[:, :C] = x.cuda()
            ops.erank_blocked_into(big[:, :C], bufs)
        else:
            ops.erank_blocked_into(x.cuda(), bufs)
        torch.cuda.synchronize()
        return [(bufs.sigma, bufs.stats, bufs.af_t, None)], bufs
    n = len(xs)
    sig, st, aft = torch.empty(n, C, device=dev), torch.empty(n, 4, device=dev), torch.empty(n, C, R, device=dev)
    if m.route == "warm":
        vt = torch.empty(C, C, device=dev)
        ops.erank_jacobi_warm(xs[0].cuda(), sig, st, vt, af_t=aft)
        torch.cuda.synchronize()
        return [(sig[0], st[0], aft[0], vt)], None
    if isinstance(m.layout, tuple):                       # ("batch", n, extra): padded batch stride, NaN in the padding
        extra = m.layout[2]
        big = torch.full((n, R + extra, C), float("nan"), device=dev)
        for b in range(n):
            big[b, :R] = xs[b].cuda()
        x = big[:, :R]
    elif m.layout == "ld":
        big = torch.full((R, C + 9), float("nan"), device=dev)
        big[:, :C] = xs[0].cuda()
        x = big[:, :C]
    else:
        x = xs[0].cuda()
    ops.erank_jacobi(x, sig, st, af_t=aft)
    torch.cuda.synchronize()
    return [(sig[b], st[b], aft[b], None) for b in range(n)], None


@pytest.mark.parametrize("m", EC.MATRICES, ids=EC.matrix_id)
def test_matrix_row_against_fp64(ops, m):
    from r3d_amd.erank import ErankBackward, effective_rank
    t0 = time.time()
    R, C = m.R, m.C
    k = min(R, C)
    p = ops.erank_plan(R, C, warm=m.route == "warm", blocked=m.route == "blocked")
    assert EC.plan_key(p, m.route) == m.plan
    n = m.layout[1] if isinstance(m.layout, tuple) else 1
    x64 = [make_matrix(R, C, m.spectrum, seed=R + 7 * C + 101 * b) for b in range(n)]
    xs = [x.float() for x in x64]
    outs, bufs = _launch(ops, m, xs)
    gtol = 2e-3 if m.spectrum == "sep" else 3e-3
    worst_sig, worst_grad, sweeps = 0.0, 0.0, []
    for b, (sig, st, A, vt) in enumerate(outs):
        x = xs[b]
        sv = torch.linalg.svdvals(x.double())
        smax = float(sv[0])
        got = torch.sort(sig.cpu().double(), descending=True)[0]
        assert_close(got[:k], sv[:k], 1e-4, 1e-4 * smax, f"{EC.matrix_id(m)}[{b}] sigma")
        worst_sig = max(worst_sig, float((got[:k] - sv[:k]).abs().max()) / smax)
        if C > k:
            assert float(got[k:].abs().max()) <= 1e-5 * smax, f"surplus sigma {float(got[k:].abs().max()):.3e}"
        er_ref, g_ref = erank64(x)
        er = float(st[0])
        assert abs(er - er_ref) < 5e-3 * max(1.0, er_ref / 50), (er, er_ref)
        sweeps.append(float(st[3]))
        assert float(st[3]) < SWEEPS, f"{EC.matrix_id(m)}: not converged in {SWEEPS} sweeps"
        # the rotated columns: orthogonal, norms sigma (same order)
        Ad = A.cpu().double()
        assert torch.isfinite(Ad).all()
        G = Ad @ Ad.t()
        off = G - torch.diag(torch.diag(G))
        assert float(off.abs().max()) < 1e-3 * smax ** 2, float(off.abs().max()) / smax ** 2
        assert float((torch.diag(G).clamp_min(0).sqrt() - sig.cpu().double()).abs().max()) <= 1e-4 * smax
        if vt is not None:
            V = vt.cpu().double().t()
            assert float((V.t() @ V - torch.eye(C, dtype=torch.float64)).abs().max()) < 1e-4
            assert float((x.double() @ V - Ad.t()).abs().max()) < 4e-4 * smax
        # the gradient from this launch's own outputs (the backward the training step runs)
        xd = x.cuda()
        dx = torch.empty_like(xd)
        gout = torch.ones(1, device="cuda")
        ErankBackward(R, C, False, "cuda", ld=A.stride(0)).run(xd, A, sig, st, gout, dx, False, ops.GemmWorkspace("cuda"))
        torch.cuda.synchronize()
        e = _grad_err(dx, g_ref)
        worst_grad = max(worst_grad, e)
        assert e <= gtol, f"{EC.matrix_id(m)}[{b}]: gradient error / scale {e:.2e}"
    if bufs is not None:                                  # the padding of af_t ([Cpad, Rp]) is exactly 0
        full = bufs.af_full.cpu()
        assert torch.equal(full[C:], torch.zeros_like(full[C:])), "padding rows of af_t"
        assert torch.equal(full[:, R:], torch.zeros_like(full[:, R:])), "row tails of af_t"
    if m.layout == "plain" and m.route in ("lds", "blocked"):
        # and through the differentiable op
        xg = xs[0].cuda().requires_grad_(True)
        er_t = effective_rank(xg, route=m.route)
        er_t.backward()
        torch.cuda.synchronize()
        e = _grad_err(xg.grad, erank64(xs[0])[1])
        worst_grad = max(worst_grad, e)
        assert e <= gtol, f"{EC.matrix_id(m)}: effective_rank(route={m.route}) gradient error / scale {e:.2e}"
    print(f"[erank matrix {EC.matrix_id(m)} plan {m.plan}] sigma err/max {worst_sig:.2e}, sweeps "
          f"{'/'.join(f'{s:.0f}' for s in sweeps)}, gradient err/scale {worst_grad:.2e} ({time.time() - t0:.1f} s)")


# ------------------------------------------------------------------------------------------------------------------
# training steps
# ------------------------------------------------------------------------------------------------------------------
def _model(s):
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    model = FUTR(EC.K, s.H, EC.K + 1, torch.device("cuda"), ARGS, n_query=EC.Q, n_head=s.heads, num_encoder_layers=2,
                 num_decoder_layers=1)
    names = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    params = {n: torch.from_numpy(v) for n, v in synth.fill_state(names).items()}
    missing = model.load_state_dict(params, strict=False)
    assert not missing.unexpected_keys
    return model.to("cuda").eval(), params


def _device_batch(s, seed=77):
    """The row's batch generated on the device (the "fused" rows: the oracle needs only the step's fused tokens)."""
    B, S, pad_idx = s.B, s.S, EC.K + 1
    g = torch.Generator(device="cuda").manual_seed(seed)
    feats = (torch.rand(B, S, 2048, device="cuda", generator=g) * 2 - 1) * math.sqrt(3.0)
    depth = torch.rand(B, S, 1, 224, 224, device="cuda", generator=g)
    lab = torch.randint(0, EC.K - 1, (B, S), device="cuda", generator=g)
    if s.pad == "tail":
        lab[1::2, S - max(S // 8, 1):] = pad_idx
    small = synth.make_batch(B, 1, EC.K, pad_idx, seed)
    return [feats, depth, lab, torch.from_numpy(small[3]).cuda(), torch.from_numpy(small[4]).cuda()]


ADMITTED = [s for s in EC.STEPS if s.refuse is None]
REFUSED = [s for s in EC.STEPS if s.refuse is not None]


@pytest.mark.parametrize("s", ADMITTED, ids=EC.step_id)
def test_step_row_against_fp64(ops, s, oracle_lib, monkeypatch):
    t0 = time.time()
    N, H = s.B * s.S, s.H
    model, params = _model(s)
    if s.check == "model":
        batch = WC.make_batch(WC._c(s.B, s.S, H, s.heads, pad=s.pad))
        d = [t.cuda() for t in batch]
    else:
        d = _device_batch(s)
    eng = model.engine()
    eng.erank_weight = EC.LAM
    eng.erank_warm_start = s.warm
    calls = []
    for nm in ("erank_jacobi", "erank_jacobi_warm", "erank_blocked_into"):
        fn = getattr(ops, nm)
        monkeypatch.setattr(ops, nm, lambda *a, _fn=fn, _nm=nm, **kw: (calls.append(_nm), _fn(*a, **kw))[1])
    eng.forward(d[0], d[1], d[2], "train", training=False)
    eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    w = eng.last["w"]
    # ---- the route the engine took
    assert (w.er_blk is None) == (s.route == "lds")
    if w.er_blk is not None:
        assert bool(w.er_flip) == s.flip and calls == ["erank_blocked_into"], calls
        R, C = (H, N) if s.flip else (N, H)
        assert (w.er_blk.R, w.er_blk.C) == (R, C)
        assert EC.plan_key(ops.erank_plan(R, C, blocked=True), "blocked") == s.plan
        cap = eng.erank_max_sweeps
    else:
        assert calls == (["erank_jacobi_warm"] if s.used else ["erank_jacobi"]), calls
        assert EC.plan_key(ops.erank_plan(N, H, warm=s.used), "lds") == s.plan
        cap = SWEEPS
    assert any(isinstance(k, tuple) and k[0] == "bwd_chain" for k in w.tables) == s.chain, sorted(map(str, w.tables))
    sweeps = float(w.er_stats[0, 3])
    assert sweeps < cap, f"{EC.step_id(s)}: {sweeps:.0f} sweeps, {cap} enqueued"
    # ---- the effective rank and the penalty's gradient with respect to the fused tokens, on the step's own tokens
    fused = w.fused.reshape(N, H)
    er_ref, g_ref = erank64(fused)
    got = float(eng.erank_value())
    assert abs(got - er_ref) < 5e-3 * max(1.0, er_ref / 50), (got, er_ref)
    if N < H and w.er_blk is None:                        # rank <= N: every surplus sigma is 0
        sg = torch.sort(w.er_sigma[0].cpu().double(), descending=True)[0]
        assert float(sg[N:].abs().max()) <= 1e-5 * float(sg[0]), float(sg[N:].abs().max()) / float(sg[0])
    buf = torch.empty_like(fused)
    eng._erank_backward(w, ops.GemmWorkspace("cuda"), dst=buf)        # a second backward over the step's sweep
    torch.cuda.synchronize()
    e_fused = _grad_err(buf, -EC.LAM * g_ref)
    # (1e-2 of scale: fp32 singular vectors of the smallest sigma, see test_effective_rank_penalty_gradients)
    assert e_fused <= 1e-2, f"{EC.step_id(s)}: penalty gradient w.r.t. the fused tokens, error / scale {e_fused:.2e}"
    worst = (0.0, "")
    if s.check == "model":
        tr = O.CpuTrainer(params, EC.K + 1, s.heads, 1)
        out, aux = O.forward(tr.p, (batch[0], batch[2]), batch[1], "train", EC.K + 1, s.heads, 1)
        res = O.losses(out, batch[2], batch[3], batch[4], EC.K + 1)
        er_o = O.effective_rank_torch(aux["fused"].reshape(-1, H).double())
        assert abs(got - float(er_o)) < 5e-3 * max(1.0, float(er_o) / 50), (got, float(er_o))
        (res["loss"] - EC.LAM * er_o.float()).backward()
        for n, p in tr.p.items():
            if p.grad is not None:
                g, r = eng.arena.g(n).double().cpu(), p.grad.double()
                worst = max(worst, (float((g - r).abs().max()) / max(float(r.abs().max()), 1e-5), n))
        assert worst[0] <= 1e-2, worst
    print(f"[erank step {EC.step_id(s)} {N}x{H} {s.route}{' flip' if s.flip else ''} plan {s.plan}] erank {got:.4f} vs "
          f"{er_ref:.4f}, sweeps {sweeps:.0f} (of {cap}), d fused err/scale {e_fused:.2e}"
          + (f", worst parameter gradient {worst[0]:.2e} ({worst[1]})" if s.check == "model" else "")
          + f" ({time.time() - t0:.1f} s)")


@pytest.mark.parametrize("s", REFUSED, ids=EC.step_id)
def test_step_row_refused_before_any_launch(ops, s, monkeypatch):
    from tests.test_width_shapes_gpu import Recorder
    model, _ = _model(s)
    eng = model.engine()
    eng.erank_weight = EC.LAM
    B, S = s.B, s.S
    feats = torch.zeros(B, S, 2048, device="cuda")
    depth = torch.zeros(B, S, 224 * 224, device="cuda")
    lab = torch.full((B, S), EC.K + 1, dtype=torch.int64, device="cuda")
    rec = Recorder(monkeypatch)
    calls = []
    for nm in ("erank_jacobi", "erank_jacobi_warm", "erank_blocked_into", "gemm"):
        fn = getattr(ops, nm)
        monkeypatch.setattr(ops, nm, lambda *a, _fn=fn, _nm=nm, **kw: (calls.append(_nm), _fn(*a, **kw))[1])
    with pytest.raises(ValueError, match=s.refuse):
        eng.forward(feats, depth, lab, "train", training=False)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert not rec.calls and not calls and not eng.shapes, (rec.names(), calls)


# ------------------------------------------------------------------------------------------------------------------
# the penalised step as a replayed hipGraph; a second backward over one sweep
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,H", [(10, 32, 128), (8, 64, 512)])
def test_graphed_penalised_step_equals_eager(ops, B, S, H):
    """train()'s graphed step (train_proposed_depth._GraphedSteps: eager, then captured + replayed, then replayed) with
    the rank penalty on, against the same steps enqueued eagerly: losses and parameters within 1e-6 relative.  320 x 128
    on the chain (blocked, b 16) and cfg4's 512 x 512 (blocked, 32 blocks): the blocked launches and the side-stream fork
    inside a captured graph."""
    from r3d_amd.train_proposed_depth import _GraphedSteps
    s = EC._s(B, S, H)
    batch = [t.cuda() for t in WC.make_batch(WC._c(B, S, H, 8))]
    hyper = (5e-3, (0.9, 0.999), 1e-8)
    runs = []
    for graphed in (False, True):
        model, _ = _model(s)
        eng = model.engine()
        eng.erank_weight = EC.LAM
        acc_loss = torch.zeros(4, dtype=torch.float64, device="cuda")
        acc_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        gs = _GraphedSteps(eng, acc_loss, acc_cnt)
        trace = []
        for _ in range(3):
            if graphed:
                gs.step(batch, 1e-3, hyper, False)
            else:
                eng.set_lr(1e-3)
                gs._enqueue(batch, 1e-3, hyper, False)
            torch.cuda.synchronize()
            trace.append((acc_loss.clone(), eng.arena.params.clone(), float(eng.last["w"].er_stats[0, 3])))
        if graphed:
            st = next(iter(gs.shapes.values()))
            assert st["graph"] is not None, "the step was not captured"
        assert eng.last["w"].er_blk is not None
        runs.append(trace)
    for i, ((l0, p0, s0), (l1, p1, s1)) in enumerate(zip(*runs)):
        assert float((l0 - l1).abs().max()) <= 1e-6 * float(l0.abs().max()), (i, l0, l1)
        assert float((p0 - p1).abs().max()) <= 1e-6 * float(p0.abs().max()), (i, float((p0 - p1).abs().max()))
        assert s1 < 16 and s0 < 16
    assert not torch.equal(runs[0][0][1], runs[0][2][1]), "the steps changed no parameter"
    print(f"[erank graphed {B * S}x{H}] sweeps eager {[t[2] for t in runs[0]]} graphed {[t[2] for t in runs[1]]}")


@pytest.mark.parametrize("route,R,C", [("lds", 200, 64), ("blocked", 520, 512), ("blocked", 64, 300)])
def test_second_backward_over_one_sweep_is_bit_identical(route, R, C):
    """effective_rank(x).backward(retain_graph=True) twice: the backward must not consume what the sweep saved (it used to
    scale the rotated columns in place to U^T, so the second pass applied 1 / sigma again)."""
    from r3d_amd.erank import effective_rank
    x = make_matrix(R, C, "sep", seed=5).float().cuda().requires_grad_(True)
    er = effective_rank(x, route=route)
    er.backward(retain_graph=True)
    torch.cuda.synchronize()
    g1 = x.grad.clone()
    x.grad = None
    er.backward(retain_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g1, x.grad), float((g1 - x.grad).abs().max()) / float(g1.abs().max())
    e = _grad_err(g1, erank64(x)[1])
    assert e <= 2e-3, e
