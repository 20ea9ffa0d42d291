"""The TCN baseline (reference model/tcn.py + train/train_tcn.py) on the MI355X: the three shifted-operand products and the
weight-norm forward / backward of csrc/tconv.hip against float64 over the pinned shapes, the clip-boundary mask, the whole
step against fixtures generated from the imported reference, determinism, the graphed step, dropout, train() / validate(),
the autograd bridge, checkpoint loading and the shape refusals."""
import contextlib
import io
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import synth
from tests import tcn_cases as TC
from tests import tcn_oracle as TO
from tests.helpers import load_fixture, fixture_params, assert_close, stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = dict(dtype=torch.float64, device=DEV)
fwd_atol = lambda t: 1e-3 * max(1.0, float(t.detach().abs().max()))         # noqa: E731
grad_atol = lambda t: 2e-5 * max(1.0, float(t.detach().abs().max()))        # noqa: E731


def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32) * scale).contiguous()


def _conv_inputs(ci, co, B, S, seed):
    x = _rand((B * S, ci), seed)
    v = _rand((co, ci, 3), seed + 1, (3 * ci) ** -0.5)
    dz = _rand((B * S, co), seed + 2)
    return x, v, dz


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,co,d,B,S", TC.CONV_CASES)
def test_conv_products_match_float64(ci, co, d, B, S):
    from r3d_amd import ops
    N = B * S
    assert ops.tconv_supported(N, S, ci, co, d)
    x, v, dz = _conv_inputs(ci, co, B, S, 11 * B + S)
    ones, zeros = torch.ones(co, device=DEV), torch.zeros(co, device=DEV)
    p, y = torch.empty(N, co, device=DEV), torch.empty(N, co, device=DEV)
    dx, gv = torch.empty(N, ci, device=DEV), torch.empty(co, ci, 3, device=DEV)
    ops.tconv_fwd(x, v, ones, zeros, S, d, y, p_out=p)
    ops.tconv_dx(dz, v, ones, S, d, dx)
    ops.tconv_wgrad(dz, x, None, S, d, gv, ws=torch.empty(max(4, ops.tconv_wgrad_ws_floats(N, ci, co)), device=DEV))
    rp, rdx, rgv = TO.conv_products(x.double().view(B, S, ci), v.double(), dz.double().view(B, S, co), d)
    what = f"{ci}->{co} d{d} B{B} S{S}"
    assert_close(p, rp.reshape(N, co), rtol=1e-3, atol=fwd_atol(rp), what="P " + what)
    assert_close(y, rp.reshape(N, co).clamp(min=0), rtol=1e-3, atol=fwd_atol(rp), what="relu " + what)
    assert_close(dx, rdx.reshape(N, ci), rtol=2e-3, atol=grad_atol(rdx), what="dX " + what)
    assert_close(gv, rgv, rtol=2e-3, atol=grad_atol(rgv), what="G " + what)


@pytest.mark.parametrize("ci,co,d,B,S", TC.CONV_CASES)
def test_weight_norm_forward_backward_match_float64(ci, co, d, B, S):
    from r3d_amd import ops
    N = B * S
    x, v, dy = _conv_inputs(ci, co, B, S, 7 * B + S)
    g, b = _rand((co, 1, 1), 5, 1.0), _rand((co,), 6, 0.1)
    # ReLU units whose pre-activation is within fp32 rounding of the kink (identified from the oracle: |pre| <= 1e-5 max|pre|,
    # the accumulation error of a 6144-term product) may land on either side; their output gradient is set to zero on BOTH
    # sides, so the side they land on does not matter
    with torch.no_grad():
        pre = TO.wn_conv(x.double().view(B, S, ci), v.double(), g.double(), b.double(), d).reshape(N, co)
        dy[pre.abs() <= 1e-5 * float(pre.abs().max())] = 0.0
    s, inv, coef = (torch.empty(co, device=DEV) for _ in range(3))
    p, y, dz = (torch.empty(N, co, device=DEV) for _ in range(3))
    db, dg, dx, dv = torch.empty(co, device=DEV), torch.empty(co, device=DEV), torch.empty(N, ci, device=DEV), torch.empty_like(v)
    ws = torch.empty(max(1, ops.tconv_ws_floats(N, co)), device=DEV)
    ops.tconv_wnorm(v, g, s, inv)
    ops.tconv_fwd(x, v, s, b, S, d, y, p_out=p)
    ops.tconv_bwd_prep(dy, y, p, inv, dz, db, dg, coef, ws)
    ops.tconv_dx(dz, v, s, S, d, dx)
    ops.tconv_wgrad(dz, x, v, S, d, dv, s=s, coef=coef, ws=torch.empty(max(4, ops.tconv_wgrad_ws_floats(N, ci, co)), device=DEV))
    q = [t.double().requires_grad_(True) for t in (x.view(B, S, ci), v, g, b)]
    ry = torch.relu(TO.wn_conv(q[0], q[1], q[2], q[3], d))
    ry.backward(dy.double().view(B, S, co))
    assert_close(s, TO.wn_scale(q[1], q[2]).detach(), rtol=1e-4, atol=1e-6, what="s")
    assert_close(y, ry.detach().reshape(N, co), rtol=1e-3, atol=fwd_atol(ry), what="y")
    assert_close(dx, q[0].grad.reshape(N, ci), rtol=2e-3, atol=grad_atol(q[0].grad), what="dX")
    assert_close(dv, q[1].grad, rtol=2e-3, atol=grad_atol(q[1].grad), what="dv")
    assert_close(dg, q[2].grad.reshape(-1), rtol=2e-3, atol=grad_atol(q[2].grad), what="dg")
    assert_close(db, q[3].grad, rtol=2e-3, atol=grad_atol(q[3].grad), what="db")


@pytest.mark.parametrize("ci,co,d,S", [(512, 256, 8, 17), (256, 512, 2, 3), (2048, 256, 1, 64), (512, 512, 4, 5)])
def test_clip_boundary_mask_is_exact(ci, co, d, S):
    """Altering clip 0's frames (and its output gradients) leaves clip 1's outputs and input gradients bit-identical."""
    from r3d_amd import ops
    B, N = 2, 2 * S
    x, v, dz = _conv_inputs(ci, co, B, S, 3)
    ones, zeros = torch.ones(co, device=DEV), torch.zeros(co, device=DEV)

    def run(x, dz):
        p, y, dx = torch.empty(N, co, device=DEV), torch.empty(N, co, device=DEV), torch.empty(N, ci, device=DEV)
        ops.tconv_fwd(x, v, ones, zeros, S, d, y, p_out=p)
        ops.tconv_dx(dz, v, ones, S, d, dx)
        return p, dx
    p0, dx0 = run(x, dz)
    x2, dz2 = x.clone(), dz.clone()
    x2[:S] = _rand((S, ci), 99, 50.0)
    dz2[:S] = _rand((S, co), 98, 50.0)
    p1, dx1 = run(x2, dz2)
    assert torch.equal(p0[S:], p1[S:]) and torch.equal(dx0[S:], dx1[S:])
    assert not torch.equal(p0[:S], p1[:S])
    # and the other way round: clip 1 altered, clip 0 (whose last frames sit right before clip 1's first) unchanged
    x3, dz3 = x.clone(), dz.clone()
    x3[S:] = _rand((S, ci), 97, 50.0)
    dz3[S:] = _rand((S, co), 96, 50.0)
    p2, dx2 = run(x3, dz3)
    assert torch.equal(p0[:S], p2[:S]) and torch.equal(dx0[:S], dx2[:S])


def test_plain_row_cross_entropy_matches_float64():
    from r3d_amd import ops
    for rows, C, pad in ((16, 17, 16), (64, 122, 123), (104, 17, 3), (8, 1, 5), (24, 300, 7)):
        x = _rand((rows, C), rows + C, 3.0)
        g = torch.Generator().manual_seed(rows)
        tgt = torch.randint(0, C, (rows,), generator=g)
        tgt[::3] = pad
        loss, counts = torch.empty(4, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
        dx = torch.empty(rows, C, device=DEV)
        ops.ce_rows_fwd_bwd(x, tgt.to(DEV), pad, loss, counts, dx)
        q = x.double().cpu().requires_grad_(True)
        rl, nc, nt = TO.loss_counts(q, tgt, pad)
        rl.backward()
        assert abs(float(loss[3]) - float(rl)) <= 1e-4 * max(1.0, float(rl)) and float(loss[1]) == float(loss[3])
        assert counts.tolist() == [0, 0, nc, nt]
        assert_close(dx, q.grad, rtol=2e-3, atol=grad_atol(q.grad), what=f"d_logits {rows}x{C}")


# ---------------------------------------------------------------------------------------------------------------------
# whole step
# ---------------------------------------------------------------------------------------------------------------------
def _model(fx, p_drop=0.0):
    from r3d_amd.model.tcn import MustafaNet1DTCN
    model = MustafaNet1DTCN(num_classes=fx["meta"]["num_classes"], anticipated_frames=8)
    p = fixture_params(fx)
    with torch.no_grad():
        for n, q in model.named_parameters():
            q.copy_(p[n])
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p_drop
    return model.to(DEV)


def _batch(m, seed=None, B=None, S=None):
    b = synth.make_batch(B or m["B"], S or m["S"], m["n_class"], m["pad_idx"], m["seed"] if seed is None else seed,
                         depth_hw=(2, 2))
    return torch.from_numpy(b[0]).to(DEV), torch.from_numpy(b[4]).to(DEV)


def _check_samples(n, t, want, kink_rows, what, grad_ref=None):
    """The 32 recorded elements of a post-AdamW tensor (the first 16 and 16 spread over it: stats()[3:]) at the element
    tolerance: for weight_v (|p| <= 0.06) it is far below lr = 1e-3, so a missing or wrong step shows.  Left out: rows of a
    ReLU unit on the kink (tcn_oracle.kink_channels) and elements whose recorded gradient is below 1e-6 (the first AdamW
    step is sign-like there; the fixture generator leaves the same ones out).
    The recorded GRADIENT elements of the large tensors are not compared one by one: a ReLU unit that lands on the other
    side of its kink moves every weight-gradient element of every layer below it (at tcn_odd, level 0 conv1.weight_v: by up
    to 3.5e-6 on elements of at most 8.8e-4, against an atol of 2e-6), while the first AdamW step, being sign-like, does
    not feel it.  Gradients are held element by element where kink units can be masked on both sides: by
    test_weight_norm_forward_backward_match_float64 over every case, and here through their norms and the full bias /
    weight_g tensors."""
    flat = t.detach().reshape(-1).double().cpu()
    k = flat.numel()
    if k < 16:
        return
    idx = torch.cat([torch.arange(16), torch.linspace(0, k - 1, steps=16).long()])
    row = idx // (k // t.shape[0])
    keep = torch.tensor([int(r) not in kink_rows for r in row])
    ref = torch.from_numpy(np.asarray(want[3:], dtype=np.float64))
    if grad_ref is not None:
        keep &= torch.from_numpy(np.abs(np.asarray(grad_ref[3:], dtype=np.float64)) > 1e-6)
    assert_close(flat[idx][keep], ref[keep], rtol=2e-3, atol=2e-3 * max(1e-3, float(ref.abs().max())), what=f"{what} {n}")


def _loop_batch(m, B, S, seed):
    b = [torch.from_numpy(x) for x in synth.make_batch(B, S, m["n_class"], m["pad_idx"], seed, depth_hw=(2, 2))]
    return b[0], b[2], b[3], b[4], torch.zeros(0)


@pytest.mark.parametrize("tag", [c[0] for c in TC.STEP_CASES])
def test_train_step_matches_reference(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    model = _model(fx).train()
    eng = model.engine()
    feats, tgt = _batch(m)
    N = m["B"] * m["S"]
    for name, shape, dtype in eng.workspace_shapes(m["B"], m["S"]):           # no im2col buffer: nothing of N x 3 C_in
        n = int(np.prod(shape))
        assert not (len(shape) == 2 and shape[0] == N and shape[1] >= 768), (name, shape)
        if dtype == torch.float32 and name != "wgrad_part" and n > max(4096, m["B"] * 8 * m["num_classes"]):
            assert n <= N * 512, (name, shape)                                 # (the smallest im2col would be N x 768)
    cap = []
    with torch.no_grad():                                                       # the oracle's ReLU inputs, float64 on the GPU
        TO.forward({n: q.double().to(DEV) for n, q in fixture_params(fx).items()}, feats.double(), capture=cap)
    kinks = TO.kink_channels(cap)
    loss, counts = eng.train_step(feats, tgt, m["pad_idx"], m["lr"], m["wd"], training=True)
    torch.cuda.synchronize()
    out = eng.last["w"].logits.view(m["B"], 8, -1)
    assert_close(out, fx["out"], rtol=1e-3, atol=fwd_atol(torch.from_numpy(fx["out"])), what="out")
    assert abs(float(loss[3]) - float(fx["loss"])) <= 1e-3 * max(1.0, float(fx["loss"])), (float(loss[3]), float(fx["loss"]))
    assert counts.tolist()[2:] == fx["counts"].tolist()
    for j, n in enumerate(fx["param_names"]):
        gs, want = stats(eng.arena.g(n)), fx["grad_stats"][j]
        assert abs(gs[0] - want[0]) <= 2e-3 * max(1e-3, float(want[0])), (n, gs[0], want[0])
        if "grad::" + n in fx:
            full = fx["grad::" + n]
            keep = [c for c in range(full.shape[0]) if c not in kinks.get(n, ())]     # (see tcn_oracle.kink_channels)
            assert len(keep) >= 0.9 * full.shape[0], (n, sorted(kinks[n]))        # the rule must stay an exception
            assert_close(eng.arena.g(n).cpu()[keep], full[keep], rtol=2e-3, atol=2e-3 * max(1e-3, float(np.abs(full).max())),
                         what=n)
        ps, want = stats(eng.arena.p(n)), fx["post_stats"][j]
        assert abs(ps[0] - want[0]) <= 2e-3 * max(1.0, float(want[0])), (n, ps[0], want[0])
        rows = kinks.get(n.rsplit(".", 1)[0] + ".bias", set())
        _check_samples(n, eng.arena.p(n), fx["post_stats"][j], rows, "post", grad_ref=fx["grad_stats"][j])


@pytest.mark.parametrize("tag", [c[0] for c in TC.STEP_CASES])
def test_eval_forward_matches_reference(tag):
    fx = load_fixture(tag)
    model = _model(fx, p_drop=0.2).eval()
    with torch.no_grad():
        out = model(_batch(fx["meta"])[0])
    assert_close(out, fx["eval_out"], rtol=1e-3, atol=fwd_atol(torch.from_numpy(fx["eval_out"])), what="eval")


@pytest.mark.parametrize("S", [1, 2, 3])
def test_clips_shorter_than_a_shift_train(S):
    fx = load_fixture("tcn_tiny")
    m = fx["meta"]
    model = _model(fx).train()
    eng = model.engine()
    feats, tgt = _batch(m, S=S)
    tr = TO.Trainer(fixture_params(fx), m["pad_idx"], lr=m["lr"], wd=m["wd"])
    rl, nc, nt, rout = tr.step(feats.cpu(), tgt.cpu())
    loss, counts = eng.train_step(feats, tgt, m["pad_idx"], m["lr"], m["wd"], training=True)
    assert_close(eng.last["w"].logits.view(rout.shape), rout, rtol=1e-3, atol=fwd_atol(rout), what="out")
    assert abs(float(loss[3]) - float(rl)) <= 1e-3 * max(1.0, float(rl)) and counts.tolist()[2:] == [nc, nt]
    for n, q in tr.p.items():
        assert_close(eng.arena.p(n), q.detach(), rtol=2e-3, atol=2e-3 * max(1e-3, float(q.abs().max())), what=n)


def _three_steps(fx, graphed, p_drop):
    from r3d_amd.train_tcn import _TcnSteps
    m = fx["meta"]
    model = _model(fx, p_drop=p_drop).train()
    eng = model.engine()
    acc_l = torch.zeros(4, dtype=torch.float64, device=DEV)
    acc_c = torch.zeros(4, dtype=torch.int64, device=DEV)
    gs = _TcnSteps(eng, acc_l, acc_c, pad_idx=m["pad_idx"])
    hyper = (m["wd"], (0.9, 0.999), 1e-8)
    for i in range(3):
        feats, tgt = _batch(m, seed=m["seed"] + i)
        if graphed:
            gs.step([feats, tgt], m["lr"], hyper, True)
        else:
            eng.set_lr(m["lr"])
            gs._enqueue([feats, tgt], m["lr"], hyper, True)
    torch.cuda.synchronize()
    if graphed:
        assert next(iter(gs.shapes.values()))["graph"] is not None      # steps 2 and 3 ran as a captured graph
    assert bool(torch.isfinite(eng.arena.params).all())
    return eng.arena.params.clone(), eng.arena.exp_avg.clone(), eng.arena.exp_avg_sq.clone(), acc_l.clone(), acc_c.clone()


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
def test_two_runs_and_graph_replay_are_bit_identical(p_drop):
    fx = load_fixture("tcn_cfg")
    runs = [_three_steps(fx, False, p_drop), _three_steps(fx, False, p_drop), _three_steps(fx, True, p_drop)]
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert torch.equal(x, y)


def test_dropout_masks():
    fx = load_fixture("tcn_cfg")
    m = fx["meta"]
    model = _model(fx, p_drop=0.2).train()
    eng = model.engine()
    feats, tgt = _batch(m)
    seen = []
    for _ in range(2):
        loss, _ = eng.train_step(feats, tgt, m["pad_idx"], m["lr"], m["wd"], training=True)
        w = eng.last["w"]
        assert eng.last["drop"] and len(w.drop) == 8
        seen.append([d.clone() for d in w.drop])
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(eng.arena.grads).all())
    for a, b in zip(*seen):
        assert not torch.equal(a, b)
        for d in (a, b):
            n = d.numel()
            assert set(d.unique().tolist()) <= {0, 1}
            assert abs(float(d.float().mean()) - 0.8) <= 5 * (0.16 / n) ** 0.5, (n, float(d.float().mean()))
    # the forward applies them: every dropped element of level 0's conv1 output is zero
    y1 = eng.last["w"].y1[0]
    assert bool((y1[seen[1][0].view_as(y1) == 0] == 0).all())
    assert bool(torch.isfinite(eng.arena.params).all())


# ---------------------------------------------------------------------------------------------------------------------
# train() / validate()
# ---------------------------------------------------------------------------------------------------------------------
_NUM = re.compile(r"-?\d+\.\d+|-?\d+")


@pytest.mark.parametrize("flat", [False, True])
def test_train_loop_matches_reference(tmp_path, flat):
    from r3d_amd import train_tcn as TT
    from r3d_amd.optim import FlatAdamW
    fx = load_fixture(TC.TRAIN_LOOP["tag"])
    m = fx["meta"]
    model = _model(fx)
    batches = [_loop_batch(m, m["B"], m["S"], m["seed"] + i) for i in range(m["n_steps"])]
    batches.insert(1, _loop_batch(m, 3, m["S"], m["seed"] + 50))
    val = [_loop_batch(m, 2, m["val_S"], m["seed"] + 100), _loop_batch(m, 1, m["val_S"] + 2, m["seed"] + 101)]
    opt = (FlatAdamW if flat else torch.optim.AdamW)(model.parameters(), m["lr"], weight_decay=m["wd"])

    class Args:
        epochs = m["epochs"]

    class NoSched:
        def step(self):
            pass
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ret = TT.train(Args(), model, batches, val, opt, NoSched(), None, str(tmp_path), m["pad_idx"], torch.device(DEV))
    assert ret is model and model.training is bool(int(fx["training_after"]))      # validate() leaves eval() on
    got, want = buf.getvalue().splitlines(), json.loads(str(fx["stdout"])).splitlines()
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert _NUM.sub("#", g) == _NUM.sub("#", w), (g, w)
        for a, b in zip([float(x) for x in _NUM.findall(g)], [float(x) for x in _NUM.findall(w)]):
            assert abs(a - b) <= 2e-3 * max(1.0, abs(b)) + 1e-3, (g, w)
    assert sorted(os.listdir(tmp_path)) == fx["ckpt_files"]
    keys = list(torch.load(os.path.join(tmp_path, fx["ckpt_files"][0]), weights_only=True).keys())
    assert keys == fx["ckpt_keys"]
    eng = model.engine()
    for j, n in enumerate(fx["param_names"]):
        ps, want = stats(eng.arena.p(n)), fx["post_stats"][-1][j]
        assert abs(ps[0] - want[0]) <= 2e-3 * max(1.0, float(want[0])), (n, ps[0], want[0])


# ---------------------------------------------------------------------------------------------------------------------
# autograd bridge, checkpoints, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_autograd_bridge_gradients():
    fx = load_fixture("tcn_tiny")
    m = fx["meta"]
    model = _model(fx).train()
    feats, tgt = _batch(m)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    out = model(feats)
    loss, _, _ = TO.loss_counts(out, tgt, m["pad_idx"])
    loss.backward()
    tr = TO.Trainer(fixture_params(fx), m["pad_idx"])
    rl, _, _, rout = tr.step(feats.cpu(), tgt.cpu(), apply=False)
    assert_close(out.detach(), rout, rtol=1e-3, atol=fwd_atol(rout), what="out")
    assert abs(float(loss) - float(rl)) <= 1e-3 * max(1.0, float(rl))
    before = {n: q.detach().clone() for n, q in model.named_parameters()}
    for n, q in model.named_parameters():
        want = tr.p[n].grad
        assert q.grad is not None, n
        assert_close(q.grad, want, rtol=2e-3, atol=2e-3 * max(1e-3, float(want.abs().max())), what=n)
    opt.step()
    for n, q in model.named_parameters():
        assert torch.allclose(q.detach(), before[n] - 0.1 * q.grad, rtol=1e-6, atol=1e-7), n


def test_other_optimiser_route_draws_fresh_masks(tmp_path):
    """train() with an optimiser it does not fuse (SGD steps on the arena gradients), dropout on: consecutive steps use
    different keep-masks, and so do consecutive forwards through the autograd bridge."""
    from r3d_amd import train_tcn as TT
    fx = load_fixture(TC.TRAIN_LOOP["tag"])
    m = fx["meta"]
    model = _model(fx, p_drop=0.2)
    seen = []

    class SpySGD(torch.optim.SGD):
        def step(self, closure=None):
            w = model.engine().last["w"]
            assert model.engine().last["drop"]
            seen.append(([d.clone() for d in w.drop], int(model.engine().drop_offset)))
            return super().step(closure)

    class Args:
        epochs = 1

    class NoSched:
        def step(self):
            pass
    batches = [_loop_batch(m, m["B"], m["S"], m["seed"] + i) for i in range(3)]
    before = model.tcn_local.network[0].conv1.weight_v.detach().clone()
    with contextlib.redirect_stdout(io.StringIO()):
        TT.train(Args(), model, batches, [_loop_batch(m, 2, m["val_S"], m["seed"] + 100)], SpySGD(model.parameters(), lr=1e-2),
                 NoSched(), None, str(tmp_path), m["pad_idx"], torch.device(DEV))
    assert len(seen) == 3 and [o for _, o in seen] == [1, 2, 3]
    for (a, _), (b, _) in zip(seen, seen[1:]):
        for x, y in zip(a, b):
            assert not torch.equal(x, y)
    assert not torch.equal(before.to(DEV), model.tcn_local.network[0].conv1.weight_v.detach())
    # the autograd bridge: two train-mode forwards in a row
    model.train()
    eng = model.engine()
    feats = batches[0][0].to(DEV)
    masks = []
    for _ in range(2):
        model(feats).sum().backward()
        masks.append([d.clone() for d in eng.last["w"].drop])
    for x, y in zip(*masks):
        assert not torch.equal(x, y)
        assert abs(float(x.float().mean()) - 0.8) <= 5 * (0.16 / x.numel()) ** 0.5


def test_reference_state_dict_loads_strict():
    fx = load_fixture("tcn_tiny")
    keys, shapes = json.loads(str(fx["state_keys"])), json.loads(str(fx["state_shapes"]))
    p = fixture_params(fx)
    alias = lambda k: k.replace(".net.0.", ".conv1.").replace(".net.4.", ".conv2.")        # noqa: E731
    sd = {k: p[alias(k)].clone() for k in keys}
    assert [list(sd[k].shape) for k in keys] == shapes
    from r3d_amd.model.tcn import MustafaNet1DTCN
    model = MustafaNet1DTCN(num_classes=fx["meta"]["num_classes"]).to(DEV).eval()
    with torch.no_grad():
        model(_batch(fx["meta"])[0])                                       # an engine exists before the load
    r = model.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    with torch.no_grad():
        out = model(_batch(fx["meta"])[0])
    assert_close(out, fx["eval_out"], rtol=1e-3, atol=fwd_atol(torch.from_numpy(fx["eval_out"])), what="eval after load")


def test_refusals_raise_before_any_launch():
    from r3d_amd.model.tcn import MustafaNet1DTCN
    model = MustafaNet1DTCN(num_classes=17).to(DEV)
    big = torch.zeros(1, 1, 2048, device=DEV).expand(1024, 1024, 2048)        # B * S * 2048 = 2^31 (no memory behind it)
    with pytest.raises(ValueError, match=r"2\^31"):
        model(big)
    assert model._engine is None
    with pytest.raises(ValueError, match="window"):
        model(torch.zeros(2, 4, 1024, device=DEV))
    assert model._engine is None
    wide = MustafaNet1DTCN(num_classes=8193).to(DEV)
    with pytest.raises(ValueError, match="regression head"):
        wide(torch.zeros(1, 4, 2048, device=DEV))
    assert wide._engine is None
    from r3d_amd import ops, _lib
    x = torch.zeros(10, 40, device=DEV)
    v = torch.zeros(32, 40, 3, device=DEV)
    with pytest.raises(_lib.R3DHipError):
        ops.tconv_fwd(x, v, torch.ones(32, device=DEV), torch.zeros(32, device=DEV), 5, 1, torch.zeros(10, 32, device=DEV))
