"""The stepwise LSTM route (csrc/lstm_steps.hip, opts --wide_rnn) on the MI355X: its kernels against float64 over the pinned
shapes of tests/rnn_wide_cases.py with the measured bounds, determinism, agreement with the registers route where both
exist, the whole training step at hidden 264 and 512 against fixtures generated from the imported reference, the graphed
step, train() / validate() and the refusal without the flag."""
import contextlib
import io
import json
import math

import numpy as np
import pytest
import torch

from oracle import synth
from tests import rnn_wide_cases as WC
from tests.helpers import load_fixture, assert_close, stats
from tests.test_rnn_gpu import DEV, _args, _batch, _dev, _model, _numbers, _run_layer

pytestmark = pytest.mark.gpu


def _run_layer_steps(B, S, H, w, x, dy):
    """test_rnn_gpu._run_layer with the recurrence on the stepwise kernels; every output buffer starts as NaN."""
    from r3d_amd import ops
    from r3d_amd._lib import GEMM_NN, GEMM_TN
    h, N = H // 2, B * S
    f32 = lambda t: t.to(device=DEV, dtype=torch.float32).contiguous()       # noqa: E731
    w_ih = f32(torch.cat([w[("w_ih", 0)], w[("w_ih", 1)]], 0))
    b_ih = torch.cat([w[("b_ih", 0)], w[("b_ih", 1)]])
    gin = f32(x.reshape(N, H) @ torch.cat([w[("w_ih", 0)], w[("w_ih", 1)]], 0).T + b_ih)
    whh = [f32(w[("w_hh", d)]) for d in (0, 1)]
    bhh = [f32(w[("b_hh", d)]) for d in (0, 1)]
    e = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)   # noqa: E731
    y, gates, cell, hp = e(N, H), e(N, 4 * H), e(N, H), e(N, H)
    ops.lstm_steps_layer_fwd(gin, whh[0], whh[1], bhh[0], bhh[1], y, gates, cell, hp, B, S)
    dg, lws = e(N, 4 * H), e(ops.lstm_steps_ws_floats(B, H))
    ops.lstm_steps_layer_bwd(f32(dy.reshape(N, H)), whh[0], whh[1], gates, cell, dg, B, S, lws)
    ws = ops.GemmWorkspace(torch.device(DEV))
    dw_ih, db_ih = e(4 * H, H), e(4 * H)
    ops.gemm(GEMM_TN, dg, f32(x.reshape(N, H)), dw_ih, bias_grad=db_ih, ws=ws)
    dw_hh, db_hh = e(8 * h, h), e(8 * h)
    for d in (0, 1):
        ops.gemm(GEMM_TN, dg[:, 2 * H * d:2 * H * (d + 1)], hp[:, h * d:h * (d + 1)], dw_hh[4 * h * d:4 * h * (d + 1)],
                 bias_grad=db_hh[4 * h * d:4 * h * (d + 1)], ws=ws)
    dx = e(N, H)
    ops.gemm(GEMM_NN, dg, w_ih, dx, ws=ws)
    torch.cuda.synchronize()
    return dict(y=y, gates=gates, cell=cell, hprev=hp, dg=dg, dx=dx, dw_ih=dw_ih, db_ih=db_ih, dw_hh=dw_hh, db_hh=db_hh)


@pytest.mark.parametrize("B,S,H", WC.ALL_CASES)
def test_step_kernels_match_float64(B, S, H):
    w, x, dy = WC.inputs(B, S, H)
    WC.check(_run_layer_steps(B, S, H, w, x, dy), B, S, H, what="steps")


def test_step_kernels_bitwise_reproducible():
    B, S, H = 13, 37, 1024
    w, x, dy = WC.inputs(B, S, H)
    a, b = _run_layer_steps(B, S, H, w, x, dy), _run_layer_steps(B, S, H, w, x, dy)
    for k in WC.TENSORS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("B,S,H", WC.NARROW_CASES)
def test_steps_route_against_registers_route(B, S, H):
    w, x, dy = WC.inputs(B, S, H)
    st = _run_layer_steps(B, S, H, w, x, dy)
    rg = _run_layer(B, S, H, w, x, dy)
    rg["dw_hh"], rg["db_hh"] = torch.cat(rg["dw_hh"], 0), torch.cat(rg["db_hh"])
    WC.check(st, B, S, H, what="steps")
    WC.check(rg, B, S, H, what="registers")
    _, bounds = WC.reference(B, S, H)
    for k in WC.TENSORS:
        err = float((st[k].double() - rg[k].double()).abs().max())
        print(f"steps - registers B{B} S{S} H{H} {k}: {err:.3e} bound {bounds[k][0]:.3e}")
        assert err <= bounds[k][0], (k, err, bounds[k][0])


# ---------------------------------------------------------------------------------------------------------------------
# the whole step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["rnn_wide_264", "rnn_wide_512"])
def test_wide_step_matches_reference(tag):
    from r3d_amd.engine_rnn import lstm_route
    fx = load_fixture(tag)
    model = _model(fx, wide_rnn=True)
    eng = model.engine()
    assert eng.steps and lstm_route(eng.H, eng.wide) == "steps"
    feats, lab, dur, tgt = _dev(_batch(fx))
    if tag == "rnn_wide_512":
        assert bool((lab == 120).any()) and bool((tgt == 120).any())
    dead = json.loads(str(fx["dead_names"]))
    before = {n: eng.arena.p(n).clone() for n in dead}
    out = eng.forward(feats, None, lab, "train", training=True)
    res = {k: v.detach().cpu().clone() for k, v in out.items()}
    loss, counts = eng.losses(lab, tgt, dur, tick=True)
    eng.backward()
    grads = {n: eng.arena.g(n).detach().cpu().clone() for n in fx["live_names"]}
    eng.adamw(1e-3, 5e-3, ticked=True)
    torch.cuda.synchronize()
    sc = lambda a: 1e-3 * max(1.0, float(np.abs(a).max()))      # noqa: E731
    for k in ("action", "duration", "seg"):
        assert_close(res[k], fx["out_" + k], rtol=1e-3, atol=sc(fx["out_" + k]), what=k)
    assert_close(torch.tensor(stats(res["supcon"])[:3]), fx["supcon_stats"][:3], rtol=1e-3, atol=1e-3, what="supcon")
    assert_close(loss.cpu(), fx["losses"], rtol=1e-3, atol=1e-4, what="losses")
    assert counts.cpu().tolist() == fx["counts"].tolist()
    assert sorted(eng.arena.live_names) == sorted(fx["live_names"])
    for j, n in enumerate(fx["live_names"]):
        gs, want = stats(grads[n]), fx["grad_stats"][j]
        lim = 2e-3 * max(1e-3, float(want[0]))
        assert abs(gs[0] - want[0]) <= lim, (n, gs[0], want[0])
    for j, n in enumerate(fx["live_names"]):
        if n == "fc_len.bias":              # (its gradient is zero up to rounding: AdamW moves it either way)
            continue
        ps, want = stats(eng.arena.p(n)), fx["post_stats"][j]
        assert abs(ps[0] - want[0]) <= 2e-3 * max(1.0, float(want[0])), (n, ps[0], want[0])
    for n in dead:
        assert torch.equal(eng.arena.p(n), before[n]), n


def test_forced_steps_route_matches_reference_at_hidden_128():
    """use_lstm_steps = True at a hidden size the registers route takes: the same step, the same fixture."""
    fx = load_fixture("rnn_cfg")
    feats, lab, dur, tgt = _dev(_batch(fx))
    runs = []
    for force in (None, True):
        eng = _model(fx).engine()
        eng.use_lstm_steps = force
        assert eng.steps is bool(force)
        loss, _ = eng.train_step(feats, None, lab, dur, tgt, 1e-3, 5e-3)
        torch.cuda.synchronize()
        runs.append((loss.cpu(), eng.arena.grads.cpu()))
    assert_close(runs[1][0], fx["losses"], rtol=1e-3, atol=1e-4, what="losses")
    g0, g1 = runs[0][1], runs[1][1]
    assert float((g0 - g1).abs().max()) <= 2e-3 * float(g0.abs().max())


def test_wide_graphed_replay_bit_identical_to_eager():
    from r3d_amd.train_unimodal import _UnimodalSteps
    fx = load_fixture("rnn_wide_512")
    feats, lab, dur, tgt = _dev(_batch(fx))
    hyper = (5e-3, (0.9, 0.999), 1e-8)
    runs = []
    for graphed in (False, True):
        eng = _model(fx, wide_rnn=True).engine()
        acc_l = torch.zeros(4, dtype=torch.float64, device=DEV)
        acc_c = torch.zeros(4, dtype=torch.int64, device=DEV)
        gs = _UnimodalSteps(eng, acc_l, acc_c)
        for _ in range(3):
            if graphed:
                gs.step([feats, lab, dur, tgt], 1e-3, hyper, True)
            else:
                gs._enqueue([feats, lab, dur, tgt], 1e-3, hyper, True)
        torch.cuda.synchronize()
        if graphed:
            assert next(iter(gs.shapes.values()))["graph"] is not None     # steps 2 and 3 ran as a captured graph
        runs.append((eng.arena.params.clone(), eng.arena.exp_avg.clone(), acc_l.clone(), acc_c.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(runs[0][2]).all())


def test_wide_train_and_validate_two_epochs_repeatable(tmp_path):
    from r3d_amd import train_unimodal as TU
    fx = load_fixture("rnn_wide_264")
    m = fx["meta"]
    mk = lambda B, S, seed, **kw: [torch.from_numpy(x) for x in synth.make_batch(        # noqa: E731
        B, S, m["n_class"], m["pad_idx"], seed, depth_hw=tuple(m["depth_hw"]), **kw)]
    batches = [mk(m["B"], m["S"], m["seed"] + i) for i in range(2)]
    val = [mk(1, m["S"] + 3, m["seed"] + 100, pad_tail=False)]

    class NoSched:
        def step(self):
            pass
    outs = []
    for run in range(2):
        model = _model(fx, wide_rnn=True)
        opt = torch.optim.AdamW(model.parameters(), 1e-3, weight_decay=5e-3)
        buf = io.StringIO()
        ckpt = tmp_path / f"run{run}"
        ckpt.mkdir()
        with contextlib.redirect_stdout(buf):
            TU.train(_args(m["H"], wide_rnn=True, epochs=2), model, batches, opt, NoSched(), torch.nn.MSELoss(reduction="none"),
                     str(ckpt), m["pad_idx"], torch.device(DEV), val, m["seed"])
            vres = TU.validate(model, val, torch.nn.MSELoss(reduction="none"), m["pad_idx"], torch.device(DEV))
        assert model.engine().steps
        nums = _numbers(buf.getvalue())
        assert len(nums) > 8 and all(math.isfinite(v) for v in nums) and all(math.isfinite(float(v)) for v in vres)
        assert "nan" not in buf.getvalue().lower()
        outs.append((buf.getvalue(), tuple(float(v) for v in vres), model.engine().arena.params.clone()))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    assert torch.equal(outs[0][2], outs[1][2])


# ---------------------------------------------------------------------------------------------------------------------
# the flag
# ---------------------------------------------------------------------------------------------------------------------
def test_hidden_512_refused_without_the_flag():
    from r3d_amd.model.rnn import FUTR
    model = FUTR(17, 512, 18, torch.device(DEV), _args(512), n_query=8, n_head=8, num_encoder_layers=1,
                 num_decoder_layers=1).to(DEV)
    with pytest.raises(ValueError, match="--wide_rnn"):
        model.engine()
    assert model._engine is None


def test_entry_script_flags_build_a_wide_engine():
    from r3d_amd import opts
    from r3d_amd.model.rnn import FUTR
    args = opts.parser.parse_args(["--hidden_dim", "512", "--wide_rnn"])
    args.n_query = 8
    model = FUTR(17, args.hidden_dim, device=torch.device(DEV), args=args, src_pad_idx=18, n_query=args.n_query,
                 n_head=args.n_head, num_encoder_layers=1, num_decoder_layers=1).to(DEV)
    eng = model.engine()
    assert eng.steps and eng.H == 512
    with pytest.raises(ValueError, match="256 columns"):
        eng.supcon_weight = 0.5
    assert eng.supcon_weight == 0.0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from r3d_amd import ops
    B, S, H = 2, 3, 264
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)      # noqa: E731
    whh, bhh = z(2 * H, H // 2), z(2 * H)
    with pytest.raises(Exception, match="R3D_EINVAL"):
        ops.lstm_steps_layer_fwd(z(B * S, 4 * 1032), z(2 * 1032, 516), z(2 * 1032, 516), z(2 * 1032), z(2 * 1032),
                                 z(B * S, 1032), z(B * S, 4 * 1032), z(B * S, 1032), z(B * S, 1032), B, S)
    gin = z(B * S, 4 * H + 1)[:, 1:]                                       # a misaligned view
    with pytest.raises(Exception, match="R3D_EALIGN"):
        ops.lstm_steps_layer_fwd(gin, whh, whh, bhh, bhh, z(B * S, H), z(B * S, 4 * H), z(B * S, H), z(B * S, H), B, S)
    torch.cuda.synchronize()
