"""The RNN baseline (reference model/rnn.py + train/train_unimodal.py) on the MI355X: the recurrence kernels of
csrc/lstm.hip against a float64 restatement over the pinned shapes, the whole step against fixtures generated from the
imported reference, determinism, the graphed step, train() / validate(), the autograd bridge, the predict path and the
shape refusals."""
import argparse
import contextlib
import io
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import synth
from tests import rnn_oracle as RO
from tests.helpers import load_fixture, fixture_params, assert_close, stats
from tests.rnn_cases import KERNEL_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _args(H, **kw):
    a = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript",
                           hidden_dim=H, n_query=8, n_head=8, epochs=1, task="long", erank_weight=0.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _model(fx, **kw):
    from r3d_amd.model.rnn import FUTR
    m = fx["meta"]
    model = FUTR(m["n_class"], m["H"], m["pad_idx"], torch.device(DEV), _args(m["H"], **kw), n_query=8, n_head=8,
                 num_encoder_layers=2, num_decoder_layers=1)
    p = fixture_params(fx)
    with torch.no_grad():
        for n, q in model.named_parameters():
            q.copy_(p[n])
    return model.to(DEV)


def _batch(fx):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    m = fx["meta"]
    b = synth.make_batch(m["B"], m["S"], m["n_class"], m["pad_idx"], m["seed"], depth_hw=tuple(m["depth_hw"]))
    if m.get("with_exclusion"):
        b[2][0, 1:4] = 120
        b[2][2, 0] = 120
        b[4][1, 0] = 120
        b[4][3, 1] = 120
    return [torch.from_numpy(x) for x in b]


def _dev(batch):
    f, _d, lab, dur, tgt = batch
    return f.to(DEV).contiguous(), lab.to(DEV).contiguous(), dur.to(DEV).contiguous(), tgt.to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the recurrence kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
def _layer_inputs(B, S, H, seed):
    g = torch.Generator().manual_seed(seed)
    h = H // 2
    sd = 1.0 / h ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1)      # noqa: E731
    w = {}
    for d in (0, 1):
        w[("w_ih", d)] = u(4 * h, H) * sd
        w[("w_hh", d)] = u(4 * h, h) * sd
        w[("b_ih", d)] = u(4 * h) * sd
        w[("b_hh", d)] = u(4 * h) * sd
    x = u(B, S, H)
    dy = u(B, S, H) * 0.5
    return {k: v.float().double() for k, v in w.items()}, x.float().double(), dy.float().double()


def _run_layer(B, S, H, w, x, dy):
    from r3d_amd import ops
    from r3d_amd._lib import GEMM_NN, GEMM_TN
    h = H // 2
    N = B * S
    f32 = lambda t: t.to(device=DEV, dtype=torch.float32).contiguous()       # noqa: E731
    w_ih = f32(torch.cat([w[("w_ih", 0)], w[("w_ih", 1)]], 0))
    b_ih = torch.cat([w[("b_ih", 0)], w[("b_ih", 1)]])
    gin = f32(x.reshape(N, H) @ torch.cat([w[("w_ih", 0)], w[("w_ih", 1)]], 0).T + b_ih)
    whh = [f32(w[("w_hh", d)]) for d in (0, 1)]
    bhh = [f32(w[("b_hh", d)]) for d in (0, 1)]
    e = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)   # noqa: E731
    y, gates, cell, hp = e(N, H), e(N, 4 * H), e(N, H), e(N, H)
    ops.lstm_layer_fwd(gin, whh[0], whh[1], bhh[0], bhh[1], y, gates, cell, hp, B, S)
    dg = e(N, 4 * H)
    ops.lstm_layer_bwd(f32(dy.reshape(N, H)), whh[0], whh[1], gates, cell, dg, B, S)
    ws = ops.GemmWorkspace(torch.device(DEV))
    dw_ih, db_ih = e(4 * H, H), e(4 * H)
    ops.gemm(GEMM_TN, dg, f32(x.reshape(N, H)), dw_ih, bias_grad=db_ih, ws=ws)
    dw_hh = [e(4 * h, h), e(4 * h, h)]
    db_hh = [e(4 * h), e(4 * h)]
    for d in (0, 1):
        ops.gemm(GEMM_TN, dg[:, 2 * H * d:2 * H * (d + 1)], hp[:, h * d:h * (d + 1)], dw_hh[d], bias_grad=db_hh[d], ws=ws)
    dx = e(N, H)
    ops.gemm(GEMM_NN, dg, w_ih, dx, ws=ws)
    torch.cuda.synchronize()
    return dict(y=y, gates=gates, cell=cell, hprev=hp, dg=dg, dx=dx, dw_ih=dw_ih, db_ih=db_ih, dw_hh=dw_hh, db_hh=db_hh)


@pytest.mark.parametrize("B,S,H", KERNEL_CASES)
def test_lstm_layer_kernels_match_float64(B, S, H):
    w, x, dy = _layer_inputs(B, S, H, seed=B * 1000 + S * 7 + H)
    ref = RO.lstm_layer_grads(x, w, dy)
    got = _run_layer(B, S, H, w, x, dy)
    N, h = B * S, H // 2
    for k in ("y", "gates", "cell", "hprev"):
        assert_close(got[k].cpu(), ref[k].reshape(N, -1), rtol=1e-3, atol=1e-5, what=f"{k} B{B} S{S} H{H}")
    sc = lambda t: 2e-5 * max(1.0, float(t.abs().max()))       # noqa: E731
    assert_close(got["dg"].cpu(), ref["dg"].reshape(N, -1), rtol=2e-3, atol=sc(ref["dg"]), what="dG")
    assert_close(got["dx"].cpu(), ref["dx"].reshape(N, H), rtol=2e-3, atol=sc(ref["dx"]), what="dX")
    dw_ih = torch.cat(ref["dw_ih"], 0)
    assert_close(got["dw_ih"].cpu(), dw_ih, rtol=2e-3, atol=sc(dw_ih), what="dW_ih")
    db = torch.cat(ref["db"])
    assert_close(got["db_ih"].cpu(), db, rtol=2e-3, atol=sc(db), what="db_ih")
    for d in (0, 1):
        assert_close(got["dw_hh"][d].cpu(), ref["dw_hh"][d], rtol=2e-3, atol=sc(ref["dw_hh"][d]), what=f"dW_hh[{d}]")
        assert_close(got["db_hh"][d].cpu(), ref["db"][d], rtol=2e-3, atol=sc(ref["db"][d]), what=f"db_hh[{d}]")


def test_lstm_kernels_bitwise_reproducible():
    B, S, H = 13, 37, 136
    w, x, dy = _layer_inputs(B, S, H, seed=5)
    a, b = _run_layer(B, S, H, w, x, dy), _run_layer(B, S, H, w, x, dy)
    for k in ("y", "gates", "cell", "hprev", "dg", "dx", "dw_ih"):
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# the whole step against the reference's fixtures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["rnn_tiny", "rnn_cfg"])
def test_step_matches_reference(tag):
    fx = load_fixture(tag)
    model = _model(fx)
    eng = model.engine()
    feats, lab, dur, tgt = _dev(_batch(fx))
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
        if "grad::" + n in fx:
            full = fx["grad::" + n]
            assert_close(grads[n], full, rtol=2e-3, atol=2e-3 * max(1e-3, float(np.abs(full).max())), what=n)
    for j, n in enumerate(fx["live_names"]):
        if n == "fc_len.bias":              # (its gradient is zero up to rounding: AdamW moves it either way)
            continue
        ps, want = stats(eng.arena.p(n)), fx["post_stats"][j]
        assert abs(ps[0] - want[0]) <= 2e-3 * max(1.0, float(want[0])), (n, ps[0], want[0])
    for n in dead:
        assert torch.equal(eng.arena.p(n), before[n]), n


def test_test_mode_forward_b1_matches_reference():
    fx = load_fixture("rnn_tiny")
    model = _model(fx).eval()
    feats = _batch(fx)[0]
    sc = lambda a: 1e-3 * max(1.0, float(np.abs(a).max()))      # noqa: E731
    with torch.no_grad():
        for b in range(feats.shape[0]):                          # B = 1, the bare tensor, as predict_nturgbd calls it
            out = model(feats[b:b + 1].to(DEV), mode="test")
            for k in ("action", "duration", "seg"):
                want = fx["test_" + k][b:b + 1]
                assert_close(out[k].cpu(), want, rtol=1e-3, atol=sc(want), what=k)


def _one_step(model, batch):
    eng = model.engine()
    feats, lab, dur, tgt = batch
    loss, counts = eng.train_step(feats, None, lab, dur, tgt, 1e-3, 5e-3)
    torch.cuda.synchronize()
    return loss.cpu(), counts.cpu(), eng.arena.params.clone(), eng.arena.grads.clone()


def test_two_runs_bit_identical():
    fx = load_fixture("rnn_cfg")
    batch = _dev(_batch(fx))
    a = _one_step(_model(fx), batch)
    b = _one_step(_model(fx), batch)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_graphed_replay_bit_identical_to_eager():
    from r3d_amd.train_unimodal import _UnimodalSteps
    fx = load_fixture("rnn_cfg")
    feats, lab, dur, tgt = _dev(_batch(fx))
    hyper = (5e-3, (0.9, 0.999), 1e-8)
    runs = []
    for graphed in (False, True):
        model = _model(fx)
        eng = model.engine()
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
            st = next(iter(gs.shapes.values()))
            assert st["graph"] is not None                        # steps 2 and 3 ran as a captured graph
        runs.append((eng.arena.params.clone(), eng.arena.exp_avg.clone(), acc_l.clone(), acc_c.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# train() / validate()
# ---------------------------------------------------------------------------------------------------------------------
_NUM = re.compile(r"-?\d+\.\d+|-?\d+")


def _numbers(s):
    return [float(x) for x in _NUM.findall(s)]


@pytest.mark.parametrize("flat", [False, True])
def test_train_loop_matches_reference(tmp_path, flat):
    from r3d_amd import train_unimodal as TU
    from r3d_amd.optim import FlatAdamW
    fx = load_fixture("rnn_train_loop")
    m = fx["meta"]
    model = _model(fx)
    batches = []
    for i in range(m["n_steps"]):
        b = synth.make_batch(m["B"], m["S"], m["n_class"], m["pad_idx"], m["seed"] + i, depth_hw=tuple(m["depth_hw"]))
        b[2][0, 1:4] = 120
        b[2][2, 0] = 120
        b[4][1, 0] = 120
        b[4][3, 1] = 120
        batches.append([torch.from_numpy(x) for x in b])
    batches.insert(1, [torch.from_numpy(x) for x in synth.make_batch(3, m["S"], m["n_class"], m["pad_idx"], m["seed"] + 50,
                                                                       depth_hw=tuple(m["depth_hw"]))])
    val = [[torch.from_numpy(x) for x in synth.make_batch(1, m["val_S"], m["n_class"], m["pad_idx"], m["seed"] + 100,
                                                          pad_tail=False, depth_hw=tuple(m["depth_hw"]))]]
    opt = (FlatAdamW if flat else torch.optim.AdamW)(model.parameters(), 1e-3, weight_decay=5e-3)

    class NoSched:
        def step(self):
            pass
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TU.train(_args(m["H"]), model, batches, opt, NoSched(), torch.nn.MSELoss(reduction="none"), str(tmp_path),
                 m["pad_idx"], torch.device(DEV), val, m["seed"])
    got, want = buf.getvalue().splitlines(), json.loads(str(fx["stdout"])).splitlines()
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert _NUM.sub("#", g) == _NUM.sub("#", w), (g, w)
        for a, b in zip(_numbers(g), _numbers(w)):
            assert abs(a - b) <= 2e-3 * max(1.0, abs(b)) + 1e-3, (g, w)
    assert sorted(os.listdir(tmp_path)) == fx["ckpt_files"]
    keys = list(torch.load(os.path.join(tmp_path, fx["ckpt_files"][0]), weights_only=True).keys())
    assert keys == fx["ckpt_keys"]
    with contextlib.redirect_stdout(io.StringIO()):
        vres = TU.validate(model, val, torch.nn.MSELoss(reduction="none"), m["pad_idx"], torch.device(DEV))
    assert_close(torch.tensor(vres, dtype=torch.float64), fx["val_result"], rtol=2e-3, atol=1e-4, what="validate")
    live = fx["live_names"]
    eng = model.engine()
    for j, n in enumerate(live):
        if n == "fc_len.bias":
            continue
        ps, want = stats(eng.arena.p(n)), fx["post_stats"][-1][j]
        assert abs(ps[0] - want[0]) <= 2e-3 * max(1.0, float(want[0])), (n, ps[0], want[0])


# ---------------------------------------------------------------------------------------------------------------------
# autograd bridge, predict path, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_autograd_bridge_gradients():
    fx = load_fixture("rnn_tiny")
    model = _model(fx).train()
    feats, lab = _batch(fx)[0], _batch(fx)[2]
    g = torch.Generator().manual_seed(7)
    out = model((feats.to(DEV), lab.to(DEV)))
    coef = {k: torch.randn(out[k].shape, generator=g, dtype=torch.float64) for k in ("action", "duration", "seg", "supcon")}
    loss = sum((out[k].double() * coef[k].to(DEV)).sum() for k in coef)
    loss.backward()
    p = {n: t.double().requires_grad_(RO.is_live(n)) for n, t in fixture_params(fx).items()}
    ro = RO.forward(p, feats.double())
    sum((ro[k] * coef[k]).sum() for k in coef).backward()
    for n, q in model.named_parameters():
        if not RO.is_live(n):
            assert q.grad is None, n
            continue
        want = p[n].grad
        assert_close(q.grad.cpu(), want, rtol=2e-3, atol=2e-3 * max(1e-3, float(want.abs().max())), what=n)


def test_predict_nturgbd_on_synthetic_videos():
    from r3d_amd.predict import predict_nturgbd
    fx = load_fixture("rnn_tiny")
    m = fx["meta"]
    n_actions = m["n_class"] - 1
    actions = {f"act{i:02d}": i for i in range(n_actions)}
    videos = {}
    for v in range(3):
        feats, _dep, lines = synth.make_video(40 + 9 * v, n_actions, 20 + v, depth_hw=(2, 2))
        videos[f"vid{v}"] = (feats, lines)

    class Reader:
        def exists(self, base):
            return base in videos

        def load(self, base):
            feats, lines = videos[base]
            return base, [ln.split(",")[0] for ln in lines], [ln.split(",")[1] for ln in lines], feats, \
                np.zeros((len(lines), 1, 2, 2), np.float32)

    model = _model(fx)
    args = argparse.Namespace(sample_rate=1, dataset="nturgbd")
    details = []
    with contextlib.redirect_stdout(io.StringIO()):
        ant, seg = predict_nturgbd(model, [f"vid{v}.txt" for v in range(3)], args, 0.5, m["n_class"], actions, DEV,
                                   reader=Reader(), details=details)
    assert len(details) == 3 and np.isfinite(ant) and np.isfinite(seg)
    p = {n: t.double() for n, t in fixture_params(fx).items()}
    for d in details:
        feats, lines = videos[d["video"]]
        T = len(lines)
        ro = RO.forward(p, torch.from_numpy(np.ascontiguousarray(feats[:int(0.5 * T)])).double().unsqueeze(0))
        ok_seg = (ro["seg"][0].argmax(-1) == d["seg_labels"]).double().mean()
        ok_act = (ro["action"][0].argmax(-1) == d["action_labels"]).double().mean()
        assert ok_seg >= 0.9 and ok_act >= 0.875, (d["video"], float(ok_seg), float(ok_act))


@pytest.mark.parametrize("H,n_query,erank", [(264, 8, 0.0), (12, 8, 0.0), (128, 9, 0.0)])
def test_engine_refuses_before_any_launch(H, n_query, erank):
    from r3d_amd.model.rnn import FUTR
    model = FUTR(17, H, 18, torch.device(DEV), _args(H), n_query=n_query, n_head=4, num_encoder_layers=1, num_decoder_layers=1)
    model = model.to(DEV)
    with pytest.raises(ValueError):
        model.engine()
    assert model._engine is None


def test_train_refuses_erank_weight_before_any_launch(tmp_path):
    from r3d_amd import train_unimodal as TU
    fx = load_fixture("rnn_tiny")
    model = _model(fx)
    with pytest.raises(ValueError, match="erank_weight"):
        TU.train(_args(16, erank_weight=0.1), model, [], torch.optim.AdamW(model.parameters()), None, None, str(tmp_path),
                 fx["meta"]["pad_idx"], torch.device(DEV), [], 1)
    assert model._engine is None
