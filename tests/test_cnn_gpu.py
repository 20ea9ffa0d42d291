"""The CNN baseline (reference model/cnn.py + train/train_unimodal.py) on the MI355X: the segmentation-head step kernel
(csrc/cnn.hip) against the float64 restatement over every case of tests/cnn_cases.py with that file's tolerances, its
refusals, the whole step on both routes against fixtures generated from the imported reference, route agreement,
determinism, the graphed step, validation and test-mode forwards, train() end to end, --supcon_weight, the predict path
and the refusals of the rank penalty and the rank report."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import synth
from tests import cnn_cases as CC, cnn_oracle as CO, supcon_oracle as SO
from tests.helpers import load_fixture, fixture_params, assert_close, stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = ["cnn_tiny", "cnn_cfg", "cnn_odd"]
ROUTES = [False, True]          # use_seg_chain


def _args(H, **kw):
    a = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript",
                           hidden_dim=H, n_query=8, n_head=8, epochs=1, task="long", erank_weight=0.0, temperature=0.07)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _model(fx, **kw):
    from r3d_amd.model.cnn import FUTR
    m = fx["meta"]
    model = FUTR(m["n_class"], m["H"], m["pad_idx"], torch.device(DEV), _args(m["H"], **kw), n_query=8, n_head=8,
                 num_encoder_layers=2, num_decoder_layers=1)
    p = fixture_params(fx)
    with torch.no_grad():
        for n, q in model.named_parameters():
            q.copy_(p[n])
    return model.to(DEV)


def _batch(fx, seed=None, B=None, S=None, exclusion=None, **kw):
    m = fx["meta"]
    b = synth.make_batch(B or m["B"], S or m["S"], m["n_class"], m["pad_idx"], m["seed"] if seed is None else seed,
                         depth_hw=tuple(m["depth_hw"]), **kw)
    if m.get("with_exclusion") if exclusion is None else exclusion:
        b[2][0, 1:4] = 120
        b[2][2, 0] = 120
        b[4][1, 0] = 120
        b[4][3, 1] = 120
    return [torch.from_numpy(x) for x in b]


def _dev(batch):
    f, _d, lab, dur, tgt = batch
    return f.to(DEV).contiguous(), lab.to(DEV).contiguous(), dur.to(DEV).contiguous(), tgt.to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# r3d_cnn_seg_step against float64
# ---------------------------------------------------------------------------------------------------------------------
def _run_kernel(c, seg=True, extra=False, strided=False):
    from r3d_amd import ops
    N, H, K = c["N"], c["H"], c["K"]
    t = lambda a: torch.from_numpy(a).to(DEV)        # noqa: E731
    x, d_x0 = t(c["x"]), t(c["d_x0"])
    if strided:                                      # columns [8, 8 + H) of a wider buffer: row stride H + 12
        wide = lambda v: torch.cat([torch.full((N, 8), 7.0, device=DEV), v, torch.full((N, 4), 7.0, device=DEV)], 1)[:, 8:8 + H]   # noqa: E731
        x, d_x0 = wide(x), wide(d_x0)
        assert x.stride(0) == H + 12 and d_x0.stride(0) == H + 12
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)       # noqa: E731
    out = dict(seg=nan(N, K) if seg else None, d_seg=nan(N, K), d_pre=nan(N, H), ws=nan(4 * N + 4))
    ops.cnn_seg_step(x, t(c["w"]), t(c["b"]), t(c["labels"]), c["pad_idx"], CC.EXCLUDE, out["d_seg"], out["d_pre"], out["ws"],
                     seg=out["seg"], d_x0=d_x0, d_extra=t(c["d_extra"]) if extra else None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("row", CC.CASES, ids=lambda r: "N%d-H%d-K%d-%s" % r[:4])
def test_seg_step_kernel_matches_float64(row):
    c = CC.make_case(*row[:5])
    ref, tol = CC.reference(c), CC.tolerances(row)
    N = c["N"]
    a = _run_kernel(c)
    units = a["ws"][:4 * N].view(N, 4)[:, :3].cpu().double().numpy()
    got = dict(logits=a["seg"], loss=units[:, 0], d_seg=a["d_seg"], d_pre0=a["d_pre"])
    for q, v in got.items():
        v = v.cpu().double().numpy() if torch.is_tensor(v) else v
        err = CC.rel_err(v, ref[q])
        print(f"{q}: error {err:.3e} tolerance {tol[q]:.3e}")
        assert err <= tol[q], (row[:5], q, err, tol[q])
    # flags and counters: exact (a missed + 2 penalty is a loss error of 2, far outside the loss tolerance above)
    assert np.array_equal(units[:, 1:], ref["units"][:, 1:]), row[:5]
    assert torch.isnan(a["ws"][4 * N:]).all()                    # nothing past the N segmentation units is written
    # d_x0 + d_extra, seg = NULL: the other outputs keep their bits
    b = _run_kernel(c, seg=False, extra=True)
    err = CC.rel_err(b["d_pre"].cpu().double().numpy(), ref["d_pre"])
    print(f"d_pre: error {err:.3e} tolerance {tol['d_pre']:.3e}")
    assert err <= tol["d_pre"], (row[:5], "d_pre", err, tol["d_pre"])
    assert torch.equal(b["d_seg"], a["d_seg"]) and torch.equal(b["ws"][:4 * N].view(N, 4)[:, :3], a["ws"][:4 * N].view(N, 4)[:, :3])
    # strided x / d_x0, and the same call twice: the same bits
    s = _run_kernel(c, strided=True)
    a2 = _run_kernel(c)
    for k in ("seg", "d_seg", "d_pre"):
        assert torch.equal(s[k], a[k]) and torch.equal(a2[k], a[k]), (row[:5], k)
    assert torch.equal(a2["ws"][:4 * N].view(N, 4)[:, :3], a["ws"][:4 * N].view(N, 4)[:, :3])


def _raw_call(H, K, N=4, misalign=None, ld_x=None):
    from r3d_amd import _lib
    lib = _lib.load()
    f = lambda *s: torch.full(s, 3.0, dtype=torch.float32, device=DEV)       # noqa: E731
    Hh, Kk = max(H, 4), max(K, 1)
    x, w, b, d_seg, d_pre, ws = f(N, Hh + 4), f(Kk, Hh), f(Kk), f(N, Kk), f(N, Hh), f(4 * N + 4)
    lab = torch.zeros(N, dtype=torch.int64, device=DEV)
    a = _lib.CnnSegArgs()
    a.x, a.ld_x, a.w, a.b, a.labels = x.data_ptr() + (4 if misalign == "x" else 0), ld_x or Hh + 4, w.data_ptr(), b.data_ptr(), lab.data_ptr()
    a.N, a.H, a.Kseg, a.pad_idx, a.exclude_idx, a.grad_scale = N, H, K, Kk + 2, 120, 1.0
    a.d_seg, a.ld_dseg, a.d_pre, a.ld_dpre = d_seg.data_ptr(), Kk, d_pre.data_ptr() + (4 if misalign == "d_pre" else 0), Hh
    rc = lib.r3d_cnn_seg_step(C.byref(a), C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for t in (d_seg, d_pre, ws):
        assert bool((t == 3.0).all())                 # the output buffers are untouched
    return rc


@pytest.mark.parametrize("H,K", CC.REFUSED_SHAPES)
def test_seg_step_refuses_shapes_before_any_launch(H, K):
    from r3d_amd import ops
    assert not ops.cnn_seg_supported(H, K)
    assert _raw_call(H, K) == -1                        # R3D_EINVAL
    if H >= 1 and K >= 1:
        z = torch.zeros(4, H, device=DEV)
        with pytest.raises(ValueError, match="segmentation-head step"):
            ops.cnn_seg_step(z, torch.zeros(K, H, device=DEV), torch.zeros(K, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV),
                             K + 2, 120, torch.zeros(4, K, device=DEV), z.clone(), torch.zeros(32, device=DEV))


@pytest.mark.parametrize("what", ["x", "d_pre", "ld_x"])
def test_seg_step_refuses_misalignment_before_any_launch(what):
    assert _raw_call(16, 5, misalign=what, ld_x=18 if what == "ld_x" else None) == -2      # R3D_EALIGN


# ---------------------------------------------------------------------------------------------------------------------
# the whole step against the reference's fixtures, both routes
# ---------------------------------------------------------------------------------------------------------------------
def _step(fx, chain, batch=None):
    model = _model(fx)
    eng = model.engine()
    eng.use_seg_chain = chain
    feats, lab, dur, tgt = _dev(batch or _batch(fx))
    dead = json.loads(str(fx["dead_names"])) if "dead_names" in fx else []
    before = {n: eng.arena.p(n).clone() for n in dead}
    out = eng.forward(feats, None, lab, "train", training=True)
    assert eng.last["deferred"] == bool(chain)
    loss, counts = eng.losses(lab, tgt, dur, tick=True)
    eng.backward()
    grads = {n: eng.arena.g(n).detach().cpu().clone() for n in eng.arena.live_names}
    eng.adamw(1e-3, 5e-3, ticked=True)
    torch.cuda.synchronize()
    res = {k: v.detach().cpu().clone() for k, v in out.items()}
    return dict(eng=eng, out=res, loss=loss.cpu().clone(), counts=counts.cpu().clone(), grads=grads, before=before,
                post={n: eng.arena.p(n).detach().cpu().clone() for n in eng.arena.live_names}, step=int(eng.step_t))


@pytest.mark.parametrize("chain", ROUTES)
@pytest.mark.parametrize("tag", TAGS)
def test_step_matches_reference(tag, chain):
    fx = load_fixture(tag)
    r = _step(fx, chain)
    eng, res = r["eng"], r["out"]
    assert r["step"] == 1
    sc = lambda a: 1e-3 * max(1.0, float(np.abs(a).max()))      # noqa: E731
    for k in ("action", "duration", "seg"):
        assert_close(res[k], fx["out_" + k], rtol=1e-3, atol=sc(fx["out_" + k]), what=k)
    assert_close(torch.tensor(stats(res["supcon"])[:3]), fx["supcon_stats"][:3], rtol=1e-3, atol=1e-3, what="supcon")
    assert_close(r["loss"], fx["losses"], rtol=1e-3, atol=1e-4, what="losses")
    assert r["counts"].tolist() == fx["counts"].tolist()
    assert sorted(eng.arena.live_names) == sorted(fx["live_names"])
    for j, n in enumerate(fx["live_names"]):
        gs, want = stats(r["grads"][n]), fx["grad_stats"][j]
        assert abs(gs[0] - want[0]) <= 2e-3 * max(1e-3, float(want[0])), (n, gs[0], want[0])
        if "grad::" + n in fx:
            full = fx["grad::" + n]
            assert_close(r["grads"][n], full, rtol=2e-3, atol=2e-3 * max(1e-3, float(np.abs(full).max())), what=n)
    for j, n in enumerate(fx["live_names"]):
        if n == "fc_len.bias":              # (its gradient is zero up to rounding: AdamW moves it either way)
            continue
        ps, want = stats(r["post"][n]), fx["post_stats"][j]
        assert abs(ps[0] - want[0]) <= 2e-3 * max(1.0, float(want[0])), (n, ps[0], want[0])
    for n, b in r["before"].items():
        assert torch.equal(eng.arena.p(n), b), n


@pytest.mark.parametrize("tag", TAGS)
def test_routes_agree(tag):
    """chain against composed: two float32 evaluations of the same formulas, so each quantity may differ by the kernel
    tolerance of the cases at the fixture's own width (cnn_cases.width_tolerance); equal counters.  'supcon' = x comes from
    the same launch on both routes: equal bits.  seg and the heads' outputs are dot products of that width plus a bias: the
    logit tolerance.  A weight gradient sums B*S products of the two routes' d_seg / d_pre / d_actdur rows, whose own
    difference is within the d_seg / d_pre / logit tolerance; the sum's cancellation is allowed a factor of 8."""
    fx = load_fixture(tag)
    a, b = _step(fx, False), _step(fx, True)
    assert a["counts"].tolist() == b["counts"].tolist()
    tol = CC.width_tolerance(fx["meta"]["H"])
    assert torch.equal(a["out"]["supcon"], b["out"]["supcon"])
    for k in ("action", "duration", "seg"):
        err = CC.rel_err(b["out"][k].numpy(), a["out"][k].double().numpy())
        print(f"{k}: difference {err:.3e} tolerance {tol['logits']:.3e}")
        assert err <= tol["logits"], k
    err = CC.rel_err(b["loss"].numpy(), a["loss"].double().numpy())
    print(f"loss: difference {err:.3e} tolerance {tol['loss']:.3e}")
    assert err <= tol["loss"]
    which = {"fc_seg.": "d_seg", "input_embed.": "d_pre", "fc.": "logits", "fc_len.": "logits"}
    for n in a["grads"]:
        if n == "fc_len.bias":              # (zero up to rounding on both routes)
            continue
        q = next(v for k, v in which.items() if n.startswith(k))
        err = CC.rel_err(b["grads"][n].numpy(), a["grads"][n].double().numpy())
        print(f"{n}: difference {err:.3e} tolerance {8 * tol[q]:.3e}")
        assert err <= 8 * tol[q], n


@pytest.mark.parametrize("chain", ROUTES)
def test_two_runs_bit_identical(chain):
    fx = load_fixture("cnn_cfg")
    a, b = _step(fx, chain), _step(fx, chain)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["counts"], b["counts"])
    assert torch.equal(a["eng"].arena.params, b["eng"].arena.params) and torch.equal(a["eng"].arena.grads, b["eng"].arena.grads)


@pytest.mark.parametrize("chain", ROUTES)
def test_graphed_replay_bit_identical_to_eager(chain):
    from r3d_amd.train_unimodal import _UnimodalSteps
    fx = load_fixture("cnn_cfg")
    feats, lab, dur, tgt = _dev(_batch(fx))
    hyper = (5e-3, (0.9, 0.999), 1e-8)
    runs = []
    for graphed in (False, True):
        eng = _model(fx).engine()
        eng.use_seg_chain = chain
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
            assert next(iter(gs.shapes.values()))["graph"] is not None      # steps 2 and 3 ran as a captured graph
        runs.append((eng.arena.params.clone(), eng.arena.exp_avg.clone(), acc_l.clone(), acc_c.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert float(runs[0][2][0]) > 0 and int(runs[0][3][1]) > 0          # the seg loss and its counter reached the sums


@pytest.mark.parametrize("chain", ROUTES)
def test_validation_and_test_mode_forwards(chain):
    fx = load_fixture("cnn_tiny")
    model = _model(fx).eval()
    model.engine().use_seg_chain = chain
    batch = _batch(fx)
    feats = batch[0]
    sc = lambda a: 1e-3 * max(1.0, float(np.abs(a).max()))      # noqa: E731
    with torch.no_grad():
        for b in range(feats.shape[0]):                          # B = 1, the bare tensor, as predict_nturgbd calls it
            out = model(feats[b:b + 1].to(DEV), mode="test")
            for k in ("action", "duration", "seg"):
                want = fx["test_" + k][b:b + 1]
                assert_close(out[k].cpu(), want, rtol=1e-3, atol=sc(want), what=k)
    # validate()'s calls: the train-mode forward without gradients, the losses in validation mode
    eng = model.engine()
    f, lab, dur, tgt = _dev(batch)
    out = eng.forward(f, None, lab, "train", training=False, need_grad=False)
    loss, counts = eng.losses(lab, tgt, dur, with_grad=False, val_mode=True)
    torch.cuda.synchronize()
    p = {n: t.double() for n, t in fixture_params(fx).items()}
    ro = CO.forward(p, batch[0].double())
    for k in ("action", "duration", "seg"):
        assert_close(out[k].cpu(), ro[k], rtol=1e-3, atol=sc(ro[k].numpy()), what=k)
    res = CO.losses(ro, batch[2], batch[3].double(), batch[4], fx["meta"]["pad_idx"])
    assert abs(float(loss[1]) - float(res["loss_action"])) <= 1e-3 * max(1.0, float(res["loss_action"]))
    assert counts.cpu().tolist()[2:] == [res["act_correct"], res["act_total"]]


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
    fx = load_fixture("cnn_train_loop")
    m = fx["meta"]
    model = _model(fx)
    batches = [_batch(fx, seed=m["seed"] + i, exclusion=True) for i in range(m["n_steps"])]
    batches.insert(1, _batch(fx, seed=m["seed"] + 50, B=3, exclusion=False))
    val = [_batch(fx, seed=m["seed"] + 100, B=1, S=m["val_S"], exclusion=False, pad_tail=False)]
    val[0][4] = torch.from_numpy(fx["val_target"])               # (the future labels the fixture's generator chose)
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
    assert sorted(os.listdir(tmp_path)) == fx["ckpt_files"] and fx["ckpt_files"]
    keys = list(torch.load(os.path.join(tmp_path, fx["ckpt_files"][0]), weights_only=True).keys())
    assert keys == fx["ckpt_keys"]
    with contextlib.redirect_stdout(io.StringIO()):
        vres = TU.validate(model, val, torch.nn.MSELoss(reduction="none"), m["pad_idx"], torch.device(DEV))
    assert_close(torch.tensor(vres, dtype=torch.float64), fx["val_result"], rtol=2e-3, atol=1e-4, what="validate")
    eng = model.engine()
    for j, n in enumerate(fx["live_names"]):
        if n == "fc_len.bias":
            continue
        ps, want = stats(eng.arena.p(n)), fx["post_stats"][-1][j]
        assert abs(ps[0] - want[0]) <= 2e-3 * max(1.0, float(want[0])), (n, ps[0], want[0])


# ---------------------------------------------------------------------------------------------------------------------
# --supcon_weight, autograd bridge, predict path, refusals
# ---------------------------------------------------------------------------------------------------------------------
W = 0.5


def close_rel(got, ref, what, rtol):
    err = CC.rel_err(got.detach().cpu().double().numpy(), ref.detach().double().numpy())
    assert err <= rtol, (what, err)


@pytest.mark.parametrize("chain", ROUTES)
@pytest.mark.parametrize("tag", ["cnn_cfg", "cnn_odd"])
def test_step_with_supcon_matches_float64(tag, chain):
    """tolerances of tests/test_supcon_gpu.py's engine test: 1e-3 of the reference's scale"""
    fx = load_fixture(tag)
    pad = fx["meta"]["pad_idx"]
    batch = _batch(fx)

    def term(out, b):
        H = out["supcon"].shape[-1]
        return W * SO.supcon(out["supcon"].reshape(-1, H), b[2].reshape(-1), temperature=0.07, base_temperature=0.07,
                             ignore_index=pad, normalize=True)[0]
    tr = CO.Trainer(fixture_params(fx), pad, extra=term)
    res, _, _ = tr.step(batch, apply=False)
    eng = _model(fx).engine()
    eng.use_seg_chain = chain
    eng.supcon_weight, eng.supcon_temperature = W, 0.07
    feats, lab, dur, tgt = _dev(batch)
    eng.forward(feats, None, lab, "train", training=True)
    loss, _ = eng.losses(lab, tgt, dur, tick=True)
    eng.backward()
    grads = {n: eng.arena.g(n).detach().cpu().clone() for n in eng.arena.live_names}
    eng.adamw(1e-3, 5e-3, ticked=True)
    torch.cuda.synchronize()
    want = [float(res["loss_seg"]), float(res["loss_action"]), float(res["loss_dur"]), float(res["loss"] + res["extra"])]
    for g, r in zip(loss.cpu().double().tolist(), want):
        assert abs(g - r) <= 1e-3 * max(abs(r), 1e-5), (loss.tolist(), want)
    assert abs(W * float(eng.last["w"].sc_loss) - float(res["extra"])) <= 1e-3 * abs(float(res["extra"]))
    for n, g in grads.items():
        if n == "fc_len.bias":              # (zero up to rounding in the oracle: the duration normalisation is shift-invariant)
            continue
        close_rel(g, tr.p[n].grad, n, 1e-3)


def test_supcon_weight_zero_launches_nothing_of_it_and_wide_models_are_refused():
    fx = load_fixture("cnn_cfg")
    eng = _model(fx).engine()
    feats, lab, dur, tgt = _dev(_batch(fx))
    for chain in (True, False):
        eng.use_seg_chain = chain
        eng.train_step(feats, None, lab, dur, tgt, 1e-3, 5e-3)
        torch.cuda.synchronize()
        w = eng.last["w"]
        assert w.sc_ws is None and w.sc_loss is None and w.d_extra is None        # (not even allocated)
        assert (w.d_x is None) == chain                                            # d_x: the composed route's only
    from r3d_amd.model.cnn import FUTR
    wide = FUTR(17, 264, 18, torch.device(DEV), _args(264), n_query=8, n_head=8, num_encoder_layers=1, num_decoder_layers=1).to(DEV)
    e2 = wide.engine()
    e2.supcon_weight = W
    b = [torch.from_numpy(x) for x in synth.make_batch(2, 5, 17, 18, 3, depth_hw=(2, 2))]
    f2, l2, d2, t2 = _dev(b)
    e2.forward(f2, None, l2, "train", training=True)
    with pytest.raises(ValueError, match="256"):
        e2.losses(l2, t2, d2, tick=True)


def test_autograd_bridge_gradients():
    fx = load_fixture("cnn_tiny")
    model = _model(fx).train()
    feats, lab = _batch(fx)[0], _batch(fx)[2]
    g = torch.Generator().manual_seed(7)
    out = model((feats.to(DEV), lab.to(DEV)))
    coef = {k: torch.randn(out[k].shape, generator=g, dtype=torch.float64) for k in ("action", "duration", "seg", "supcon")}
    loss = sum((out[k].double() * coef[k].to(DEV)).sum() for k in coef)
    loss.backward()
    p = {n: t.double().requires_grad_(CO.is_live(n)) for n, t in fixture_params(fx).items()}
    ro = CO.forward(p, feats.double())
    sum((ro[k] * coef[k]).sum() for k in coef).backward()
    for n, q in model.named_parameters():
        if not CO.is_live(n):
            assert q.grad is None, n
            continue
        want = p[n].grad
        assert_close(q.grad.cpu(), want, rtol=2e-3, atol=2e-3 * max(1e-3, float(want.abs().max())), what=n)


def test_predict_nturgbd_on_synthetic_videos():
    from r3d_amd.predict import predict_nturgbd
    fx = load_fixture("cnn_tiny")
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
        ro = CO.forward(p, torch.from_numpy(np.ascontiguousarray(feats[:int(0.5 * T)])).double().unsqueeze(0))
        ok_seg = (ro["seg"][0].argmax(-1) == d["seg_labels"]).double().mean()
        ok_act = (ro["action"][0].argmax(-1) == d["action_labels"]).double().mean()
        assert ok_seg >= 0.9 and ok_act >= 0.875, (d["video"], float(ok_seg), float(ok_act))


@pytest.mark.parametrize("H,n_query,n_class", [(1032, 8, 17), (12, 8, 17), (128, 9, 17), (128, 8, 1024)])
def test_engine_refuses_before_any_launch(H, n_query, n_class):
    from r3d_amd.model.cnn import FUTR
    model = FUTR(n_class, H, n_class + 1, torch.device(DEV), _args(H), n_query=n_query, n_head=4, num_encoder_layers=1,
                 num_decoder_layers=1).to(DEV)
    with pytest.raises(ValueError):
        model.engine()
    assert model._engine is None


def test_rank_penalty_and_rank_report_are_refused(tmp_path):
    from r3d_amd import train_unimodal as TU
    from r3d_amd.rankstream import measure_rank
    fx = load_fixture("cnn_tiny")
    model = _model(fx)
    with pytest.raises(ValueError, match="erank_weight"):
        TU.train(_args(16, erank_weight=0.1), model, [], torch.optim.AdamW(model.parameters()), None, None, str(tmp_path),
                 fx["meta"]["pad_idx"], torch.device(DEV), [], 1)
    assert model._engine is None
    with pytest.raises(ValueError, match="fused token matrix"):
        measure_rank(model, [], torch.device(DEV))
    with pytest.raises(ValueError, match="erank_weight"):
        model.engine().erank_weight = 0.1
