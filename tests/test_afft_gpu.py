"""The AFFT baseline (model/afft.py) on the device: the pooled-head chain's two kernels through r3d_amd.ops against the
float64 restatement (tests/afft_oracle.tail) over tests/afft_cases.KERNEL_CASES, their bit reproducibility and add / gscale
form; the model through the fixtures from the imported reference (train step, AdamW, dead parameters, validation forward in
both input forms, mode 'test'); a step with dropout on (the engine's own mask handed to the restatement); the chain
against the composed tail; graphed against eager steps; train() / validate() with its checkpoint writes; the autograd bridge; measure_rank; every refusal before a launch.

Bounds: what the model shares with the plain SA-Fuser uses tests/test_plain_fuser_gpu.py's bounds unchanged (outputs and
fused 1e-3, losses rtol 1e-3, gradients 2e-3, AdamW step 2e-2, all relative to the tensor's scale); the new kernels use
afft_cases.KERNEL_RTOL, derived there from the float32-CPU error of the same formulas."""
import argparse
import contextlib
import io
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import synth  # noqa: E402
from tests import afft_cases as AC  # noqa: E402
from tests import afft_oracle as AO  # noqa: E402
from tests import rank_cases as RC  # noqa: E402
from tests import rank_oracle as RO  # noqa: E402
from tests.helpers import fixture_params, load_fixture  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

TAGS = ["afft_tiny", "afft_cfg2", "afft_odd"]
EXCLUDE = 47


def _args(seg=False):
    return argparse.Namespace(input_dim=2048, seg=seg, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")


def _model(params, H, K, pad_idx, hw=(224, 224), seg=False, n_enc=2):
    from r3d_amd.model.afft import FUTR
    model = FUTR(K, H, pad_idx, torch.device("cuda"), _args(seg), n_query=8, n_head=8, num_encoder_layers=n_enc,
                 num_decoder_layers=1, depth_pixels=hw[0] * hw[1])
    missing = model.load_state_dict(params, strict=False)
    assert not missing.unexpected_keys and all("pos_table" in k for k in missing.missing_keys), missing
    return model.to("cuda")


def _params(H, K, hw, n_enc=2):
    from r3d_amd.model.afft import FUTR
    m = FUTR(K, H, K + 1, torch.device("cpu"), _args(), n_query=8, n_head=8, num_encoder_layers=n_enc, num_decoder_layers=1,
             depth_pixels=hw[0] * hw[1])
    ns = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    return {n: torch.from_numpy(synth.fill_value(n, s, j)) for j, (n, s) in enumerate(ns)}


def _batch(B, S, K, seed, hw=(224, 224)):
    return [torch.from_numpy(x) for x in synth.make_batch(B, S, K, K + 1, seed, depth_hw=hw)]


def _step(eng, d, training=False):
    out = eng.forward(d[0], d[1], d[2], "train", training=training)
    out = {k: v.clone() for k, v in out.items()}
    loss, counts = eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()
    return out, loss.clone(), counts.clone()


# ---- the two kernels through ops -------------------------------------------------------------------------------------------
_REF = {}


def _ref(c):
    """The float64 restatement of a kernel case: computed once, shared, never modified."""
    key = AC.kernel_id(c)
    if key not in _REF:
        x = AC.kernel_inputs(c)
        _REF[key] = (x, AO.tail(x["fused"].double(), x["w_head"].double(), x["b_head"].double(), c.Q, x["lab"], x["dur"],
                                x["tgt_oracle"], x["pad"]))
    return _REF[key]


def _run_step(ops, c, x, d_fused=None, **kw):
    dev = "cuda"
    N, BQ = c.B * c.S, c.B * c.Q
    fused = x["fused"].reshape(N, c.H).to(dev)
    w_head, b_head = x["w_head"].to(dev), x["b_head"].to(dev)
    pooled = torch.full((BQ, c.H), float("nan"), device=dev)
    out = torch.full((BQ, c.K1), float("nan"), device=dev)
    d_out = torch.full((BQ, c.K1), float("nan"), device=dev)
    if d_fused is None:
        d_fused = torch.full((N, c.H), float("nan"), device=dev)
    ws = torch.zeros(ops.losses_ws_floats(c.B, c.S, c.Q), device=dev)
    ws[:4 * (N + BQ + c.B)] = 7.0             # what an earlier user of the scratch may have left in the units: all rewritten
    loss, counts = torch.zeros(4, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    ops.afft_head_step(fused, w_head, b_head, pooled, out, c.B, c.S, c.Q, x["lab"].to(dev), x["tgt"].to(dev), x["dur"].to(dev),
                       x["pad"], EXCLUDE, d_out, d_fused, ws, **kw)
    part = ws.clone()
    ops.losses_finalize(ops.loss_finalize_job(ws, c.B, c.S, c.Q, False, None, loss, counts))
    torch.cuda.synchronize()
    return dict(pooled=pooled, actdur=out, d_actdur=d_out, d_fused=d_fused, losses=loss, counts=counts, part=part)


@pytest.mark.parametrize("c", AC.KERNEL_CASES, ids=AC.kernel_id)
def test_head_kernels_against_fp64(c):
    from r3d_amd import ops
    x, r = _ref(c)
    N, BQ = c.B * c.S, c.B * c.Q
    got = _run_step(ops, c, x)
    tol = AC.KERNEL_RTOL
    for k, shape in (("pooled", (BQ, c.H)), ("actdur", (BQ, c.K1)), ("d_actdur", (BQ, c.K1)), ("d_fused", (N, c.H))):
        err = float((got[k].double().cpu() - r[k].reshape(shape)).abs().max()) / max(float(r[k].abs().max()), 1e-5)
        print(f"[afft kernel {AC.kernel_id(c)}] {k} rel err {err:.2e} (bound {tol[k]:.2e})")
    for k, shape in (("pooled", (BQ, c.H)), ("actdur", (BQ, c.K1)), ("d_actdur", (BQ, c.K1)), ("d_fused", (N, c.H))):
        assert torch.isfinite(got[k]).all(), k
        close_rel(got[k], r[k].reshape(shape), f"{AC.kernel_id(c)} {k}", rtol=tol[k])
    close_rel(got["losses"], r["losses"], f"{AC.kernel_id(c)} losses", rtol=tol["losses"])
    assert got["counts"].cpu().tolist() == r["counts"].tolist()
    # the loss partials: the segmentation units untouched, one anticipation unit per row, one duration unit per clip
    part = got["part"][:4 * (N + BQ + c.B)].view(-1, 4).cpu().double()
    assert not part[:N].any()
    assert abs(float(part[N:N + BQ, 0].sum()) / BQ - r["losses"][1]) <= tol["losses"] * max(r["losses"][1], 1e-5)
    assert int(part[N:N + BQ, 2].sum()) == int(r["counts"][3]) and int(part[N:N + BQ, 1].sum()) == int(r["counts"][2])
    assert float(got["part"][4 * (N + BQ + c.B):].abs().sum()) == 0.0          # the arrival word stays zero
    # the forward kernel: the same pooled rows and logits, bit for bit
    pooled = torch.full((BQ, c.H), float("nan"), device="cuda")
    out = torch.full((BQ, c.K1), float("nan"), device="cuda")
    ops.afft_head_fwd(x["fused"].reshape(N, c.H).cuda(), x["w_head"].cuda(), x["b_head"].cuda(), pooled, out, c.B, c.S, c.Q)
    torch.cuda.synchronize()
    assert torch.equal(pooled, got["pooled"]) and torch.equal(out, got["actdur"])


@pytest.mark.parametrize("c", [AC.KERNEL_CASES[i] for i in (3, 4, 6)], ids=AC.kernel_id)
def test_head_step_is_bit_reproducible_and_takes_add_and_gscale(c):
    from r3d_amd import ops
    x, r = _ref(c)
    a = _run_step(ops, c, x)
    b = _run_step(ops, c, x)
    for k in ("pooled", "actdur", "d_actdur", "d_fused", "losses", "counts", "part"):
        assert torch.equal(a[k], b[k]), k
    base = torch.randn(c.B * c.S, c.H, device="cuda")
    s = _run_step(ops, c, x, d_fused=base.clone(), add=True, gscale=0.5)
    close_rel(s["d_fused"], base.double().cpu() + 0.5 * r["d_fused"].reshape(-1, c.H), "add / gscale",
              rtol=AC.KERNEL_RTOL["d_fused"])
    assert torch.equal(s["d_actdur"], a["d_actdur"])
    g = _run_step(ops, c, x, grad_scale=4.0)                                  # grad_scale: as the loss launch, into d_actdur
    close_rel(g["d_actdur"], 4.0 * r["d_actdur"].reshape(-1, c.K1), "grad_scale d_actdur", rtol=AC.KERNEL_RTOL["d_actdur"])
    close_rel(g["d_fused"], 4.0 * r["d_fused"].reshape(-1, c.H), "grad_scale d_fused", rtol=AC.KERNEL_RTOL["d_fused"])
    assert torch.equal(g["losses"], a["losses"])
    # the step counter and the dropout offset tick once per call
    ta, tb = torch.tensor([5], device="cuda"), torch.tensor([9], device="cuda")
    _run_step(ops, c, x, tick_a=ta, tick_b=tb)
    assert ta.item() == 6 and tb.item() == 10


def test_ops_refuse_before_launching(monkeypatch):
    from r3d_amd import ops
    calls = []
    real = ops.check
    monkeypatch.setattr(ops, "check", lambda *a, **k: (calls.append(a), real(*a, **k))[1])
    f = lambda *s: torch.zeros(*s, device="cuda")       # noqa: E731
    with pytest.raises(ValueError, match="LDS"):
        ops.afft_head_fwd(f(32, 1024), f(123, 1024), f(123), f(2 * 64, 1024), f(2 * 64, 123), 2, 16, 64)
    with pytest.raises(ValueError, match="n_query <= 64"):
        ops.afft_head_fwd(f(32, 64), f(18, 64), f(18), f(2 * 65, 64), f(2 * 65, 18), 2, 16, 65)
    with pytest.raises(AssertionError):
        ops.afft_head_fwd(f(31, 64), f(18, 64), f(18), f(16, 64), f(16, 18), 2, 16, 8)
    assert not calls


# ---- the model through the fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [True, False], ids=["chain", "composed"])
@pytest.mark.parametrize("tag", TAGS)
def test_afft_step_parity_and_adamw(tag, chain, oracle_lib):
    fx = load_fixture(tag)
    m = fx["meta"]
    H, K = m["H"], m["n_class"]
    batch = _batch(m["B"], m["S"], K, m["seed"])
    p = fixture_params(fx)
    t64 = AO.Trainer(p, m["pad_idx"], 8, 8, lr=m["lr"], wd=m["wd"], dtype=torch.float64)
    res64, out64, aux64 = t64.step(batch, apply=False)
    g64 = {n: q.grad.clone() for n, q in t64.p.items() if q.grad is not None}
    model = _model(p, H, K, m["pad_idx"], n_enc=m["n_encoder_layer"]).eval()
    assert list(model.state_dict().keys()) == json.loads(str(fx["state_keys"]))
    eng = model.engine()
    assert sorted(eng.arena.live_names) == sorted(fx["live_names"])
    eng.use_head_chain = chain                 # the one-launch tail, and the composed launches the engine routes to by default
    assert eng._chain(eng._shape(m["B"], m["S"], True)) == chain
    before = eng.arena.params.clone()
    d = [t.cuda() for t in batch]
    out, loss, counts = _step(eng, d)
    w = eng.last["w"]
    assert sorted(out) == ["action", "duration"]
    for k in ("action", "duration"):
        close_rel(out[k], fx["out_" + k], f"{tag}/{k} vs reference fixture", rtol=1e-3)
        close_rel(out[k], out64[k].detach(), f"{tag}/{k} vs fp64", rtol=1e-3)
    close_rel(w.fused.view(m["B"], m["S"], H), fx["fused"], f"{tag}/fused", rtol=1e-3)
    np.testing.assert_allclose(loss.cpu().numpy(), fx["losses"], rtol=1e-3, atol=1e-6)
    assert counts.cpu().tolist() == fx["counts"].tolist()
    for n in fx["live_names"]:
        if n == "fc_len.bias":                     # exactly zero in exact arithmetic (the duration is L1-normalised)
            continue
        close_rel(eng.arena.g(n), g64[n], f"{tag}/grad {n}", rtol=2e-3)
    for n in ("fuser.modality_token", "fuser.norm.weight", "depth_layernorm.weight", "input_embed.bias", "fc.bias", "fc_len.weight"):
        close_rel(eng.arena.g(n), fx["grad::" + n], f"{tag}/grad {n} vs reference", rtol=2e-3)
    qk = eng.arena.g("fuser.blocks.0.attn.qkv.weight")[:2 * H]
    assert not qk.any()                                     # the Q and K rows: live, with an exactly zero gradient
    grads = eng.arena.grads.clone()
    _step(eng, d)                                           # the same step again: every gradient bit for bit
    assert torch.equal(eng.arena.grads, grads)
    assert torch.equal(eng.arena.params, before)
    # ---- one fused AdamW step: live parameters against the restatement, the Q / K rows decayed, dead parameters untouched
    eng.adamw(m["lr"], m["wd"])
    torch.cuda.synchronize()
    t64.step(batch, apply=True)
    for n in fx["live_names"]:
        g = g64[n]
        keep = (g.abs() > 1e-3 * float(g.abs().max())) if float(g.abs().max()) > 0 else torch.zeros_like(g, dtype=torch.bool)
        if n == "fc_len.bias" or not keep.any():
            continue
        o, k, shp = eng.arena.offsets[n]
        delta = (eng.arena.p(n) - before[o:o + k].view(shp)).double().cpu()
        close_rel(delta[keep], (t64.p[n].detach() - p[n].double())[keep], f"{tag}/AdamW step {n}", rtol=2e-2)
    o, k, shp = eng.arena.offsets["fuser.blocks.0.attn.qkv.weight"]
    qk0 = before[o:o + 2 * H * H]
    close_rel(eng.arena.params[o:o + 2 * H * H], qk0.double() * (1.0 - m["lr"] * m["wd"]), "Q / K rows: decay only", rtol=2e-7)
    assert not torch.equal(eng.arena.params[o:o + 2 * H * H], qk0)
    assert torch.equal(eng.arena.params[eng.arena.n_live:], before[eng.arena.n_live:])         # dead: bit-unchanged
    for n in ("fc_l3.weight", "pos_embedding", "fuser.projection.weight", "query_embed.weight"):
        assert not eng.arena.is_live(n) and torch.equal(eng.arena.p(n).cpu(), p[n]), n


def test_afft_val_forward_bare_tensor_tuple_and_test_mode(oracle_lib):
    fx = load_fixture("afft_cfg2")
    m = fx["meta"]
    batch = _batch(m["B"], m["S"], m["n_class"], m["seed"])
    model = _model(fixture_params(fx), m["H"], m["n_class"], m["pad_idx"], n_enc=m["n_encoder_layer"]).eval()
    d = [t.cuda() for t in batch]
    with torch.no_grad():
        bare = model(d[0], d[1], mode="val")
        tup = model((d[0], d[2]), d[1], mode="val")
    torch.cuda.synchronize()
    assert sorted(bare) == ["action", "duration"]
    for k in ("action", "duration"):
        close_rel(bare[k], fx["val_" + k], f"val {k} (bare tensor)", rtol=1e-3)
        assert torch.equal(bare[k], tup[k]), k
    close_rel(model.engine().last["w"].fused.view(m["B"], m["S"], m["H"]), fx["val_fused"], "val fused", rtol=1e-3)
    # validate()'s loss launch on these outputs: the unmasked duration target
    eng = model.engine()
    eng.forward(d[0], d[1], d[2], "val", training=False, need_grad=False)
    loss, counts = eng.losses(d[2], d[4], d[3], with_grad=False, val_mode=True)
    ref = AO.losses({"action": torch.from_numpy(fx["val_action"]).double(), "duration": torch.from_numpy(fx["val_duration"]).double()},
                    batch[2], batch[3].double(), batch[4], m["pad_idx"], val_mode=True)
    np.testing.assert_allclose(loss.cpu().numpy()[1:3], [float(ref["loss_action"]), float(ref["loss_dur"])], rtol=1e-3)
    assert counts.cpu().tolist()[2:] == [ref["act_correct"], ref["act_total"]]
    with torch.no_grad():                                  # the per-video call of predict.py's loop (which then reads 'seg')
        one = model(d[0][1:2], d[1][1:2], "test")
    for k in ("action", "duration"):
        close_rel(one[k][0], fx["val_" + k][1], f"mode 'test', one clip: {k}", rtol=1e-3)


@pytest.mark.parametrize("B,S,H,K,hw", AC.STEP_CASES, ids=lambda v: str(v))
def test_afft_step_shapes_dropout_and_chain_vs_composed(B, S, H, K, hw, oracle_lib):
    """Dropout on: the engine's own keep mask read back and handed to the float64 restatement; then the same step with the
    composed tail (the launches that existed before the chain) against the chain's."""
    batch = _batch(B, S, K, 300 + B + S, hw)
    p = _params(H, K, hw)
    model = _model(p, H, K, K + 1, hw).train()
    eng = model.engine()
    d = [t.cuda() for t in batch]
    snaps = {}
    for chain in (True, False):
        eng.use_head_chain = chain
        eng.drop_offset.zero_()
        out, loss, counts = _step(eng, d, training=True)
        w = eng.last["w"]
        snaps[chain] = dict(out=out, loss=loss, counts=counts, grads=eng.arena.grads.clone(), pooled=w.pooled.clone(),
                            d_fused=w.d_fused.clone(), mask=w.drop["x0"].clone())
    a, b = snaps[True], snaps[False]
    assert torch.equal(a["mask"], b["mask"]) and not a["mask"].all()     # the same masks both times, and some frames dropped
    assert torch.equal(a["pooled"], b["pooled"])                        # the same sequential window sums
    close_rel(a["loss"], b["loss"], "chain vs composed: loss", rtol=1e-5)
    close_rel(a["d_fused"], b["d_fused"], "chain vs composed: d_fused", rtol=AC.KERNEL_RTOL["d_fused"] * 2)
    keep = a["mask"].view(2 * B * S, H).cpu().double() / (1.0 - 0.1)
    t64 = AO.Trainer(p, K + 1, 8, 8, dtype=torch.float64)
    res64, out64, aux64 = t64.step(batch, apply=False, x0_hook=lambda x: x * keep.view(x.shape))
    for k in ("action", "duration"):
        close_rel(a["out"][k], out64[k].detach(), f"dropout step {k}", rtol=1e-3)
    np.testing.assert_allclose(a["loss"].cpu().numpy()[1:], [float(res64[k]) for k in ("loss_action", "loss_dur", "loss")], rtol=1e-3)
    assert a["counts"].cpu().tolist() == [0, 0, res64["act_correct"], res64["act_total"]] == b["counts"].cpu().tolist()
    for which, s in (("chain", a), ("composed", b)):
        for n, q in t64.p.items():
            if q.grad is None or n == "fc_len.bias":
                continue
            o, k, shp = eng.arena.offsets[n]
            close_rel(s["grads"][o:o + k].view(shp), q.grad, f"dropout step ({which}) grad {n}", rtol=2e-3)


@pytest.mark.parametrize("chain", [True, None], ids=["chain", "routed"])
def test_afft_graph_replay_equals_eager(chain):
    """Three steps of train()'s graphed step path (_GraphedSteps: eager, capture, replay) against the same three enqueued
    eagerly on a second engine, dropout on: every parameter and the epoch sums bit for bit."""
    from r3d_amd.train_proposed_depth import _GraphedSteps
    K, hw = 17, (12, 16)
    p = _params(128, K, hw)
    batches = [[t.cuda() for t in _batch(8, 16, K, 100 + i, hw)] for i in range(3)]
    engs, accs = [], []
    for graphed in (True, False):
        model = _model(p, 128, K, K + 1, hw).train()
        eng = model.engine()
        eng.defer_tail = True
        eng.use_head_chain = chain
        acc_l = torch.zeros(4, dtype=torch.float64, device="cuda")
        acc_c = torch.zeros(4, dtype=torch.int64, device="cuda")
        gs = _GraphedSteps(eng, acc_l, acc_c, None, K + 1)
        hyper = (5e-3, (0.9, 0.999), 1e-8)
        for b in batches:
            if graphed:
                gs.step(b, 1e-3, hyper, True)
            else:
                eng._drop_ready = None
                gs._enqueue(b, 1e-3, hyper, True)
            torch.cuda.synchronize()
        if graphed:
            assert all(st["graph"] is not None for st in gs.shapes.values())      # steps 2.. replayed a capture
        engs.append(eng)
        accs.append((acc_l.clone(), acc_c.clone()))
    a, b = engs
    assert torch.equal(a.arena.params, b.arena.params)
    assert torch.equal(a.arena.exp_avg_sq, b.arena.exp_avg_sq)
    assert torch.equal(accs[0][0], accs[1][0]) and torch.equal(accs[0][1], accs[1][1])
    assert int(a.step_t) == 3 and int(a.drop_offset) == 3 and float(accs[0][0][3]) > 0 and int(accs[0][1][3]) > 0
    tok0 = p["fuser.modality_token"].cuda()
    assert float((a.arena.p("fuser.modality_token") - tok0).abs().max()) > 1e-4        # the token trained
    assert torch.equal(a.arena.p("fc_l3.weight").cpu(), p["fc_l3.weight"])              # a dead one did not move


def test_afft_train_and_validate_one_epoch(tmp_path):
    from r3d_amd.optim import FlatAdamW
    from r3d_amd.train_proposed_depth import train
    K, hw = 17, (12, 16)
    p = _params(128, K, hw)
    p["fc.bias"][3] = 50.0                    # class 3 wins every row whatever three steps do to the rest ...
    model = _model(p, 128, K, K + 1, hw)
    batches = [_batch(8, 16, K, 400 + i, hw) for i in range(3)]
    val = [[t[:1] for t in _batch(2, 16, K, 999, hw)], [t[:1] for t in _batch(2, 9, K, 998, hw)]]
    for v in val:
        v[4][:] = 3                           # ... and is every validation target: accuracy 1, so the checkpoint is written
    args = argparse.Namespace(epochs=1, input_type="i3d_transcript", seg=False, anticipate=True, task="long", min_batch=1)

    class NoSched:
        def step(self):
            pass
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train(args, model, batches, FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3), NoSched(), None, str(tmp_path),
              K + 1, torch.device("cuda"), val, seed=3)
    torch.cuda.synchronize()
    text = buf.getvalue()
    for piece in ("Training Start", "Epoch [ 1 / 1 ] Loss :", "Training Acc :", "CE loss :", "dur loss:", "Validation Loss:",
                  "Segmentation Accuracy: 0.000"):
        assert piece in text, (piece, text)
    eng = model.engine()
    assert int(eng.step_t) == 3
    assert "Class Accuracy: 1.000" in text and "Best model saved with validation loss:" in text, text
    assert sorted(f.name for f in tmp_path.iterdir()) == ["seed_3_best.ckpt", "seed_3_checkpoint0.ckpt"]
    for name in ("seed_3_best.ckpt", "seed_3_checkpoint0.ckpt"):
        sd = torch.load(tmp_path / name, map_location="cpu")
        assert list(sd.keys()) == list(model.state_dict().keys())
        fresh = _model(_params(128, K, hw), 128, K, K + 1, hw)
        fresh.load_state_dict(sd, strict=True)
        assert torch.equal(sd["fc.weight"], model.state_dict()["fc.weight"].cpu())
        assert not torch.equal(sd["fc.weight"], p["fc.weight"])              # the trained weights, not the initial ones


def test_afft_autograd_bridge(oracle_lib):
    """The reference loop's route: model(...) with grad enabled, a torch loss on its outputs, loss.backward() -- .grad of the
    live parameters equals the engine's own backward of the same output gradients bit for bit and the float64 restatement's
    autograd within the plain model's gradient bound; dead parameters keep grad None."""
    fx = load_fixture("afft_tiny")
    m = fx["meta"]
    H, K, B = m["H"], m["n_class"], m["B"]
    batch = _batch(B, m["S"], K, m["seed"])
    p = fixture_params(fx)
    model = _model(p, H, K, m["pad_idx"], n_enc=m["n_encoder_layer"]).eval()
    d = [t.cuda() for t in batch]
    g = torch.Generator().manual_seed(11)
    ca, cd = torch.randn(B, 8, K, generator=g), torch.randn(B, 8, generator=g)
    out = model((d[0], d[2]), d[1], "train")
    assert sorted(out) == ["action", "duration"] and out["action"].requires_grad
    ((out["action"] * ca.cuda()).sum() + (out["duration"] * cd.cuda()).sum()).backward()
    torch.cuda.synchronize()
    got = {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}
    eng = model.engine()
    assert sorted(got) == sorted(fx["live_names"])
    eng.forward(d[0], d[1], d[2], "train", training=False)
    eng.backward(d_actdur=torch.cat([ca.reshape(-1, K), cd.reshape(-1, 1)], dim=1).cuda())
    torch.cuda.synchronize()
    t64 = AO.Trainer(p, m["pad_idx"], 8, 8, dtype=torch.float64)
    o64, _ = AO.forward(t64.p, (batch[0].double(), batch[2]), batch[1].double(), "train", m["pad_idx"], 8, 8)
    ((o64["action"] * ca.double()).sum() + (o64["duration"] * cd.double()).sum()).backward()
    for n in fx["live_names"]:
        assert torch.equal(got[n], eng.arena.g(n)), n
        close_rel(got[n], t64.p[n].grad, f"autograd bridge grad {n}", rtol=2e-3)
    # only the action gradient handed in: the duration column is zero, not stale
    model.zero_grad(set_to_none=True)
    out = model((d[0], d[2]), d[1], "train")
    (out["action"] * ca.cuda()).sum().backward()
    for q in t64.p.values():
        q.grad = None
    o64, _ = AO.forward(t64.p, (batch[0].double(), batch[2]), batch[1].double(), "train", m["pad_idx"], 8, 8)
    (o64["action"] * ca.double()).sum().backward()
    close_rel(model.fc.weight.grad, t64.p["fc.weight"].grad, "action only: grad fc.weight", rtol=2e-3)
    assert not model.fc_len.weight.grad.any() and not model.fc_len.bias.grad.any()
    close_rel(model.input_embed.bias.grad, t64.p["input_embed.bias"].grad, "action only: grad input_embed.bias", rtol=2e-3)


def test_afft_measure_rank_against_svdvals():
    from r3d_amd.engine_afft import AfftEngine
    from r3d_amd.rankstream import BUFFERS, measure_rank
    K, hw, H = 17, (12, 16), 128
    model = _model(_params(H, K, hw), H, K, K + 1, hw).eval()
    loader = [_batch(4, 16, K, 700, hw), _batch(3, 37, K, 701, hw), _batch(2, 6, K, 702, hw)]
    kept = {name: [] for name in BUFFERS}
    real = AfftEngine.forward

    def forward(self, feats, depth, labels, mode="train", **kw):
        out = real(self, feats, depth, labels, mode, **kw)
        ok = (labels != K + 1).reshape(-1)
        for name, attr in BUFFERS.items():
            kept[name].append(getattr(self.last["w"], attr)[ok].cpu())
        return out
    AfftEngine.forward = forward
    try:
        res = measure_rank(model, loader, torch.device("cuda"))
    finally:
        AfftEngine.forward = real
    assert model.engine().rank_stream is None
    n_valid = sum(int((b[2] != K + 1).sum()) for b in loader)
    for name in ("rgb", "depth", "fused"):
        x = torch.cat(kept[name]).numpy()
        er_ref = RO.erank64(x)
        print(f"[afft rank {name}] erank {res[name]['erank']:.5f} vs {er_ref:.5f} over {n_valid} frames")
        assert res[name]["rows"] == n_valid == x.shape[0]
        assert abs(res[name]["erank"] - er_ref) <= RC.erank_tol(er_ref), (name, res[name]["erank"], er_ref)


def test_afft_refusals_raise_before_any_launch(monkeypatch, tmp_path):
    from r3d_amd import ops
    from r3d_amd.model.afft import FUTR
    from r3d_amd.parallel import DataParallelStep
    calls = []
    real = ops.check
    monkeypatch.setattr(ops, "check", lambda *a, **k: (calls.append(a), real(*a, **k))[1])
    mk = lambda H, heads, Q, K, seg=False: FUTR(K, H, K + 1, torch.device("cuda"), _args(seg), n_query=Q, n_head=heads,     # noqa: E731
                                                num_encoder_layers=1, num_decoder_layers=1, depth_pixels=48).to("cuda")
    for (H, heads, Q, K), word in (((1032, 8, 8, 17), "1024"), ((128, 8, 65, 17), "n_query"), ((1024, 8, 40, 17), "LDS")):
        model = mk(H, heads, Q, K)
        with pytest.raises(ValueError, match=word):
            model.engine()
        assert model._engine is None
    model = mk(64, 8, 8, 17, seg=True)
    with pytest.raises(ValueError, match="no 'seg' output"):
        model.engine()
    model = mk(64, 8, 8, 17)
    eng = model.engine()
    with pytest.raises(ValueError, match="effective-rank penalty"):
        eng.erank_weight = 0.05
    eng.erank_weight = 0.0
    with pytest.raises(ValueError, match="one GPU"):
        DataParallelStep(eng)
    assert eng.grad_hook is None and eng.tp is None
    assert not calls                                       # nothing was enqueued by any of the refusals above
    d = [t.cuda() for t in _batch(2, 6, 17, 1, (6, 8))]
    eng.forward(d[0], d[1], d[2], "train", training=False)
    calls.clear()
    with pytest.raises(AssertionError, match="follows losses"):        # a backward with no losses() before it
        eng.backward()
    assert not calls
