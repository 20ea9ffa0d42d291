"""The query models (r3d_amd/engine_unsup.py) with --long_clips on, at clips past the S x S attention core's limits, against
the oracle run in float64: both decoder attentions of every layer run through the tiled core (csrc/attention_tiled.hip),
never the S x S one; the memory, the queries, the decoder output, the pooled rows and the outputs match within 1e-3 of scale,
the losses ("depth" rows) within 1e-3 and every live gradient within 2e-3 (4e-3 with the FFN's ReLU-kink units excluded) --
the tolerances of tests/test_query_shapes_gpu.py.  Then: the flag off still refuses; the flag on at a short clip launches the
S x S core and gives the flag-off bits; the shape cache keeps route and buffers per shape; a forward alone; train() with
graph replay against the eager loop; dropout on.  Needs an MI355X."""
import argparse
import io
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import futr_oracle as O  # noqa: E402
from tests import query_cases as QC  # noqa: E402
from tests import test_query_shapes_gpu as QS  # noqa: E402
from tests.helpers import assert_close, ffn_kink_units, without_kink_units  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

ARGS_LONG = argparse.Namespace(**vars(QS.ARGS), long_clips=True)


class Recorder(QS.Recorder):
    NAMES = ("mha_core_fwd", "mha_core_bwd", "mha_tiled_fwd", "mha_tiled_bwd", "check")


def build_model(c, p, long_clips=True):
    """tests/test_query_shapes_gpu.build_model with the flag in the args namespace."""
    args = ARGS_LONG if long_clips else QS.ARGS
    if c.variant == "depth":
        from r3d_amd.model.futr_unsupervised_depth import FUTR
        kw = dict(depth_pixels=c.hw[0] * c.hw[1])
    else:
        from r3d_amd.model.futr_proposed import FUTR
        kw = dict(query_num=QC.QUERY_NUM)
    model = FUTR(c.K, c.H, c.K + 1, torch.device("cuda"), args, n_query=QC.Q, n_head=c.heads, num_encoder_layers=2,
                 num_decoder_layers=c.n_dec, **kw)
    assert model.r3d_long_clips is long_clips
    assert not model.load_state_dict(p, strict=False).unexpected_keys
    return model.to("cuda")


CASES = [
    QC._c("depth", 2, 65, 128, 8),
    QC._c("depth", 1, 130, 64, 8, pad="none"),
    QC._c("depth", 3, 41, 200, 8, pad=(1, 20, 41)),
    QC._c("depth", 2, 17, 512, 8),
    QC._c("depth", 1, 9, 1024, 8, pad="none"),
    QC._c("depth", 2, 129, 96, 6, K=122),
    QC._c("depth", 1, 257, 128, 8, n_dec=2, pad="none"),
    QC._c("depth", 2, 300, 128, 8, n_dec=1),
    QC._c("label", 1, 65, 128, 8, pad="none"),
    QC._c("label", 1, 193, 128, 8, n_dec=2, pad="none"),
    QC._c("label", 2, 200, 128, 8, n_dec=1),
]


@pytest.mark.parametrize("c", CASES, ids=QC.case_id)
def test_long_clip_against_fp64_oracle(c, oracle_lib, monkeypatch):
    B, S, H, heads, Q = c.B, c.S, c.H, c.heads, QC.Q
    dh = H // heads
    cid = QC.case_id(c)
    batch = QC.make_batch(c)
    p = QS.params(c)
    res, oout, oaux, ograd = QS.oracle64(c, batch, p)
    model = build_model(c, p).eval()
    eng = model.engine()
    d = [t.cuda() for t in batch]
    rec = Recorder(monkeypatch)
    out, loss, grads = QS.run_step(eng, model, c, d)
    torch.cuda.synchronize()
    monkeypatch.undo()
    # ---- the attention launches: the tiled pair, S queries against S keys, in both attentions of every layer
    names = rec.names()
    assert "mha_core_fwd" not in names and "mha_core_bwd" not in names, cid
    fw = [a for n, a in rec.calls if n == "mha_tiled_fwd"]
    bw = [a for n, a in rec.calls if n == "mha_tiled_bwd"]
    assert len(fw) == 2 * c.n_dec and len(bw) == 2 * c.n_dec, (cid, len(fw), len(bw))
    for a in fw + bw:
        assert (a[-3], a[-2], a[-1]) == (S, S, dh) and a[-4] == heads, (cid, a[-4:])
    w = eng.last["w"]
    assert w.route == "tiled" and all("p_sa" not in lay and "p_ca" not in lay for lay in w.layers), cid
    # ---- activations, outputs, losses
    for got, k, rows in ((w.mem, "memory", S), (w.qpos, "query", S), (w.tgtF, "tgt", S), (w.pooled, "pooled", Q)):
        close_rel(got.view(B, rows, H), oaux[k].detach(), f"{cid}/{k}")
    for k in ("action", "duration", "seg"):
        close_rel(out[k], oout[k].detach(), f"{cid}/{k}")
    if res is not None:
        want = torch.stack([torch.as_tensor(res[k]).detach() for k in ("loss_seg", "loss_action", "loss_dur", "loss")])
        assert_close(loss.cpu(), want, 1e-3, 1e-6, f"{cid}/losses")
    # ---- every live gradient
    kink = ffn_kink_units(oaux["ffn_pre"])
    print(f"[long] {cid}: {len(kink)} FFN units on the ReLU kink")
    assert len(kink) <= 4, f"{cid}: {len(kink)} FFN units on the ReLU kink"
    rtol = 2e-3 if not kink else 4e-3
    assert sorted(grads) == sorted(ograd), (cid, sorted(set(grads) ^ set(ograd)))
    for n, r in ograd.items():
        g, r = without_kink_units(n, grads[n].cpu(), r, kink)
        if n == "fc_len.bias" and c.variant == "depth":
            # exactly zero (a shift of every duration cancels in the L1 normalisation): rounding noise on both sides
            assert float(g.abs().max()) <= 5e-4 * float(grads["fc_len.weight"].abs().max()), cid
        else:
            close_rel(g, r, f"{cid}/grad {n}" + (f" (kink units {sorted(kink)} excluded)" if kink else ""), rtol=rtol)


def test_flag_off_still_refuses(monkeypatch):
    c = QC._c("depth", 1, 65, 128, 8, pad="none")
    eng = build_model(c, QS.params(c), long_clips=False).train().engine()
    big = [t.cuda() for t in QC.make_batch(c)]
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match="clip length 65 at head width 16.*--long_clips"):
        eng.train_step(big[0], big[1], big[2], big[3], big[4], 1e-3, 5e-3)
    assert not rec.calls and not eng.shapes


def _grads(eng, c, seed):
    d = [t.cuda() for t in QC.make_batch(c, seed=seed)]
    QS.run_step(eng, None, c, d)
    return {n: eng.arena.g(n).clone() for n in eng.arena.live_names}


def test_flag_on_at_an_old_shape_is_the_core_bit_for_bit(monkeypatch):
    c = QC._c("depth", 2, 16, 128, 8)
    p = QS.params(c)
    on, off = build_model(c, p).eval().engine(), build_model(c, p, long_clips=False).eval().engine()
    rec = Recorder(monkeypatch)
    got = _grads(on, c, 3)
    monkeypatch.undo()
    want = _grads(off, c, 3)
    torch.cuda.synchronize()
    names = rec.names()
    assert names.count("mha_core_fwd") == 2 and names.count("mha_core_bwd") == 2
    assert "mha_tiled_fwd" not in names and "mha_tiled_bwd" not in names
    assert on.last["w"].route == "core"
    for n in want:
        assert torch.equal(got[n], want[n]), n


def test_cached_shapes_keep_their_route_and_buffers():
    """S = 130, then S = 16, then S = 130 on one flag-on engine: each step gives a fresh engine's gradients bit for bit."""
    base = QC._c("depth", 1, 130, 64, 8, pad="none")
    p = QS.params(base)
    eng = build_model(base, p).eval().engine()
    fresh = {}
    for S in (130, 16, 130):
        c = base._replace(S=S)
        got = _grads(eng, c, 40 + S)
        if S not in fresh:
            fresh[S] = _grads(build_model(base, p).eval().engine(), c, 40 + S)
        torch.cuda.synchronize()
        for n, want in fresh[S].items():
            assert torch.equal(got[n], want), (S, n)
    assert {k[1]: w.route for k, w in eng.shapes.items()} == {130: "tiled", 16: "core"}


def test_forward_alone_at_a_long_clip(oracle_lib, monkeypatch):
    c = QC._c("depth", 2, 300, 128, 8)
    p = QS.params(c)
    batch = QC.make_batch(c)
    model = build_model(c, p).eval()
    d = [t.cuda() for t in batch]
    rec = Recorder(monkeypatch)
    with torch.no_grad():
        out = model((d[0], d[2]), d[1])
        b64 = QS.f64(batch)
        oout, _ = O.forward_unsup_depth({n: v.double() for n, v in p.items()}, (b64[0], b64[2]), b64[1], "train", c.K + 1,
                                        c.heads, c.n_dec, QC.Q)
    torch.cuda.synchronize()
    monkeypatch.undo()
    names = rec.names()
    assert names.count("mha_tiled_fwd") == 2 * c.n_dec and "mha_tiled_bwd" not in names and "mha_core_fwd" not in names
    w = model.engine().shapes[(c.B, c.S, False)]
    assert w.route == "tiled" and w.delta is None and not hasattr(w, "glayers")
    for k in ("action", "duration", "seg"):
        close_rel(out[k], oout[k], f"forward alone/{k}")


def _train_run(c, p, batches, graph_steps, tmp_path):
    from r3d_amd.train_proposed_depth import train
    from r3d_amd.optim import FlatAdamW, LinearWarmupCosineAnnealingLR
    model = build_model(c, p)
    model.r3d_dropout_enabled = False
    args = argparse.Namespace(epochs=1, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=1,
                              graph_steps=graph_steps)
    opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)
    sch = LinearWarmupCosineAnnealingLR(opt, warmup_epochs=2, max_epochs=4)
    sch.step()
    sch.step()
    tmp_path.mkdir()
    with contextlib.redirect_stdout(io.StringIO()):
        train(args, model, batches, opt, sch, None, str(tmp_path), c.K + 1, torch.device("cuda"), [batches[0]], seed=1)
    torch.cuda.synchronize()
    eng = model.engine()
    assert {k[1]: w.route for k, w in eng.shapes.items() if k[2]} == {65: "tiled", 80: "tiled"}
    return eng.arena.params[:eng.arena.n_live].clone()


def test_graph_replay_matches_the_eager_loop(tmp_path):
    """Six batches alternating S = 65 and S = 80 through train(): the launch path allocates nothing and never synchronises,
    so each shape's step is captured once and replayed; the live parameters end bit-equal to the launch-by-launch loop's."""
    c = QC._c("depth", 2, 65, 128, 8)
    p = QS.params(c)
    batches = [QC.make_batch(c._replace(S=65 if i % 2 == 0 else 80), seed=i) for i in range(6)]
    graphed = _train_run(c, p, batches, True, tmp_path / "g")
    eager = _train_run(c, p, batches, False, tmp_path / "e")
    assert bool(torch.isfinite(graphed).all())
    assert torch.equal(graphed, eager)


def test_dropout_on_a_long_clip():
    """The check tests/test_unsup_depth_gpu.test_dropout_and_train_loop makes, on the tiled route: the Philox pool's slice
    for the self-attention probabilities keeps 0.9 +- 0.02 of them and four training steps lower the loss."""
    c = QC._c("depth", 2, 65, 128, 8)
    eng = build_model(c, QS.params(c)).train().engine()
    d = [t.cuda() for t in QC.make_batch(c)]
    eng.forward(d[0], d[1], d[2], "train", training=True)
    torch.cuda.synchronize()
    w = eng.last["w"]
    assert w.route == "tiled" and eng.last["drop"]
    assert w.drop["sa_p0"].numel() == c.B * c.heads * c.S * c.S
    assert abs(float(w.drop["sa_p0"].float().mean()) - 0.9) < 0.02
    losses = []
    for _ in range(4):
        loss, _ = eng.train_step(d[0], d[1], d[2], d[3], d[4], 1e-3, 5e-3)
        losses.append(float(loss[3]))
    assert all(x == x for x in losses) and losses[-1] < losses[0], losses
