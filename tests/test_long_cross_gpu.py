"""The fusion engine's cross-attention past the core (engine.cross_attention_route, opts --long_clips): whole training steps
against the oracle run in float64, through the helpers of tests/test_width_shapes_gpu.py.

Forced small shapes (FusionEngine.cross_route) run the split-key launches (csrc/attention_splitk.hip) and the tiled fallback
where the S x S core runs too: the oracle's bounds hold (outputs, fused tokens and losses within 1e-3 of scale, every gradient
within 2e-3, 4e-3 beside a ReLU kink) and the step agrees with the same step on the "core" route within the kernels' own
tolerances (1e-4 of scale for outputs, 1e-3 for gradients).  By rule, with the flag: the first clips past the core at head
widths 128 and 16, and a validation forward past the forward-only bound.  Then: the flag off still refuses, naming the flag;
the flag on where the core fits changes no bit; an eager and a graphed step with dropout give the same bits; a data-parallel
engine refuses a routed clip.  Needs an MI355X."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import futr_oracle as O  # noqa: E402
from tests import test_width_shapes_gpu as WS  # noqa: E402
from tests import width_cases as WC  # noqa: E402
from tests.helpers import assert_close, ffn_kink_units, without_kink_units  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

ARGS_LONG = argparse.Namespace(**vars(WS.ARGS), long_clips=True)


class Recorder(WS.Recorder):
    NAMES = ("mha_core_fwd", "mha_core_bwd", "mha_splitk_fwd", "mha_splitk_bwd", "mha_tiled_fwd", "mha_tiled_bwd",
             "embed_fuse_fwd", "plain_fuse_fwd", "token_exchange_fwd", "check")


def build_model(c, p, long_clips=False, n_dec=1):
    """tests/test_width_shapes_gpu.build_model with the flag in the args namespace and a decoder depth."""
    model = WS._cls(c.variant)(c.K, c.H, c.K + 1, torch.device("cuda"), ARGS_LONG if long_clips else WS.ARGS, n_query=WC.Q,
                               n_head=c.heads, num_encoder_layers=2, num_decoder_layers=n_dec)
    assert model.r3d_long_clips is long_clips
    assert not model.load_state_dict(p, strict=False).unexpected_keys
    return model.to("cuda")


def params(c, n_dec=1):
    if n_dec == 1:
        return WS.params(c.variant, c.H, c.heads, c.K)
    from oracle import synth
    m = WS._cls(c.variant)(c.K, c.H, c.K + 1, torch.device("cpu"), WS.ARGS, n_query=WC.Q, n_head=c.heads,
                           num_encoder_layers=2, num_decoder_layers=n_dec)
    return {n: torch.from_numpy(synth.fill_value(n, tuple(q.shape), j)) for j, (n, q) in enumerate(m.named_parameters())}


def step(eng, d, training=False):
    """One forward + losses + backward as the width test runs it; (workspace, loss, outputs, gradients), cloned."""
    eng.forward(d[0], d[1], d[2], "train", training=training)
    w = eng.last["w"]
    loss, _ = eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()
    K = eng.K
    out = dict(seg=w.seg.clone(), action=w.actdur[:, :K].clone(), duration=w.actdur[:, K].clone(), fused=w.fused.clone())
    return w, loss.clone(), out, {n: eng.arena.g(n).clone() for n in eng.arena.live_names}


def check_oracle(cid, c, w, loss, out, grads, tr, res, oout, oaux):
    """The bounds of tests/test_width_shapes_gpu.test_width_shape_against_fp64_oracle."""
    B, S, H, K = c.B, c.S, c.H, c.K
    shaped = dict(seg=out["seg"].view(B, S, K), action=out["action"].reshape(B, WC.Q, K), duration=out["duration"].reshape(B, WC.Q))
    for k in ("action", "duration", "seg"):
        close_rel(shaped[k], oout[k].detach(), f"{cid}/{k}")
    close_rel(out["fused"].view(B, S, H), oaux["fused"].detach(), f"{cid}/fused")
    want = torch.stack([torch.as_tensor(res[k]).detach() for k in ("loss_seg", "loss_action", "loss_dur", "loss")])
    assert_close(loss.cpu(), want, 1e-3, 1e-6, f"{cid}/losses")
    kink = ffn_kink_units(oaux["ffn_pre"]) if "ffn_pre" in oaux else set()
    assert len(kink) <= 4, f"{cid}: {len(kink)} FFN units on the ReLU kink"
    rtol = 2e-3 if not kink else 4e-3
    n_grads = 0
    for n, q in tr.p.items():
        if q.grad is None:
            continue
        g, r = without_kink_units(n, grads[n].cpu(), q.grad, kink)
        if n == "fc_len.bias":          # exactly zero (a shift of every duration cancels in the L1 normalisation)
            assert float(g.abs().max()) <= 5e-4 * float(grads["fc_len.weight"].abs().max()), cid
        else:
            close_rel(g, r, f"{cid}/grad {n}" + (f" (kink units {sorted(kink)} excluded)" if kink else ""), rtol=rtol)
        n_grads += 1
    assert n_grads == len(grads), cid


def attention_calls(rec, S):
    """{launch name: count} of the cross-attention launches (Lk = S; the self-attention's S x S core calls have Lk = Q)."""
    got = {}
    for n, a in rec.calls:
        if n.startswith("mha_") and a[-2] == S and a[-3] == WC.Q:
            got[n] = got.get(n, 0) + 1
    return got


FORCED = [
    (WC._c(2, 16, 136, 8), "splitk", 1),
    (WC._c(3, 300, 128, 8, pad=(1, 150, 300)), "splitk", 1),
    (WC._c(2, 16, 200, 8, K=122, variant="plain", tail1=False), "splitk", 1),
    (WC._c(2, 16, 136, 8), "tiled", 1),
    (WC._c(2, 16, 136, 8), "splitk", 2),
]


@pytest.mark.parametrize("c,route,n_dec", FORCED, ids=lambda v: WC.case_id(v) if isinstance(v, WC.Case) else str(v))
def test_forced_route_against_fp64_oracle_and_the_core_route(c, route, n_dec, oracle_lib, monkeypatch):
    cid = f"{WC.case_id(c)}/{route}/L{n_dec}"
    batch = WC.make_batch(c)
    p = params(c, n_dec)
    if n_dec == 1:
        tr, res, oout, oaux, _ = WS.oracle64(c, batch, p)
    else:                                   # (the width test's helper is written for one layer: the oracle's own trainer)
        tr = O.CpuTrainer({n: v.double() for n, v in p.items()}, c.K + 1, c.heads, n_dec)
        res, oout, oaux = tr.step(WS.f64(batch), apply=False)
    d = [t.cuda() for t in batch]
    eng = build_model(c, p, n_dec=n_dec).eval().engine()
    eng.defer_tail = True
    eng.cross_route = route
    rec = Recorder(monkeypatch)
    w, loss, out, grads = step(eng, d)
    monkeypatch.undo()
    assert w.route == route and all("p_ca" not in lay and "lse_ca" in lay for lay in w.layers), cid
    assert all(("ws_ca" in lay) == (route == "splitk") for lay in w.layers) and tuple(w.delta.shape) == (c.B, c.heads, WC.Q)
    assert attention_calls(rec, c.S) == {f"mha_{route}_fwd": n_dec, f"mha_{route}_bwd": n_dec}, (cid, rec.names())
    check_oracle(cid, c, w, loss, out, grads, tr, res, oout, oaux)
    # the same step on the core route: two fp32 evaluations of the same sums
    core = build_model(c, p, n_dec=n_dec).eval().engine()
    core.defer_tail = True
    core.cross_route = "core"
    wc, loss_c, out_c, grads_c = step(core, d)
    assert wc.route == "core" and all("p_ca" in lay for lay in wc.layers), cid
    for k in out:
        close_rel(out[k], out_c[k], f"{cid}/{k} against the core route", rtol=1e-4)
    for n in grads:
        if n == "fc_len.bias":
            continue
        close_rel(grads[n], grads_c[n], f"{cid}/grad {n} against the core route", rtol=1e-3)


BY_RULE = [WC._c(1, 934, 1024, 8, pad="none", tail1=False, side=True), WC._c(1, 1606, 128, 8, pad="none")]


@pytest.mark.parametrize("c", BY_RULE, ids=WC.case_id)
def test_first_clip_past_the_core_trains_with_the_flag(c, oracle_lib, monkeypatch):
    """The rows tests/width_cases.py lists as refused (the flag off), at the tolerances of its (1, 933, 1024, 8) row."""
    cid = WC.case_id(c) + "/long_clips"
    batch = WC.make_batch(c)
    p = params(c)
    tr, res, oout, oaux, _ = WS.oracle64(c, batch, p)
    d = [t.cuda() for t in batch]
    off = build_model(c, p).train().engine()
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match=f"clip length {c.S} at head width {c.H // c.heads}.*--long_clips"):
        off.train_step(d[0], d[1], d[2], d[3], d[4], 1e-3, 5e-3)
    assert not rec.calls and not off.shapes, rec.names()
    del off
    eng = build_model(c, p, long_clips=True).eval().engine()
    eng.defer_tail = True
    assert eng.long_clips and eng.cross_route is None
    w, loss, out, grads = step(eng, d)
    monkeypatch.undo()
    assert w.route == "splitk" and eng._multi_stream() == c.side, cid
    assert attention_calls(rec, c.S) == {"mha_splitk_fwd": 1, "mha_splitk_bwd": 1}, (cid, rec.names())
    check_oracle(cid, c, w, loss, out, grads, tr, res, oout, oaux)


def test_val_forward_past_the_forward_only_bound(oracle_lib, monkeypatch):
    """(1, 1465, 1024, 8): one frame past the longest forward-only clip.  The flag off refuses before any launch; with it
    validate()'s forward matches the fp64 oracle's."""
    c = WC._c(1, 1465, 1024, 8, pad="none")
    batch = WC.make_batch(c)
    p = params(c)
    d = [t.cuda() for t in batch]
    off = build_model(c, p).eval().engine()
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match="clip length 1465 at head width 128.*forward.*--long_clips"):
        off.forward(d[0], d[1], d[2], "val", training=False, need_grad=False)
    assert not rec.calls and not off.shapes, rec.names()
    del off
    eng = build_model(c, p, long_clips=True).eval().engine()
    out = {k: v.clone() for k, v in eng.forward(d[0], d[1], d[2], "val", training=False, need_grad=False).items()}
    torch.cuda.synchronize()
    monkeypatch.undo()
    w = eng.last["w"]
    assert w.route == "splitk" and not hasattr(w, "delta") and not hasattr(w, "glayers")
    assert attention_calls(rec, c.S) == {"mha_splitk_fwd": 1}, rec.names()
    oout, _ = WS.val_oracle("tf", p, batch, c.K, c.heads, None, torch.float64)
    for k in ("action", "duration", "seg"):
        close_rel(out[k], oout[k], f"val S1465/{k}")


def test_flag_on_where_the_core_fits_changes_no_bit(monkeypatch):
    c = WC._c(1, 257, 128, 8)
    p = params(c)
    d = [t.cuda() for t in WC.make_batch(c)]
    on, off = build_model(c, p, long_clips=True).eval().engine(), build_model(c, p).eval().engine()
    rec = Recorder(monkeypatch)
    w, loss, out, grads = step(on, d)
    monkeypatch.undo()
    _, loss0, out0, grads0 = step(off, d)
    assert w.route == "core" and attention_calls(rec, c.S) == {"mha_core_fwd": 1, "mha_core_bwd": 1}, rec.names()
    assert torch.equal(loss, loss0)
    for k in out:
        assert torch.equal(out[k], out0[k]), k
    for n in grads:
        assert torch.equal(grads[n], grads0[n]), n


def test_graphed_step_with_dropout_gives_the_eager_bits():
    """Forced split-key at (2, 16, 136, 8), dropout on: the launches allocate nothing and never synchronise, so the step is
    captured; at the same seed and offset the replay's outputs and gradients are the eager step's."""
    c = WC._c(2, 16, 136, 8)
    p = params(c)
    d = [t.cuda() for t in WC.make_batch(c)]
    eng = build_model(c, p).train().engine()
    eng.cross_route = "splitk"
    w, loss, out, grads = step(eng, d, training=True)          # eager (and the warm-up: shape buffers, function attributes)
    assert w.route == "splitk" and eng.last["drop"] and int(eng.drop_offset.item()) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.forward(d[0], d[1], d[2], "train", training=True)
        loss_g, _ = eng.losses(d[2], d[4], d[3])
        eng.backward()
    for t in (w.seg, w.actdur, eng.arena.grads):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert int(eng.drop_offset.item()) == 0
    assert torch.equal(loss_g, loss) and torch.equal(w.seg, out["seg"]) and torch.equal(w.actdur[:, :eng.K], out["action"])
    for n in grads:
        assert torch.equal(eng.arena.g(n), grads[n]), n
    assert bool(torch.isfinite(eng.arena.grads[:eng.arena.n_live]).all())


def test_train_loop_takes_1142_frame_clips_at_hidden_1024(tmp_path):
    """train_proposed_depth.train() with graph replay over two batches of one 1142-frame clip at hidden 1024 with 8 heads (a
    whole DARai observation at configuration five's width): raises without the flag, trains with it."""
    import contextlib
    import io
    from r3d_amd.train_proposed_depth import train
    from r3d_amd.optim import FlatAdamW, LinearWarmupCosineAnnealingLR
    c = WC._c(1, 1142, 1024, 8, pad="none")
    p = params(c)
    batches = [WC.make_batch(c, seed=i) for i in range(2)]
    args = argparse.Namespace(epochs=1, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=1,
                              graph_steps=True)
    ends = {}
    for flag in (False, True):
        model = build_model(c, p, long_clips=flag)
        opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)
        sch = LinearWarmupCosineAnnealingLR(opt, warmup_epochs=2, max_epochs=4)
        sch.step()
        sch.step()
        out = tmp_path / str(flag)
        out.mkdir()
        run = lambda: train(args, model, batches, opt, sch, None, str(out), c.K + 1, torch.device("cuda"), [batches[0]],   # noqa: E731
                            seed=1)
        with contextlib.redirect_stdout(io.StringIO()):
            if flag:
                run()
            else:
                with pytest.raises(ValueError, match="clip length 1142 at head width 128.*--long_clips"):
                    run()
        torch.cuda.synchronize()
        eng = model.engine()
        ends[flag] = eng.arena.params[:eng.arena.n_live].clone()
        assert {k[1]: w.route for k, w in eng.shapes.items() if k[2]} == ({1142: "splitk"} if flag else {})
    assert bool(torch.isfinite(ends[True]).all()) and not torch.equal(ends[True], ends[False])


def test_data_parallel_engine_refuses_a_routed_clip(monkeypatch):
    """As erank_route "tall": the routes past the core have only run on one GPU."""
    c = WC._c(2, 16, 136, 8)
    p = params(c)
    d = [t.cuda() for t in WC.make_batch(c)]
    eng = build_model(c, p).eval().engine()
    eng.cross_route = "splitk"
    eng.grad_hook = lambda stage: None         # what parallel.DataParallelEngine sets
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match="data-parallel or pixel-sharded.*one GPU"):
        eng.forward(d[0], d[1], d[2], "train", training=False)
    assert not rec.calls and not eng.shapes, rec.names()
    eng.cross_route = None                      # by rule this clip runs on the core: admitted as before
    eng.forward(d[0], d[1], d[2], "train", training=False)
    torch.cuda.synchronize()
    assert eng.last["w"].route == "core"
