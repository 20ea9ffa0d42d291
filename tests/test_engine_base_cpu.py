"""r3d_amd/engine_base.py and r3d_amd/model/_bridge.py on the CPU: the arena's head views, the arena order of every model
through the live= rule its engine passes (against tests/golden/engine_base_parent.json, recorded before the engines shared a
base -- the two models whose arena lost its subclass are written out below as well), the engine's life cycle on a model and
the bridges' gradient scatter."""
import json
import os

import pytest
import torch
from torch import nn

from r3d_amd.engine_base import EngineBase, ParamArena
from r3d_amd.model._bridge import arena_grads, logit_grads_in
from tests import engine_base_cases as C

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_base_parent.json")) as _fh:
    PARENT = json.load(_fh)
_MODELS = {}


def model(name):
    """one instance per model class, shared (its arena re-points the parameters' storage; nothing else changes)"""
    if name not in _MODELS:
        torch.manual_seed(0)
        _MODELS[name] = C.MODELS[name][0]()
    return _MODELS[name]


# ---- ParamArena.head_views ----------------------------------------------------------------------------------------------
def _head_params(K, H):
    g = torch.Generator().manual_seed(5)
    shapes = {"fc_len.bias": (1,), "body.weight": (6, H), "fc.bias": (K,), "fc_len.weight": (1, H), "body.bias": (6,),
              "fc.weight": (K, H)}                                  # (registration order: nothing where the arena wants it)
    return [(n, nn.Parameter(torch.randn(*s, generator=g))) for n, s in shapes.items()]


def test_head_views_alias_the_arena_at_the_offsets():
    K, H = 3, 8
    named = _head_params(K, H)
    want = {n: p.detach().clone() for n, p in named}
    a = ParamArena(named, torch.device("cpu"), lambda n: True)
    w, gw, b, gb = a.head_views(K, H)
    assert w.shape == gw.shape == (K + 1, H) and b.shape == gb.shape == (K + 1,)
    o_w, o_b = a.offsets["fc.weight"][0], a.offsets["fc.bias"][0]
    assert o_w == 0 and a.offsets["fc_len.weight"][0] == K * H and a.offsets["fc_len.bias"][0] == o_b + K
    assert torch.equal(w, torch.cat([want["fc.weight"], want["fc_len.weight"]])) and torch.equal(w[K], a.p("fc_len.weight")[0])
    assert torch.equal(b, torch.cat([want["fc.bias"], want["fc_len.bias"]]))
    for view, flat, o in ((w, a.params, o_w), (gw, a.grads, o_w), (b, a.params, o_b), (gb, a.grads, o_b)):
        assert view.data_ptr() == flat[o:].data_ptr() and view.is_contiguous()
        before = flat.clone()
        view.fill_(7.0)                                             # lands in the arena, in [o, o + numel) and nowhere else
        changed = (flat != before).nonzero().flatten()
        assert changed.tolist() == list(range(o, o + view.numel())) and bool((flat[o:o + view.numel()] == 7.0).all())
        flat.copy_(before)
    assert torch.equal(w[:K], want["fc.weight"]) and dict(named)["fc.bias"].data_ptr() == b.data_ptr()


def test_head_views_refuse_a_dead_fc_len():
    K, H = 3, 8
    a = ParamArena(_head_params(K, H), torch.device("cpu"), lambda n: not n.startswith("fc_len."))
    assert a.offsets["fc_len.weight"][0] >= a.n_live
    with pytest.raises(AssertionError):
        a.head_views(K, H)


# ---- the arena order of every model class ---------------------------------------------------------------------------------
UNSUP_DEPTH_LIVE = {
    "fc.weight": 0, "fc_len.weight": 80, "input_embed.weight": 96, "input_embed.bias": 480,
    "transformer.decoder.layers.0.linear1.weight": 496, "transformer.decoder.layers.0.linear1.bias": 1520,
    "transformer.decoder.layers.0.linear2.weight": 1584, "transformer.decoder.layers.0.linear2.bias": 2608,
    "transformer.decoder.layers.0.norm1.weight": 2624, "transformer.decoder.layers.0.norm1.bias": 2640,
    "transformer.decoder.layers.0.norm2.weight": 2656, "transformer.decoder.layers.0.norm2.bias": 2672,
    "transformer.decoder.layers.0.norm3.weight": 2688, "transformer.decoder.layers.0.norm3.bias": 2704,
    "transformer.decoder.layers.0.self_attn.in_proj_weight": 2720,
    "transformer.decoder.layers.0.self_attn.in_proj_bias": 3488,
    "transformer.decoder.layers.0.self_attn.out_proj.weight": 3536,
    "transformer.decoder.layers.0.self_attn.out_proj.bias": 3792,
    "transformer.decoder.layers.0.multihead_attn.in_proj_weight": 3808,
    "transformer.decoder.layers.0.multihead_attn.in_proj_bias": 4576,
    "transformer.decoder.layers.0.multihead_attn.out_proj.weight": 4624,
    "transformer.decoder.layers.0.multihead_attn.out_proj.bias": 4880, "transformer.decoder.norm.weight": 4896,
    "transformer.decoder.norm.bias": 4912, "fc_seg.weight": 4928, "depth_projection.bias": 5008,
    "depth_layernorm.weight": 5024, "depth_layernorm.bias": 5040, "fc.bias": 5056, "fc_len.bias": 5061,
    "fc_seg.bias": 5062, "pos_embedding": 5068, "depth_projection.weight": 5260}
UNSUP_LABEL_LIVE = {
    "fc.weight": 0, "fc_len.weight": 80, "input_embed.weight": 96, "input_embed.bias": 480,
    "transformer.decoder.layers.0.linear1.weight": 496, "transformer.decoder.layers.0.linear1.bias": 1520,
    "transformer.decoder.layers.0.linear2.weight": 1584, "transformer.decoder.layers.0.linear2.bias": 2608,
    "transformer.decoder.layers.0.norm1.weight": 2624, "transformer.decoder.layers.0.norm1.bias": 2640,
    "transformer.decoder.layers.0.norm2.weight": 2656, "transformer.decoder.layers.0.norm2.bias": 2672,
    "transformer.decoder.layers.0.norm3.weight": 2688, "transformer.decoder.layers.0.norm3.bias": 2704,
    "transformer.decoder.layers.0.self_attn.in_proj_weight": 2720,
    "transformer.decoder.layers.0.self_attn.in_proj_bias": 3488,
    "transformer.decoder.layers.0.self_attn.out_proj.weight": 3536,
    "transformer.decoder.layers.0.self_attn.out_proj.bias": 3792,
    "transformer.decoder.layers.0.multihead_attn.in_proj_weight": 3808,
    "transformer.decoder.layers.0.multihead_attn.in_proj_bias": 4576,
    "transformer.decoder.layers.0.multihead_attn.out_proj.weight": 4624,
    "transformer.decoder.layers.0.multihead_attn.out_proj.bias": 4880, "transformer.decoder.norm.weight": 4896,
    "transformer.decoder.norm.bias": 4912, "query_embed.weight": 4928, "fc_seg.weight": 5696, "fc_seg.bias": 5760,
    "fc.bias": 5764, "fc_len.bias": 5769, "pos_embedding": 5772}
WRITTEN_OUT = {"unsup_depth": (UNSUP_DEPTH_LIVE, 5452, 11744), "unsup_label": (UNSUP_LABEL_LIVE, 5964, 9244)}


@pytest.mark.parametrize("name", list(C.MODELS))
def test_arena_order_equals_the_parents(name):
    m = model(name)
    values = {n: p.detach().clone() for n, p in m.named_parameters()}
    a = C.arena(name, m)
    want = PARENT[name]
    assert C.offsets(a) == want["offsets"] and list(a.offsets) == list(want["offsets"])
    assert (a.n_live, a.n_total, a.live_names) == (want["n_live"], want["n_total"], want["live_names"])
    assert [n for n, _ in m.named_parameters() if a.is_live(n)] == want["attach_live"]
    for n, p in m.named_parameters():                               # the parameters moved into the arena unchanged
        assert torch.equal(p, values[n]) and p.data_ptr() == a.p(n).data_ptr()
    if name in WRITTEN_OUT:
        live, n_live, n_total = WRITTEN_OUT[name]
        assert {n: a.offsets[n][0] for n in a.live_names} == live and list(live) == a.live_names
        assert (a.n_live, a.n_total) == (n_live, n_total)
    if "fc_len.weight" in a.offsets:                                # (every model but the TCN)
        assert a.head_views(m.n_class, m.hidden_dim)[0].shape == (m.n_class + 1, m.hidden_dim)


# ---- EngineOwner ----------------------------------------------------------------------------------------------------------
NAMES = {"cnn": "r3d_amd.model.cnn.FUTR", "rnn": "r3d_amd.model.rnn.FUTR", "tcn": "r3d_amd.model.tcn.MustafaNet1DTCN"}


@pytest.mark.parametrize("name", list(C.MODELS))
def test_engine_owner_on_a_cpu_model(name):
    m = model(name)
    assert list(m.state_dict().keys()) == PARENT[name]["state_keys"]
    with pytest.raises(RuntimeError) as e:
        m.engine()
    assert str(e.value) == (f"{NAMES.get(name, 'r3d_amd.FUTR')} computes only on an MI355X through libr3d_hip.so; move the "
                            f"model to the GPU with .to('cuda') (there is deliberately no CPU path).")
    assert m._engine is None
    m._engine = stale = object()
    assert m.to("cpu") is m and m._engine is None and stale is not None         # .to() drops the engine
    m._engine = object()
    m.float()
    assert m._engine is None


def test_engine_base_declares_the_surface_the_callers_read():
    e = EngineBase()
    assert (e.dur_den, e.grad_hook, e.score_allreduce, e.tp, e.bn_sync, e.rank_stream) == (None,) * 6
    assert (e._drop_ready, e._loss_pending, e.loss_acc, e.last, e.erank_fold) == (None,) * 5
    assert (e.defer_tail, e.fused_loss_flow, e.rank_penalty, e.bn, e.vary) == (False,) * 5
    assert (e.erank_weight, e.erank_route, e.pos_grad_rows) == (0.0, "jacobi", 0) and e.depth_adamw_fusable() is False
    from r3d_amd import engine, engine_afft, engine_cnn, engine_l3, engine_m3, engine_rnn, engine_tcn, engine_unsup
    flow = {engine.FusionEngine: (True, True), engine_afft.AfftEngine: (True, False), engine_m3.M3Engine: (False, True)}
    for cls in (engine.FusionEngine, engine_afft.AfftEngine, engine_cnn.CnnEngine, engine_rnn.RnnEngine, engine_tcn.TcnEngine,
                engine_unsup.UnsupDepthEngine, engine_l3.L3Engine, engine_m3.M3Engine):
        assert issubclass(cls, EngineBase) and (cls.fused_loss_flow, cls.rank_penalty) == flow.get(cls, (False, False))
        assert "set_lr" not in vars(cls) and "_dm2" not in vars(cls) and "_copy_in" not in vars(cls)


# ---- the bridges' halves ----------------------------------------------------------------------------------------------------
class _W:
    pass


def _workspace(BQ, N, K, seg=True):
    w = _W()
    w.d_actdur = torch.full((BQ, K + 1), 9.0)
    if seg:
        w.d_seg = torch.full((N, K), 9.0)
    return w


def test_logit_grads_in_scatters_and_zeroes():
    B, Q, S, K = 2, 4, 3, 5
    g = torch.Generator().manual_seed(2)
    d_act, d_dur, d_seg = torch.randn(B, Q, K, generator=g), torch.randn(B, Q, generator=g), torch.randn(B, S, K, generator=g)
    w = _workspace(B * Q, B * S, K)
    logit_grads_in(w, K, d_act, d_dur, d_seg)
    assert torch.equal(w.d_actdur[:, :K], d_act.reshape(-1, K)) and torch.equal(w.d_actdur[:, K], d_dur.reshape(-1))
    assert torch.equal(w.d_seg, d_seg.reshape(-1, K))
    for skip in range(3):                                           # one output unused by the caller's loss: zero, not stale
        w = _workspace(B * Q, B * S, K)
        args = [d_act, d_dur, d_seg]
        args[skip] = None
        logit_grads_in(w, K, *args)
        got = (w.d_actdur[:, :K], w.d_actdur[:, K], w.d_seg)
        want = (d_act.reshape(-1, K), d_dur.reshape(-1), d_seg.reshape(-1, K))
        for i in range(3):
            assert torch.equal(got[i], torch.zeros_like(want[i]) if i == skip else want[i]), (skip, i)
    w = _workspace(B * Q, B * S, K, seg=False)                      # (AFFT: no 'seg' output, no buffer for its gradient)
    logit_grads_in(w, K, None, d_dur, None)
    assert not w.d_actdur[:, :K].any() and torch.equal(w.d_actdur[:, K], d_dur.reshape(-1)) and not hasattr(w, "d_seg")


def test_arena_grads_copies_the_live_gradients():
    K, H = 3, 8
    named = _head_params(K, H)
    eng = _W()
    eng.arena = a = ParamArena(named, torch.device("cpu"), lambda n: not n.startswith("body."))
    a.grads.copy_(torch.arange(a.n_live, dtype=torch.float32))
    names = [n for n, _ in named]
    out = arena_grads(eng, names)
    assert isinstance(out, tuple) and len(out) == len(names)
    for n, g in zip(names, out):
        if n.startswith("body."):
            assert g is None
        else:
            assert torch.equal(g, a.g(n)) and g.data_ptr() != a.g(n).data_ptr() and g.shape == dict(named)[n].shape
