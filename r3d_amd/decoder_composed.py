"""The post-norm transformer decoder (reference transformer.py:281-330) composed launch by launch from ops.gemm, ops.mha_* and
ops.layernorm_*, shared by the query engines engine_unsup, engine_l3 and engine_m3 (the token-fusion engine's decoder is
interleaved with streams, chain kernels and deferred tails: engine.py keeps its own; its dropout pool is laid out here too).

One decoder serves the three: `rows` query rows (B clips x Tq queries) attend to themselves and to the B x S rows of `mem`
(+ pos_embedding[:S]).  What differs comes in as arguments:
  qpos, qmod   the query position and its broadcast modulus -- an activation [rows, H] with modulus rows, or the query_embed
               parameter [Q, H] with modulus Q;
  g_qpos       where the query position's gradient goes -- None: added into w.d_qpos through w.d_qtmp (an activation: it flows
               on into the engine's branch); a parameter's gradient tensor: folded over the clips with rowmod_sum;
  mem          the memory (w.mem or w.fused);
  w.route      the route of both attentions (r3d_amd/attention.py).
Kernels are called as attributes of the ops module: the tests patch them there and count the calls."""
import torch

from . import attention, ops
from ._lib import GEMM_NT, GEMM_NN, GEMM_TN
from .engine_base import DROP_P

DROP_SCALE = 1.0 / (1.0 - DROP_P)


# ---- buffers ------------------------------------------------------------------------------------------------------------
def decoder_drop_sizes(L, B, heads, H, rows, Tq, Tk):
    """{site: numel} of the decoder's dropout keep-masks, layer by layer."""
    sizes = {}
    for l in range(L):
        sizes.update({f"sa_p{l}": B * heads * Tq * Tq, f"ca_p{l}": B * heads * Tq * Tk, f"d1_{l}": rows * H,
                      f"d2_{l}": rows * H, f"d3_{l}": rows * H, f"ff_{l}": rows * 4 * H})
    return sizes


def drop_pool(sizes, device):
    """(pool, {site: view}): one uint8 pool that a single Philox launch fills, every site at a 16-byte aligned offset in the
    order of `sizes` -- the order is behaviour: the mask a site receives depends on its offset."""
    tot = sum((v + 15) // 16 * 16 for v in sizes.values())
    pool = torch.ones(tot, dtype=torch.uint8, device=device)
    views, o = {}, 0
    for k, v in sizes.items():
        views[k] = pool[o:o + v]
        o += (v + 15) // 16 * 16
    return pool, views


def decoder_buffers(w, eng, Tq, route, train, own_drop_sizes):
    """The decoder's activations (w.tgt0, w.layers, w.tgtF ...), with `train` its gradients (w.glayers, w.d_mp ...) and the
    dropout pool (the engine's own sites first, then the layers), on the shape workspace w (w.B, w.S, w.N are set)."""
    dev, H, L, heads, B, S, N = eng.device, eng.H, eng.L, eng.heads, w.B, w.S, w.N
    R = B * Tq
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)     # noqa: E731
    w.route = route
    att = lambda: {**attention.saved(route, "sa", f, B, heads, Tq, Tq, H // heads, train),        # noqa: E731
                   **attention.saved(route, "ca", f, B, heads, Tq, S, H // heads, train)}
    w.delta = attention.delta_buffer(route, f, B, heads, Tq, train)
    w.tgt0 = torch.zeros(R, H, dtype=torch.float32, device=dev)           # tgt = zeros_like(query)
    w.layers = [dict(sa_qkv=f(R, 3 * H), sa_o=f(R, H), t1_pre=f(R, H), t1=f(R, H), m1=f(R), r1=f(R), caq=f(R, H),
                     cakv=f(N, 2 * H), ca_o=f(R, H), t2_pre=f(R, H), t2=f(R, H), m2=f(R), r2=f(R), ff1=f(R, 4 * H),
                     t3_pre=f(R, H), t3=f(R, H), m3=f(R), r3=f(R), **att()) for _ in range(L)]
    w.tgtF, w.mF, w.rF = f(R, H), f(R), f(R)
    if train:
        w.d_tgtF, w.d_t, w.d_mp = f(R, H), f(R, H), f(N, H)
        w.glayers = [dict(t3pre=f(R, H), ff2=f(R, H), ff1=f(R, 4 * H), t2=f(R, H), t2pre=f(R, H), cap=f(R, H), cao=f(R, H),
                          caq=f(R, H), cakv=f(N, 2 * H), caqin=f(R, H), t1pre=f(R, H), sap=f(R, H), sao=f(R, H),
                          saqkv=f(R, 3 * H), sain=f(R, H)) for _ in range(L)]
        w.drop_pool, w.drop = drop_pool({**own_drop_sizes, **decoder_drop_sizes(L, B, heads, H, R, Tq, S)}, dev)


# ---- forward and backward -----------------------------------------------------------------------------------------------
def decoder_forward(eng, w, qpos, qmod, mem, key_labels, drop):
    """w.tgt0 through the layers and transformer.decoder.norm into w.tgtF.  q = k = tgt + query_pos in the self-attention,
    q = tgt + query_pos against k = v = memory + pos in the cross-attention, whose keys key_labels == pad_idx mask."""
    a, H, heads, dh, ws, B, S = eng.arena, eng.H, eng.heads, eng.dh, eng.ws, w.B, w.S
    R = w.tgt0.shape[0]
    Tq = R // B
    dm = (lambda k: w.drop[k]) if drop else (lambda k: None)
    dm2 = lambda k, cols: eng._dm2(dm(k), R, cols)         # noqa: E731
    dsc = DROP_SCALE

    pos = a.p("pos_embedding")[0, :S]
    tgt = w.tgt0
    for l in range(eng.L):
        c, pl = w.layers[l], f"transformer.decoder.layers.{l}."
        p = lambda n: a.p(pl + n)         # noqa: E731
        ops.gemm(GEMM_NT, tgt, p("self_attn.in_proj_weight"), c["sa_qkv"], a_add=qpos, a_add_mod=qmod,
                 bias=p("self_attn.in_proj_bias"), ws=ws)
        attention.forward(w.route, "sa", c, *attention.thirds(c["sa_qkv"]), (B, heads, Tq, Tq, dh), dm(f"sa_p{l}"), dsc)
        ops.gemm(GEMM_NT, c["sa_o"], p("self_attn.out_proj.weight"), c["t1_pre"], bias=p("self_attn.out_proj.bias"),
                 drop_mask=dm2(f"d1_{l}", H), drop_scale=dsc, res1=None if l == 0 else tgt, ws=ws)
        ops.layernorm_fwd(c["t1_pre"], p("norm1.weight"), p("norm1.bias"), c["t1"], c["m1"], c["r1"])
        wi, bi = p("multihead_attn.in_proj_weight"), p("multihead_attn.in_proj_bias")
        ops.gemm(GEMM_NT, c["t1"], wi[:H], c["caq"], a_add=qpos, a_add_mod=qmod, bias=bi[:H], ws=ws)
        ops.gemm(GEMM_NT, mem, wi[H:], c["cakv"], a_add=pos, a_add_mod=S, bias=bi[H:], ws=ws)
        attention.forward(w.route, "ca", c, c["caq"], c["cakv"][:, :H], c["cakv"][:, H:], (B, heads, Tq, S, dh), dm(f"ca_p{l}"),
                          dsc, key_labels=key_labels, pad_idx=eng.pad_idx)
        ops.gemm(GEMM_NT, c["ca_o"], p("multihead_attn.out_proj.weight"), c["t2_pre"],
                 bias=p("multihead_attn.out_proj.bias"), drop_mask=dm2(f"d2_{l}", H), drop_scale=dsc, res1=c["t1"], ws=ws)
        ops.layernorm_fwd(c["t2_pre"], p("norm2.weight"), p("norm2.bias"), c["t2"], c["m2"], c["r2"])
        ops.gemm(GEMM_NT, c["t2"], p("linear1.weight"), c["ff1"], bias=p("linear1.bias"), act=1,
                 drop_mask=dm2(f"ff_{l}", 4 * H), drop_scale=dsc, ws=ws)
        ops.gemm(GEMM_NT, c["ff1"], p("linear2.weight"), c["t3_pre"], bias=p("linear2.bias"),
                 drop_mask=dm2(f"d3_{l}", H), drop_scale=dsc, res1=c["t2"], ws=ws)
        ops.layernorm_fwd(c["t3_pre"], p("norm3.weight"), p("norm3.bias"), c["t3"], c["m3"], c["r3"])
        tgt = c["t3"]
    ops.layernorm_fwd(tgt, a.p("transformer.decoder.norm.weight"), a.p("transformer.decoder.norm.bias"), w.tgtF, w.mF, w.rF)


def decoder_backward(eng, w, qpos, qmod, mem, key_labels, drop, g_qpos=None):
    """Adjoint of decoder_forward from w.d_tgtF: every decoder parameter's gradient, the query position's (see g_qpos),
    d (memory + pos) in w.d_mp and, from it, pos_embedding's gradient."""
    a, H, heads, dh, ws, B, S, L = eng.arena, eng.H, eng.heads, eng.dh, eng.ws, w.B, w.S, eng.L
    R = w.tgt0.shape[0]
    Tq = R // B
    dm = (lambda k, cols: w.drop[k].view(R, cols)) if drop else (lambda k, cols: None)
    dmf = (lambda k: w.drop[k]) if drop else (lambda k: None)
    dsc = DROP_SCALE
    pos = a.p("pos_embedding")[0, :S]

    def ln_bwd(dy, x, mean, rstd, name, dx, **kw):
        gn, bn = name + ".weight", name + ".bias"
        ops.layernorm_bwd(dy, x, mean, rstd, a.p(gn), a.p(bn), dx, a.g(gn), a.g(bn), ws=ws, **kw)

    def wgrad(dy, x, gw, gb, **kw):
        ops.gemm(GEMM_TN, dy, x, gw, bias_grad=gb, ws=ws, **kw)

    ln_bwd(w.d_tgtF, w.layers[-1]["t3"], w.mF, w.rF, "transformer.decoder.norm", w.d_t)
    dy, dy2 = w.d_t, None
    for l in reversed(range(L)):
        c, gl, pl = w.layers[l], w.glayers[l], f"transformer.decoder.layers.{l}."
        p = lambda n: a.p(pl + n)         # noqa: E731
        g = lambda n: a.g(pl + n)         # noqa: E731
        tgt_in = w.tgt0 if l == 0 else w.layers[l - 1]["t3"]
        ln_bwd(dy, c["t3_pre"], c["m3"], c["r3"], pl + "norm3", gl["t3pre"], dy2=dy2, dx2=gl["ff2"],
               drop_mask=dm(f"d3_{l}", H), drop_scale=dsc)
        wgrad(gl["ff2"], c["ff1"], g("linear2.weight"), g("linear2.bias"))
        ops.gemm(GEMM_NN, gl["ff2"], p("linear2.weight"), gl["ff1"], drop_mask=dm(f"ff_{l}", 4 * H), drop_scale=dsc,
                 aux=c["ff1"], mul=1, ws=ws)
        wgrad(gl["ff1"], c["t2"], g("linear1.weight"), g("linear1.bias"))
        ops.gemm(GEMM_NN, gl["ff1"], p("linear1.weight"), gl["t2"], res1=gl["t3pre"], ws=ws)
        ln_bwd(gl["t2"], c["t2_pre"], c["m2"], c["r2"], pl + "norm2", gl["t2pre"], dx2=gl["cap"],
               drop_mask=dm(f"d2_{l}", H), drop_scale=dsc)
        wgrad(gl["cap"], c["ca_o"], g("multihead_attn.out_proj.weight"), g("multihead_attn.out_proj.bias"))
        ops.gemm(GEMM_NN, gl["cap"], p("multihead_attn.out_proj.weight"), gl["cao"], ws=ws)
        attention.backward(w.route, "ca", c, c["caq"], c["cakv"][:, :H], c["cakv"][:, H:], gl["cao"], gl["caq"],
                           gl["cakv"][:, :H], gl["cakv"][:, H:], w.delta, (B, heads, Tq, S, dh), dmf(f"ca_p{l}"), dsc,
                           key_labels=key_labels, pad_idx=eng.pad_idx)
        wi = p("multihead_attn.in_proj_weight")
        gwi, gbi = g("multihead_attn.in_proj_weight"), g("multihead_attn.in_proj_bias")
        wgrad(gl["cakv"], mem, gwi[H:], gbi[H:], b_add=pos, b_add_mod=S)
        wgrad(gl["caq"], c["t1"], gwi[:H], gbi[:H], b_add=qpos, b_add_mod=qmod)
        ops.gemm(GEMM_NN, gl["cakv"], wi[H:], w.d_mp, accumulate=(l != L - 1), ws=ws)         # d (memory + pos)
        ops.gemm(GEMM_NN, gl["caq"], wi[:H], gl["caqin"], ws=ws)                              # d (t1 + query_pos)
        ln_bwd(gl["caqin"], c["t1_pre"], c["m1"], c["r1"], pl + "norm1", gl["t1pre"], dy2=gl["t2pre"], dx2=gl["sap"],
               drop_mask=dm(f"d1_{l}", H), drop_scale=dsc)
        wgrad(gl["sap"], c["sa_o"], g("self_attn.out_proj.weight"), g("self_attn.out_proj.bias"))
        ops.gemm(GEMM_NN, gl["sap"], p("self_attn.out_proj.weight"), gl["sao"], ws=ws)
        attention.backward(w.route, "sa", c, *attention.thirds(c["sa_qkv"]), gl["sao"], *attention.thirds(gl["saqkv"]),
                           w.delta, (B, heads, Tq, Tq, dh), dmf(f"sa_p{l}"), dsc)
        wgrad(gl["saqkv"], tgt_in, g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias"), b_add=qpos, b_add_mod=qmod)
        ops.gemm(GEMM_NN, gl["saqkv"], p("self_attn.in_proj_weight"), gl["sain"], ws=ws)      # d (tgt_in + query_pos)
        # d query_pos += caqin + sain, top layer first
        if g_qpos is not None:            # a parameter: the clips' column sums
            ops.rowmod_sum(gl["caqin"], qmod, g_qpos, accumulate=(l != L - 1))
            ops.rowmod_sum(gl["sain"], qmod, g_qpos, accumulate=True)
        elif l == L - 1:                  # an activation: its gradient flows on into the engine's branch
            ops.add_rowbcast(gl["caqin"], gl["sain"], R, w.d_qpos)
        else:
            ops.add_rowbcast(gl["caqin"], gl["sain"], R, w.d_qtmp)
            ops.add_rowbcast(w.d_qpos, w.d_qtmp, R, w.d_qpos)
        dy, dy2 = gl["sain"], gl["t1pre"]           # d t3 of layer l-1 = through the queries + the residual
    eng.pos_embedding_grad(w)
