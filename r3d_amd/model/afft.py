"""Drop-in for the reference's ``model/afft.py``: the Anticipative Feature Fusion Transformer baseline, the external
method of the paper's comparison table (main_darai.py names it in ``#from model.afft import FUTR``).

Its front is the plain SA-Fuser's, unchanged (afft.py:17-64,158-174 against futr_safuser_depth.py): relu(input_embed),
relu(depth_layernorm(depth_projection)) on 224 x 224 depth maps, the modality token, embd_drop, the one masked two-token
Block, fuser.norm and the token mean.  Behind the fused tokens there is NO decoder (:176-201):

    pooled = adaptive_avg_pool1d(fused, n_query)        [B, Q, H]   padded frames pooled like any other
    action, duration = fc(pooled), fc_len(pooled)       [B, Q, K], [B, Q]

The transformer, query_embed, pos_embedding (sliced at :165, never used), l3_attention, query_attention, fc_l3, fc_seg and
fuser.projection are constructed -- same construction order, state_dict keys and seeded initial values -- and never used:
they receive no gradient and AdamW does not touch them.  There is no 'seg' output (the branch is ``if False:``, :203).

Same class names, constructor and forward signature; the parameters are holders only, the arithmetic runs in
libr3d_hip.so (r3d_amd/engine_afft.py: the plain front's launches + csrc/afft.hip, the pooled-head chain)."""
import torch

from ._bridge import arena_grads, logit_grads_in
from . import futr_safuser_depth as _plain
from . import futr_safuser_tokenfusion as _base


class CMFuser(_plain.CMFuser):
    """SA-Fuser parameter tree of afft.py:17-29: blocks, norm, modality_token, projection (the plain SA-Fuser's)."""


class FUTR(_plain.FUTR):
    """The shared constructor (afft.py:85-121 builds in the same order; fc_seg only with args.seg, :96-98) and forward of
    futr_safuser_tokenfusion.FUTR; the bare-tensor input form of futr_safuser_depth.FUTR (afft.py:146)."""
    _fuser_cls = CMFuser
    _out_names = ("duration", "action")         # nothing else: the 'seg' branch is `if False:` (:203)
    _seg_optional = True

    def __init__(self, n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
                 num_decoder_layers=6, query_num=49, depth_pixels=224 * 224):
        super().__init__(n_class, hidden_dim, src_pad_idx, device, args, n_query, n_head, num_encoder_layers,
                         num_decoder_layers, query_num, depth_pixels)

    @staticmethod
    def _engine_cls():
        from ..engine_afft import AfftEngine
        return AfftEngine

    @staticmethod
    def _autograd_fn():
        return _PooledForward


class _PooledForward(torch.autograd.Function):
    """Bridges the engine into autograd, as futr_safuser_tokenfusion._FusedForward does for the token-fusion model."""

    @staticmethod
    def forward(ctx, eng, src, depth, labels, mode, training, names, *params):
        keep, eng.defer_tail = eng.defer_tail, False        # the caller reads the outputs before any loss exists
        try:
            out = eng.forward(src, depth, labels, mode, training=training, need_grad=True)
        finally:
            eng.defer_tail = keep
        ctx.eng, ctx.names, ctx.token = eng, names, eng.last
        return out["duration"].clone(), out["action"].clone()

    @staticmethod
    def backward(ctx, d_dur, d_act):
        eng = ctx.eng
        if eng.last is not ctx.token:
            raise RuntimeError("r3d_amd: backward() must follow the forward() it belongs to (the engine keeps one "
                               "set of saved activations per shape)")
        w, K = eng.last["w"], eng.K
        logit_grads_in(w, K, d_act, d_dur, None)
        eng.backward(d_actdur=w.d_actdur)
        return (None,) * 7 + arena_grads(eng, ctx.names)
