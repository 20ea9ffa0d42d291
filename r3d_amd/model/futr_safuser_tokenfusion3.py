"""Build-defined THREE-modality (RGB + depth + gaze) token-fusion model (BASELINE.json configs[4]: "Synthetic 3-modality
(RGB+Depth+Gaze) fusion") -- **build-defined, parity unpinned**: the reference has no three-modality model (its CMFuser is
two-token, model/futr_safuser_tokenfusion.py:74-81), so no reference output exists for it.  It is checked against the build's
own float64 restatement (tests/m3_oracle.py), which is composed of pieces the reference fixtures pin.

It is the two-modality ``futr_safuser_tokenfusion.FUTR`` with three differences:

  construction   the two-modality model's modules in that model's order (``fuser`` is a ``cmfuser3.CMFuser3``: the reference
                 CMFuser's parameter names and initialisation order), THEN ``gaze_projection = nn.Linear(gaze_dim, hidden)``
                 (xavier_uniform_ weight) and ``gaze_layernorm = nn.LayerNorm(hidden)``.  For one seed every shared parameter
                 has the two-modality model's initial value; the state_dict is that model's keys plus four; a two-modality
                 checkpoint loads with strict=False, missing exactly gaze_projection.{weight,bias} and
                 gaze_layernorm.{weight,bias}.
  forward        ``forward(inputs, depth_features, gaze, mode='train', epoch=0, idx=0)`` with gaze [B, S, gaze_dim] float32
                 (the reference's data/basedataset_darai_gaze.py produces [S, 2] tracks per clip).  The gaze embedding mirrors
                 the depth branch (futr_safuser_tokenfusion.py:194-197): gz = relu(gaze_layernorm(gaze_projection(gaze))).
  fusion         ``fuser({'rgb': src, 'depth': depth_inputs, 'gaze': gz}, mode)`` with CMFuser3's semantics unchanged: cyclic
                 exchange (m takes from (m + 1) mod 3), the constant-score tie rule in train mode and mean |x| scores
                 otherwise, three-token attention with a -inf diagonal, the triple mean.

Everything behind ``fused_features`` -- pos_embedding, query_embed, the decoder with the key padding mask in train mode only,
fc / fc_len / fc_seg and the three losses -- is the two-modality model's path.  Live and dead parameters are that model's,
plus the four gaze tensors (live).  Dead parameters get no gradient and no AdamW update, weight decay included.

The modules below are parameter holders; all arithmetic runs in HIP through r3d_amd.engine_m3.M3Engine (no CPU path).
"""
import torch
from torch import nn

from ._bridge import arena_grads, logit_grads_in
from .cmfuser3 import CMFuser3
from .futr_safuser_tokenfusion import FUTR as _FUTR2


class FUTR(_FUTR2):
    """FUTR(n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
    num_decoder_layers=6, query_num=49, depth_pixels=224*224, gaze_dim=2)"""

    _fuser_cls = CMFuser3

    @staticmethod
    def _engine_cls():
        from ..engine_m3 import M3Engine
        return M3Engine

    @staticmethod
    def _autograd_fn():
        return _FusedForward3

    def __init__(self, n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
                 num_decoder_layers=6, query_num=49, depth_pixels=224 * 224, gaze_dim=2):
        super().__init__(n_class, hidden_dim, src_pad_idx, device, args, n_query=n_query, n_head=n_head,
                         num_encoder_layers=num_encoder_layers, num_decoder_layers=num_decoder_layers, query_num=query_num,
                         depth_pixels=depth_pixels)
        self.gaze_dim = int(gaze_dim)
        self.gaze_projection = nn.Linear(self.gaze_dim, hidden_dim)
        nn.init.xavier_uniform_(self.gaze_projection.weight)
        self.gaze_layernorm = nn.LayerNorm(hidden_dim)

    def forward(self, inputs, depth_features, gaze, mode="train", epoch=0, idx=0):
        src, src_label = inputs
        eng = self.engine()
        src = src.to(device=eng.device, dtype=torch.float32)
        depth_features = depth_features.to(device=eng.device, dtype=torch.float32)
        gaze = gaze.to(device=eng.device, dtype=torch.float32).contiguous()
        if mode == "train":
            src_label = src_label.to(device=eng.device).long().contiguous()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if not need_grad:
            out = eng.forward(src, depth_features, src_label, mode, training=False, need_grad=False, gaze=gaze)
            return {k: v.clone() for k, v in out.items()}
        names = [n for n, _ in self.named_parameters()]
        params = [p for _, p in self.named_parameters()]
        outs = _FusedForward3.apply(eng, src, depth_features, gaze, src_label, mode, self.training, names, *params)
        return dict(zip(self._out_names, outs))


class _FusedForward3(torch.autograd.Function):
    """The engine inside autograd, as futr_safuser_tokenfusion._FusedForward: loss on the outputs, loss.backward(), any
    torch optimiser."""

    @staticmethod
    def forward(ctx, eng, src, depth, gaze, labels, mode, training, names, *params):
        out = eng.forward(src, depth, labels, mode, training=training, need_grad=True, gaze=gaze)
        ctx.eng, ctx.names, ctx.token = eng, names, eng.last
        return out["duration"].clone(), out["action"].clone(), out["seg"].clone()

    @staticmethod
    def backward(ctx, d_dur, d_act, d_seg):
        eng = ctx.eng
        if eng.last is not ctx.token:
            raise RuntimeError("r3d_amd: backward() must follow the forward() it belongs to (the engine keeps one "
                               "set of saved activations per shape)")
        w, K = eng.last["w"], eng.K
        logit_grads_in(w, K, d_act, d_dur, d_seg)
        eng.backward()
        return (None,) * 8 + arena_grads(eng, ctx.names)
