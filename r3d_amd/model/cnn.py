"""Drop-in for the reference's ``model/cnn.py``: the CNN baseline of the NTU / UTKinect / DARAI entry scripts (``from
model.cnn import FUTR``), which is the RNN baseline with the recurrence taken out.  Same class name, constructor and
``forward(inputs, mode='train', epoch=0, idx=0)`` signature, same ``state_dict`` keys, shapes and order (the unused
transformer, query_embed, pos_embedding and PositionalEncoding buffer included) and the same construction order, so the same
torch seed yields the same initial weights and reference ``.ckpt`` files load with ``strict=True``.

What it computes (model/cnn.py:66-111): x = relu(input_embed(src)); adaptive average pooling of x to 8 rows; the
anticipation heads on the pooled rows; fc_seg (K - 1 classes) on x; 'supcon' = x.  All arithmetic runs in libr3d_hip.so
through r3d_amd.engine_cnn.CnnEngine; modules here are parameter holders.  The autograd bridge (losses computed by the
caller on the outputs, ``.backward()``, any torch optimiser) runs the engine's composed route.

Outside train mode the reference takes the bare feature tensor (:77); the (features, labels) tuple is accepted too.
"""

import torch
from torch import nn

from ..engine_cnn import CnnEngine
from ._bridge import EngineOwner, arena_grads, logit_grads_in
from .futr_safuser_tokenfusion import _Transformer, _PositionalEncoding


class FUTR(EngineOwner, nn.Module):
    """FUTR(n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
    num_decoder_layers=6, query_num=19) -- model/cnn.py:17-56."""
    _engine_param, _engine_name, _engine_cls = "input_embed.weight", "r3d_amd.model.cnn.FUTR", CnnEngine

    def __init__(self, n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
                 num_decoder_layers=6, query_num=19):
        super().__init__()
        if getattr(args, "input_type", "i3d_transcript") != "i3d_transcript":
            raise NotImplementedError("only input_type='i3d_transcript' is built (the 'gt' embedding branch of "
                                      "model/cnn.py:54-56,87-89 is not on the NTU path)")
        if not (getattr(args, "seg", True) and getattr(args, "anticipate", True)):
            raise NotImplementedError("the fused step implements seg=True and anticipate=True (opts.py defaults)")
        self.src_pad_idx = src_pad_idx
        self.device = device
        self.hidden_dim = hidden_dim
        self.n_class = n_class
        self.n_head = n_head
        self.input_embed = nn.Linear(args.input_dim, hidden_dim)
        self.transformer = _Transformer(hidden_dim, n_head, num_encoder_layers, num_decoder_layers, hidden_dim * 4)
        self.n_query = n_query
        self.args = args
        nn.init.xavier_uniform_(self.input_embed.weight)
        self.query_embed = nn.Embedding(self.n_query, hidden_dim)                                          # :30 (unused)
        self.fc_seg = nn.Linear(hidden_dim, n_class - 1)                                                   # :35
        nn.init.xavier_uniform_(self.fc_seg.weight)
        self.fc = nn.Linear(hidden_dim, n_class)
        nn.init.xavier_uniform_(self.fc.weight)
        self.fc_len = nn.Linear(hidden_dim, 1)
        nn.init.xavier_uniform_(self.fc_len.weight)
        self.pos_embedding = nn.Parameter(torch.zeros(1, args.max_pos_len, hidden_dim))                    # :47 (unused)
        nn.init.xavier_uniform_(self.pos_embedding)
        self.pos_enc = _PositionalEncoding(hidden_dim)                                                      # :50 (unused)

    def forward(self, inputs, mode="train", epoch=0, idx=0):
        if mode == "train":
            src, _ = inputs
        else:
            src = inputs[0] if isinstance(inputs, (tuple, list)) else inputs
        eng = self.engine()
        src = src.to(device=eng.device, dtype=torch.float32).contiguous()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if not need_grad:
            out = eng.forward(src, None, None, mode, training=False, need_grad=False)
            return {k: v.clone() for k, v in out.items()}
        names = [n for n, _ in self.named_parameters()]
        params = [p for _, p in self.named_parameters()]
        dur, act, seg, sup = _Forward.apply(eng, src, mode, names, *params)
        return {"duration": dur, "action": act, "seg": seg, "supcon": sup}


class _Forward(torch.autograd.Function):
    """Bridges the engine into autograd (losses on any of the four outputs, .backward(), any torch optimiser)."""

    @staticmethod
    def forward(ctx, eng, src, mode, names, *params):
        keep, eng.defer_tail = eng.defer_tail, False        # the caller reads the outputs before any loss exists
        try:
            out = eng.forward(src, None, None, mode, training=True, need_grad=True)
        finally:
            eng.defer_tail = keep
        ctx.eng, ctx.names, ctx.token = eng, names, eng.last
        return out["duration"].clone(), out["action"].clone(), out["seg"].clone(), out["supcon"].clone()

    @staticmethod
    def backward(ctx, d_dur, d_act, d_seg, d_sup):
        eng = ctx.eng
        if eng.last is not ctx.token:
            raise RuntimeError("r3d_amd: backward() must follow the forward() it belongs to")
        w, K = eng.last["w"], eng.K
        logit_grads_in(w, K, d_act, d_dur, d_seg)
        eng.backward(d_supcon=None if d_sup is None else d_sup.to(torch.float32))
        return (None,) * 4 + arena_grads(eng, ctx.names)
