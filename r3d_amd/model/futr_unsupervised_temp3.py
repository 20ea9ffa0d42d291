"""Drop-in for the reference's ``model/futr_unsupervised_temp3.py`` (the L3 query model, the one file of that family whose
outputs train_unsupervised.py's loop accepts): same class name, constructor and ``forward(inputs, query, mode='train',
epoch=0, idx=0)`` signature, same ``state_dict`` keys / shapes and construction order (same seed -> same initial weights).

What it computes (futr_unsupervised_temp3.py:72-143): memory = pos_enc(relu(input_embed(x))); `l3_attention` over the CLIPS of
each frame (it is called after 'b t c -> t b c', so its sequence is the batch) + a sinusoidal table = l3;
adaptive_avg_pool1d(l3, n_query) is the decoder's per-clip query; the DETR decoder with the encoder bypassed; heads fc / fc_len
on the n_query decoder rows, fc_seg (n_class outputs) on the memory, fc_l3 on l3.  `query` is accepted and unused, as in the
reference.  transformer.encoder.* and query_attention.* are constructed (state_dict parity) and never used.

The arithmetic runs in libr3d_hip.so through r3d_amd.engine_l3.L3Engine; modules here are parameter holders.
r3d_amd.train_unsupervised.train() drives the engine's fused step; any other torch loss on the outputs goes through autograd."""
import math

import torch
from torch import nn

from ..engine_l3 import L3Engine
from ._bridge import EngineOwner, arena_grads, logit_grads_in
from .futr_safuser_tokenfusion import _Transformer, _PositionalEncoding


class FUTR(EngineOwner, nn.Module):
    """FUTR(n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
    num_decoder_layers=6, query_num=49) -- model/futr_unsupervised_temp3.py:20-60."""
    _engine_param, _engine_cls = "input_embed.weight", L3Engine

    def __init__(self, n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
                 num_decoder_layers=6, query_num=49):
        super().__init__()
        self.src_pad_idx = src_pad_idx
        self.query_pad_idx = query_num - 1
        self.device = device
        self.hidden_dim = hidden_dim
        self.n_class = n_class
        self.n_head = n_head
        self.num_decoder_layers = num_decoder_layers
        self.n_query = n_query
        self.args = args
        if getattr(args, "input_type", "i3d_transcript") != "i3d_transcript":
            raise NotImplementedError("only input_type='i3d_transcript' is built (futr_unsupervised_temp3.py:58-60,88-90: 'gt' embedding)")
        if not (getattr(args, "seg", True) and getattr(args, "anticipate", True)):
            raise NotImplementedError("seg=True and anticipate=True (opts.py:100-101 defaults) are implemented")
        if num_decoder_layers < 1:
            raise ValueError("num_decoder_layers must be >= 1")
        self.input_embed = nn.Linear(args.input_dim, hidden_dim)                                            # :28
        self.transformer = _Transformer(hidden_dim, n_head, num_encoder_layers, num_decoder_layers, hidden_dim * 4)
        nn.init.xavier_uniform_(self.input_embed.weight)
        self.l3_attention = nn.MultiheadAttention(hidden_dim, n_head, batch_first=True)                     # :34
        self.query_attention = nn.MultiheadAttention(hidden_dim, n_head, batch_first=True)                  # :35 (unused)
        self.fc_seg = nn.Linear(hidden_dim, n_class)                                                        # :39
        nn.init.xavier_uniform_(self.fc_seg.weight)
        self.fc = nn.Linear(hidden_dim, n_class)
        nn.init.xavier_uniform_(self.fc.weight)
        self.fc_len = nn.Linear(hidden_dim, 1)
        nn.init.xavier_uniform_(self.fc_len.weight)
        self.fc_l3 = nn.Linear(hidden_dim, query_num)                                                       # :48
        self.pos_embedding = nn.Parameter(torch.zeros(1, args.max_pos_len, hidden_dim))
        nn.init.xavier_uniform_(self.pos_embedding)
        self.pos_enc = _PositionalEncoding(hidden_dim)                                                      # :54
        # plain tensor attribute, not a buffer (:55-56): not in the state_dict
        position = torch.arange(args.max_pos_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, hidden_dim, 2) * -(math.log(10000.0) / hidden_dim))
        pe = torch.zeros(args.max_pos_len, hidden_dim)
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.positional_embedding_l3 = pe

    def forward(self, inputs, query, mode="train", epoch=0, idx=0):
        if mode == "train":
            src, src_label = inputs
        else:                                    # the bare feature tensor, no masks (:78-82)
            src, src_label = (inputs[0], None) if isinstance(inputs, (tuple, list)) else (inputs, None)
        eng = self.engine()
        src = src.to(device=eng.device, dtype=torch.float32).contiguous()
        if mode == "train":
            src_label = src_label.to(device=eng.device).long().contiguous()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if not need_grad:
            out = eng.forward(src, src_label, mode, training=False, need_grad=False)
            return {k: v.clone() for k, v in out.items()}
        names = [n for n, _ in self.named_parameters()]
        params = [p for _, p in self.named_parameters()]
        dur, act, seg, l3 = _Forward.apply(eng, src, src_label, mode, self.training, names, *params)
        return {"duration": dur, "action": act, "seg": seg, "l3": l3}


class _Forward(torch.autograd.Function):
    """Bridges the engine into autograd (losses on the outputs, losses.backward(), any torch optimiser)."""

    @staticmethod
    def forward(ctx, eng, src, labels, mode, training, names, *params):
        out = eng.forward(src, labels, mode, training=training, need_grad=True)
        ctx.eng, ctx.names, ctx.token = eng, names, eng.last
        return out["duration"].clone(), out["action"].clone(), out["seg"].clone(), out["l3"].clone()

    @staticmethod
    def backward(ctx, d_dur, d_act, d_seg, d_l3):
        eng = ctx.eng
        if eng.last is not ctx.token:
            raise RuntimeError("r3d_amd: backward() must follow the forward() it belongs to")
        w, K = eng.last["w"], eng.K
        logit_grads_in(w, K, d_act, d_dur, d_seg)
        if d_l3 is None:
            w.d_l3log.zero_()
        else:
            w.d_l3log.copy_(d_l3.reshape(w.d_l3log.shape))
        eng.backward()
        return (None,) * 6 + arena_grads(eng, ctx.names)
