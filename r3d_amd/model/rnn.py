"""Drop-in for the reference's ``model/rnn.py``: the RNN baseline that ``main_nturgbd.py`` trains (``from model.rnn import
FUTR``).  Same class name, constructor and ``forward(inputs, mode='train', epoch=0, idx=0)`` signature, same ``state_dict``
keys and shapes (the unused transformer, query_embed, pos_embedding and PositionalEncoding buffer included) and the same
construction order -- ``rnn`` first --, so the same torch seed yields the same initial weights and reference ``.ckpt``
files load.

What it computes (model/rnn.py:71-114): x = relu(input_embed(src)); a 2-layer bidirectional LSTM of hidden H/2 per direction
over x (no packing, no masking: padded frames enter the recurrence); rnn_fc; adaptive average pooling to 8 rows; the
anticipation heads on the pooled rows; fc_seg (K - 1 classes) on x; 'supcon' = rnn_fc's output.  All arithmetic runs in
libr3d_hip.so through r3d_amd.engine_rnn.RnnEngine (the recurrence in csrc/lstm.hip); modules here are parameter holders.

The LSTM parameters live in ``_LSTMParams``, which has nn.LSTM's parameter names, order, shapes and initialisation but
is a plain module: nn.LSTM re-points its weights into a MIOpen buffer on ``.to('cuda')`` (flatten_parameters), behind the
engine's arena.  Nothing here calls nn.LSTM or MIOpen.

Outside train mode the reference takes the bare feature tensor (:79); the (features, labels) tuple is accepted too.
"""
import math

import torch
from torch import nn

from ..engine_rnn import RnnEngine
from ._bridge import EngineOwner, arena_grads, logit_grads_in
from .futr_safuser_tokenfusion import _Transformer, _PositionalEncoding


class _LSTMParams(nn.Module):
    """The parameters of nn.LSTM(input_size, hidden_size, num_layers, bidirectional=True, batch_first=True): same names
    (weight_ih_l<k>[_reverse], weight_hh_l<k>[_reverse], bias_ih_l<k>[_reverse], bias_hh_l<k>[_reverse]), same order and
    the same reset_parameters (uniform(-1/sqrt(hidden), 1/sqrt(hidden)) over all of them in that order)."""

    def __init__(self, input_size, hidden_size, num_layers=2):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.bidirectional, self.batch_first, self.dropout = True, True, 0.0
        for layer in range(num_layers):
            for sfx in ("", "_reverse"):
                inp = input_size if layer == 0 else 2 * hidden_size
                setattr(self, f"weight_ih_l{layer}{sfx}", nn.Parameter(torch.empty(4 * hidden_size, inp)))
                setattr(self, f"weight_hh_l{layer}{sfx}", nn.Parameter(torch.empty(4 * hidden_size, hidden_size)))
                setattr(self, f"bias_ih_l{layer}{sfx}", nn.Parameter(torch.empty(4 * hidden_size)))
                setattr(self, f"bias_hh_l{layer}{sfx}", nn.Parameter(torch.empty(4 * hidden_size)))
        stdv = 1.0 / math.sqrt(hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -stdv, stdv)


class FUTR(EngineOwner, nn.Module):
    """FUTR(n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
    num_decoder_layers=6, query_num=19) -- model/rnn.py:17-60."""
    _engine_param, _engine_name, _engine_cls = "input_embed.weight", "r3d_amd.model.rnn.FUTR", RnnEngine

    def __init__(self, n_class, hidden_dim, src_pad_idx, device, args, n_query=8, n_head=8, num_encoder_layers=6,
                 num_decoder_layers=6, query_num=19):
        super().__init__()
        if getattr(args, "input_type", "i3d_transcript") != "i3d_transcript":
            raise NotImplementedError("only input_type='i3d_transcript' is built (the 'gt' embedding branch of "
                                      "model/rnn.py:56-58,85-87 is not on the NTU path)")
        if not (getattr(args, "seg", True) and getattr(args, "anticipate", True)):
            raise NotImplementedError("the fused step implements seg=True and anticipate=True (opts.py defaults)")
        self.rnn = _LSTMParams(hidden_dim, hidden_dim // 2, num_layers=2)                                  # :20-21
        self.rnn_fc = nn.Linear(hidden_dim, hidden_dim)
        self.src_pad_idx = src_pad_idx
        self.device = device
        self.hidden_dim = hidden_dim
        self.n_class = n_class
        self.n_head = n_head
        self.input_embed = nn.Linear(args.input_dim, hidden_dim)
        self.transformer = _Transformer(hidden_dim, n_head, num_encoder_layers, num_decoder_layers, hidden_dim * 4)
        self.n_query = n_query
        self.args = args
        self.r3d_wide_rnn = bool(getattr(args, "wide_rnn", False))         # (opts --wide_rnn: engine_rnn's stepwise route)
        nn.init.xavier_uniform_(self.input_embed.weight)
        self.query_embed = nn.Embedding(self.n_query, hidden_dim)                                          # :31 (unused)
        self.fc_seg = nn.Linear(hidden_dim, n_class - 1)                                                   # :37
        nn.init.xavier_uniform_(self.fc_seg.weight)
        self.fc = nn.Linear(hidden_dim, n_class)
        nn.init.xavier_uniform_(self.fc.weight)
        self.fc_len = nn.Linear(hidden_dim, 1)
        nn.init.xavier_uniform_(self.fc_len.weight)
        self.pos_embedding = nn.Parameter(torch.zeros(1, args.max_pos_len, hidden_dim))                    # :49 (unused)
        nn.init.xavier_uniform_(self.pos_embedding)
        self.pos_enc = _PositionalEncoding(hidden_dim)                                                      # :52 (unused)

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
        out = eng.forward(src, None, None, mode, training=True, need_grad=True)
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
