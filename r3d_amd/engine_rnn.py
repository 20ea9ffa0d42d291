"""Host-side sequencing of the RNN baseline (reference model/rnn.py, the model main_nturgbd.py trains) on one MI355X.

    x      = relu(input_embed(src))                      [B*S, H]     (no positional encoding, no dropout: :90-92)
    y0, y1 = 2-layer bidirectional LSTM(x)               [B*S, H]     (nn.LSTM(H, H/2, 2, bidirectional), :20,93)
    tgt    = rnn_fc(y1)                                  [B*S, H]     (:95; also returned as 'supcon', :113)
    pooled = adaptive_avg_pool1d(tgt, 8)                 [B*8, H]     (:97 -- 8 is hard-coded, not n_query)
    action, duration = fc(pooled), fc_len(pooled)                     (:101-105)
    seg    = fc_seg(x)                                   [B*S, K - 1] (:110, on the embedding, not on the LSTM output)

Same flat arenas, C ABI and method surface (forward / losses / backward / adamw / train_step) as engine.FusionEngine, so
the graphed steps of train_proposed_depth drive it.  Per layer the input projection of both directions is ONE GEMM (the
arena keeps weight_ih_l<k> and weight_ih_l<k>_reverse adjacent, likewise bias_ih), the recurrence is ONE launch of
csrc/lstm.hip (both directions), and the backward's dW_ih / dX are one GEMM each, dW_hh (+ d b_hh) one per direction.
Past hidden 256 (opts --wide_rnn) the recurrence is csrc/lstm_steps.hip instead: one launch per time step, W_hh spread over
the chip, the same tensors in the same layouts, so everything around it is unchanged (lstm_route picks the kernels).
"""
import torch

from . import ops
from ._lib import GEMM_NT, GEMM_NN, GEMM_TN
from .engine_base import EngineBase

EXCLUDE_CLASS_IDX = 120         # NTU's UNDEFINED class, hard-coded at train/train_unimodal.py:102,198,212
POOL_ROWS = 8                   # F.adaptive_avg_pool1d(tgt, 8) (model/rnn.py:97)
RNN_MIN_H, RNN_MAX_H = 8, 256   # the recurrence kernels' range (csrc/lstm.hip: W_hh of one direction in registers)
RNN_WIDE_MAX_H = 1024           # with --wide_rnn: the stepwise recurrence (csrc/lstm_steps.hip: one launch per time step)
SUPCON_MAX_H = 256              # the supervised contrastive kernel's column limit (csrc/supcon.hip)
SUPCON_WIDE_MAX_H = 2048        # with --wide_supcon: its wide route's, past every hidden size this model admits

SUPCON_BASE_T = 0.07            # SupConLoss's default base_temperature (loss/spc.py:69); the entry scripts pass temperature only

RNN_LIVE_PREFIXES = ("input_embed.", "rnn.", "rnn_fc.", "fc_seg.", "fc.", "fc_len.")


def is_live(name):
    return name.startswith(RNN_LIVE_PREFIXES)


def lstm_route(H, wide):
    """Which recurrence kernels run hidden H: "registers" (csrc/lstm.hip) wherever they take H, whatever the flag, so a run
    at hidden <= 256 launches the same kernels with or without --wide_rnn; "steps" (csrc/lstm_steps.hip) for wider H with the
    flag; None (refused) otherwise."""
    if ops.lstm_supported(H):
        return "registers"
    if wide and ops.lstm_steps_supported(H):
        return "steps"
    return None


def check_rnn_shape(H, n_query=POOL_ROWS, erank_weight=0.0, wide=False, supcon_weight=0.0, wide_supcon=False):
    """Raises ValueError unless the engine runs this model: hidden H in the recurrence kernels' range (up to RNN_WIDE_MAX_H
    with wide, opts --wide_rnn), n_query == 8 (the reference pools to 8 rows whatever n_query is, so its targets of n_query
    rows would not match the 8 outputs), no effective-rank penalty (defined on a fuser's token matrix; this model has none)
    and no supervised contrastive term past its kernel's width (256 columns; with wide_supcon, opts --wide_supcon, the
    kernel's wide route takes every hidden size the model itself admits).  Host-only, nothing is enqueued."""
    if wide:
        if not (RNN_MIN_H <= H <= RNN_WIDE_MAX_H) or H % 8:
            raise ValueError(f"hidden {H}: with --wide_rnn the LSTM recurrence kernels take {RNN_MIN_H} <= hidden <= "
                             f"{RNN_WIDE_MAX_H} with hidden % 8 == 0")
    elif not (RNN_MIN_H <= H <= RNN_MAX_H) or H % 8:
        hint = ""
        if RNN_MAX_H < H <= RNN_WIDE_MAX_H and H % 8 == 0:
            hint = "; the stepwise recurrence runs this hidden size: --wide_rnn"
        raise ValueError(f"hidden {H}: the LSTM recurrence kernels take {RNN_MIN_H} <= hidden <= {RNN_MAX_H} with hidden % 8 "
                         f"== 0 (W_hh of one direction, 2 hidden x hidden / 2 floats, is held in registers){hint}")
    if n_query != POOL_ROWS:
        raise ValueError(f"n_query {n_query}: the RNN model pools to {POOL_ROWS} rows (model/rnn.py:97), so its anticipation "
                         f"outputs only match targets of n_query == {POOL_ROWS} rows")
    if erank_weight:
        raise ValueError(f"erank_weight {erank_weight}: the effective-rank penalty needs a fuser's token matrix; the RNN "
                         f"model has none")
    if supcon_weight and H > (SUPCON_WIDE_MAX_H if wide_supcon else SUPCON_MAX_H):
        raise ValueError(f"supcon_weight {supcon_weight} at hidden {H}: the supervised contrastive kernel takes rows of at "
                         f"most {SUPCON_MAX_H} columns (csrc/supcon.hip), so --supcon_weight needs hidden <= {SUPCON_MAX_H}, "
                         f"or --wide_supcon (its wide route: rows of at most {SUPCON_WIDE_MAX_H} columns)")


def _arena_order(named):
    """named_parameters with each layer's two W_ih (and two b_ih) next to each other: [fwd; rev] is then one [4H, H] GEMM
    operand (the arena keeps the relative order of equally aligned parameters)."""
    out, seen = [], set()
    byname = dict(named)
    for n, p in named:
        if n in seen:
            continue
        out.append((n, p))
        seen.add(n)
        if n.startswith(("rnn.weight_ih_l", "rnn.bias_ih_l")) and not n.endswith("_reverse"):
            r = n + "_reverse"
            out.append((r, byname[r]))
            seen.add(r)
    return out


class _Shape:
    def __init__(self, eng, B, S, train):
        dev, H, K = eng.device, eng.H, eng.K
        N, BQ = B * S, B * POOL_ROWS
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)     # noqa: E731
        self.B, self.S, self.N, self.BQ = B, S, N, BQ
        self.x, self.gin = f(N, H), f(N, 4 * H)
        self.y = [f(N, H), f(N, H)]
        self.gates = [f(N, 4 * H), f(N, 4 * H)]
        self.cell = [f(N, H), f(N, H)]
        self.hprev = [f(N, H), f(N, H)]
        self.tgt, self.pooled = f(N, H), f(BQ, H)
        self.actdur = f(BQ, K + 1)
        self.seg = f(N, eng.Kseg)
        self.loss = f(4)
        self.loss_ws = torch.zeros(ops.losses_ws_floats(B, S, POOL_ROWS), dtype=torch.float32, device=dev)
        self.counts = torch.zeros(4, dtype=torch.int64, device=dev)
        if train:
            self.d_actdur, self.d_seg = torch.zeros(BQ, K + 1, dtype=torch.float32, device=dev), f(N, eng.Kseg)
            self.d_pooled, self.d_tgt = f(BQ, H), f(N, H)
            self.d_y = [f(N, H), f(N, H)]
            self.dg = f(N, 4 * H)
            self.d_x0, self.d_x, self.d_pre = f(N, H), f(N, H), f(N, H)
            self.sc_ws = f(ops.supcon_ws_floats(N, H, True, wide=eng.wide_supcon))
            self.sc_loss = torch.zeros(1, dtype=torch.float32, device=dev)
            if eng.steps:               # the stepwise backward's dc carry and transposed W_hh
                self.lstm_ws = f(ops.lstm_steps_ws_floats(B, H))


class RnnEngine(EngineBase):
    _Shape = _Shape
    use_lstm_steps = None           # None: routed by lstm_route(); True: the stepwise kernels at any admitted hidden size
    wide_supcon = False             # --wide_supcon: the contrastive term runs the kernel's wide route (hidden > 256); set before
                                    # supcon_weight and before the first training step (the step's workspace is sized by it)

    def __init__(self, module, device):
        self.wide = bool(getattr(module, "r3d_wide_rnn", False))    # (opts --wide_rnn)
        check_rnn_shape(module.hidden_dim, module.n_query, wide=self.wide)     # (before anything is enqueued)
        self.H, self.Q, self.K = module.hidden_dim, POOL_ROWS, module.n_class
        self._init_engine(module, device, is_live, _arena_order(list(module.named_parameters())))
        self.Kseg = module.fc_seg.out_features
        self.D = module.input_embed.in_features
        self.pad_idx = module.src_pad_idx
        self._supcon_weight = 0.0           # --supcon_weight: total loss += weight * SupConLoss over the 'supcon' rows
        self.supcon_temperature = 0.07      # --temperature
        a, H = self.arena, self.H
        # per layer: [W_ih fwd; W_ih rev] as one [4H, H] operand, [b_ih fwd; b_ih rev] as one [4H] bias
        self.w_ih, self.gw_ih, self.b_ih, self.gb_ih = [], [], [], []
        for l in range(2):
            ow, ob = a.offsets[f"rnn.weight_ih_l{l}"][0], a.offsets[f"rnn.bias_ih_l{l}"][0]
            assert a.offsets[f"rnn.weight_ih_l{l}_reverse"][0] == ow + 2 * H * H
            assert a.offsets[f"rnn.bias_ih_l{l}_reverse"][0] == ob + 2 * H
            self.w_ih.append(a.params[ow:ow + 4 * H * H].view(4 * H, H))
            self.gw_ih.append(a.grads[ow:ow + 4 * H * H].view(4 * H, H))
            self.b_ih.append(a.params[ob:ob + 4 * H])
            self.gb_ih.append(a.grads[ob:ob + 4 * H])

    @property
    def supcon_weight(self):
        return self._supcon_weight

    @supcon_weight.setter
    def supcon_weight(self, v):
        check_rnn_shape(self.H, self.Q, wide=self.wide, supcon_weight=v, wide_supcon=self.wide_supcon)
        self._supcon_weight = v

    @property
    def steps(self):
        """Whether the LSTM layers run the stepwise kernels (csrc/lstm_steps.hip)."""
        if self.use_lstm_steps:
            if not ops.lstm_steps_supported(self.H):
                raise ValueError(f"hidden {self.H}: the stepwise recurrence does not take it")
            return True
        return lstm_route(self.H, self.wide) == "steps"

    def _whh(self, l, grad=False):
        f = self.arena.g if grad else self.arena.p
        return f(f"rnn.weight_hh_l{l}"), f(f"rnn.weight_hh_l{l}_reverse")

    def _bhh(self, l, grad=False):
        f = self.arena.g if grad else self.arena.p
        return f(f"rnn.bias_hh_l{l}"), f(f"rnn.bias_hh_l{l}_reverse")

    # ------------------------------------------------------------------------------------------------------
    def forward(self, feats, depth=None, labels=None, mode="train", training=False, need_grad=True):
        """feats [B,S,D] f32.  depth / labels: accepted for FusionEngine's signature and never read (the model has no
        depth input and no key padding mask).  Returns views: seg [B,S,K-1], action [B,8,K], duration [B,8], supcon [B,S,H]."""
        a, H, K = self.arena, self.H, self.K
        assert feats.is_cuda and feats.dtype == torch.float32
        B, S = feats.shape[0], feats.shape[1]
        N = B * S
        x_rgb = feats.reshape(N, -1)
        assert x_rgb.shape[1] == self.D and x_rgb.is_contiguous()
        w = self._shape(B, S, need_grad)
        ws = self.ws
        ops.gemm(GEMM_NT, x_rgb, a.p("input_embed.weight"), w.x, bias=a.p("input_embed.bias"), act=1, ws=ws)
        ops.gemm(GEMM_NT, w.x, a.p("fc_seg.weight"), w.seg, bias=a.p("fc_seg.bias"), ws=ws)
        inp = w.x
        for l in range(2):
            ops.gemm(GEMM_NT, inp, self.w_ih[l], w.gin, bias=self.b_ih[l], ws=ws)
            lstm_fwd = ops.lstm_steps_layer_fwd if self.steps else ops.lstm_layer_fwd
            lstm_fwd(w.gin, *self._whh(l), *self._bhh(l), w.y[l], w.gates[l], w.cell[l], w.hprev[l], B, S)
            inp = w.y[l]
        ops.gemm(GEMM_NT, w.y[1], a.p("rnn_fc.weight"), w.tgt, bias=a.p("rnn_fc.bias"), ws=ws)
        ops.avgpool_rows_fwd(w.tgt, w.pooled, B, S, POOL_ROWS)
        ops.gemm(GEMM_NT, w.pooled, self.w_head, w.actdur, bias=self.b_head, ws=ws)
        self.last = dict(w=w, x_rgb=x_rgb, drop=False, mode=mode, tp=None)
        return dict(seg=w.seg.view(B, S, self.Kseg), action=w.actdur[:, :K].view(B, POOL_ROWS, K),
                    duration=w.actdur[:, K].view(B, POOL_ROWS), supcon=w.tgt.view(B, S, H))

    # ------------------------------------------------------------------------------------------------------
    def _supcon_kw(self):
        return dict(temperature=self.supcon_temperature, base_temperature=SUPCON_BASE_T, ignore_index=self.pad_idx,
                    normalize=True, wide=self.wide_supcon)

    def losses(self, past_label, target, target_dur, with_grad=True, val_mode=False, tick=False):
        """The 3 losses + counters of train_unimodal.py:188-225 (exclude index 120) in one launch; fills d_seg / d_actdur.
        With supcon_weight > 0 (training only) the supervised contrastive loss of the L2-normalised 'supcon' rows over the
        per-frame labels, padded frames ignored, follows: w.sc_loss holds it and loss[3] gains weight times it."""
        w, K = self.last["w"], self.K
        ops.losses_fwd_bwd_kseg(None if val_mode else w.seg, w.actdur[:, :K], w.actdur[:, K:], K + 1, past_label, target,
                                target_dur, w.B, w.S, POOL_ROWS, K, self.Kseg, self.pad_idx, EXCLUDE_CLASS_IDX, w.loss,
                                w.counts, val_mode=val_mode, dur_den=self.dur_den,
                                d_seg=w.d_seg if with_grad else None, d_act=w.d_actdur[:, :K] if with_grad else None,
                                d_dur=w.d_actdur[:, K:] if with_grad else None, ld_ddur=K + 1, ws=w.loss_ws,
                                tick_a=self.step_t if tick else None)
        if self.supcon_weight and with_grad and not val_mode:
            lab = past_label.reshape(-1)
            ops.supcon_fwd(w.tgt, lab, w.N, w.N, w.sc_ws, w.sc_loss, **self._supcon_kw())
            w.loss[3:4].add_(w.sc_loss, alpha=self.supcon_weight)
            self.last["supcon_labels"] = lab
        return w.loss, w.counts

    # ------------------------------------------------------------------------------------------------------
    def backward(self, d_seg=None, d_actdur=None, fused_adamw=None, adamw_next=False, d_supcon=None):
        """Adjoint of forward(); gradients land in the grad arena (written, not accumulated).  d_supcon (optional
        [B,S,H]): a gradient on the 'supcon' output, added to rnn_fc's output gradient.  After losses() with supcon_weight
        > 0 the contrastive term's gradient is added straight into it by its own kernel."""
        assert fused_adamw is None
        st = self.last
        w, a, H, ws = st["w"], self.arena, self.H, self.ws
        B, S, N = w.B, w.S, w.N
        if d_seg is not None and d_seg.data_ptr() != w.d_seg.data_ptr():
            w.d_seg.copy_(d_seg)
        if d_actdur is not None and d_actdur.data_ptr() != w.d_actdur.data_ptr():
            w.d_actdur.copy_(d_actdur)

        def wgrad(dy, x, gw, gb, **kw):
            ops.gemm(GEMM_TN, dy, x, gw, bias_grad=gb, ws=ws, **kw)

        # ---- heads, pooling, rnn_fc
        wgrad(w.d_actdur, w.pooled, self.gw_head, self.gb_head)
        ops.gemm(GEMM_NN, w.d_actdur, self.w_head, w.d_pooled, ws=ws)
        ops.avgpool_rows_bwd(w.d_pooled, w.d_tgt, B, S, POOL_ROWS)
        if d_supcon is not None:
            ops.add_rowbcast(w.d_tgt, d_supcon.reshape(N, H).contiguous(), N, w.d_tgt)
        if st.get("supcon_labels") is not None:
            ops.supcon_bwd(w.tgt, st["supcon_labels"], N, N, w.sc_ws, w.d_tgt, gscale=self.supcon_weight, add=True,
                           **self._supcon_kw())
        wgrad(w.d_tgt, w.y[1], a.g("rnn_fc.weight"), a.g("rnn_fc.bias"))
        ops.gemm(GEMM_NN, w.d_tgt, a.p("rnn_fc.weight"), w.d_y[1], ws=ws)
        # ---- the two LSTM layers, top down
        h = H // 2
        for l in (1, 0):
            if self.steps:
                ops.lstm_steps_layer_bwd(w.d_y[l], *self._whh(l), w.gates[l], w.cell[l], w.dg, B, S, w.lstm_ws)
            else:
                ops.lstm_layer_bwd(w.d_y[l], *self._whh(l), w.gates[l], w.cell[l], w.dg, B, S)
            inp = w.x if l == 0 else w.y[0]
            wgrad(w.dg, inp, self.gw_ih[l], self.gb_ih[l])                     # dW_ih, d b_ih of both directions
            for d, (gw, gb) in enumerate(zip(self._whh(l, grad=True), self._bhh(l, grad=True))):
                wgrad(w.dg[:, 2 * H * d:2 * H * (d + 1)], w.hprev[l][:, h * d:h * (d + 1)], gw, gb)   # dW_hh, d b_hh
            ops.gemm(GEMM_NN, w.dg, self.w_ih[l], w.d_x0 if l == 0 else w.d_y[0], ws=ws)       # dX, summed over directions
        # ---- segmentation head on the embedding, then through the ReLU into input_embed
        wgrad(w.d_seg, w.x, a.g("fc_seg.weight"), a.g("fc_seg.bias"))
        ops.gemm(GEMM_NN, w.d_seg, a.p("fc_seg.weight"), w.d_x, res1=w.d_x0, ws=ws)
        ops.posenc_bwd(w.d_x, w.d_pre, gate=w.x)
        wgrad(w.d_pre, st["x_rgb"], a.g("input_embed.weight"), a.g("input_embed.bias"))

    # ------------------------------------------------------------------------------------------------------
    def _tick_counter(self, tick_dropout):
        return None                         # (no dropout: nothing beside the step counter to advance)

    def train_step(self, feats, depth, past_label, target_dur, target, lr, weight_decay, training=True):
        """forward + losses + backward + AdamW, all enqueued, no host sync.  Returns (loss[4], counts[4]) on device.
        depth: accepted for FusionEngine's signature, never read (may be None)."""
        self.forward(feats, None, past_label, "train", training)
        loss, counts = self.losses(past_label, target, target_dur, tick=True)
        self.backward()
        self.adamw(lr, weight_decay, ticked=True)
        return loss, counts
