"""Host-side sequencing of the CNN baseline (reference model/cnn.py: the RNN model with the recurrence taken out) on one
MI355X.

    x      = relu(input_embed(src))                      [B*S, H]     (no positional encoding, no dropout: cnn.py:88-90)
    pooled = adaptive_avg_pool1d(x, 8)                   [B*8, H]     (:94 -- 8 is hard-coded, not n_query)
    action, duration = fc(pooled), fc_len(pooled)                     (:98-102)
    seg    = fc_seg(x)                                   [B*S, K - 1] (:107)
    'supcon' = x                                                      (:110)

Same flat arena, C ABI and method surface (forward / losses / backward / adamw / train_step) as engine_rnn.RnnEngine, so
train_unimodal's graphed steps drive it.  8 parameters are live (input_embed, fc_seg, fc, fc_len); everything else the
reference constructs (transformer, query_embed, pos_embedding) gets no gradient and AdamW does not touch it, weight decay
included.

Two routes, both kept:

  composed   RnnEngine's launches with the LSTM and rnn_fc left out: embedding GEMM with ReLU, fc_seg GEMM,
             avgpool_rows_fwd, head GEMM, losses_fwd_bwd_kseg and their adjoints.  Every admitted shape; also what the
             autograd bridge (model/cnn.py) uses, where the caller computes its own loss on the outputs.
  chain      where r3d_cnn_seg_supported and r3d_afft_head_supported both say yes and chain_pays(): embedding GEMM,
             r3d_afft_head_step on x (pool, heads, anticipation and duration units, d_x0; it zeroes the segmentation units
             of the loss partials and ticks the step counter, so it goes first), r3d_cnn_seg_step (csrc/cnn.hip: logits,
             segmentation units, d_seg, d_seg . W + d_x0 + d_extra through the ReLU gate), the three weight gradients, AdamW
             with the loss reduction riding in it (has_seg = 1).

The chain needs forward -> losses -> backward back to back: with defer_tail (the engine's default; the autograd bridge
clears it) a training forward() is the embedding GEMM alone and its outputs are valid after losses().  With
losses(tick=True) on the chain the loss statistics are reduced by the AdamW launch: loss / counts are valid after adamw()."""
import torch

from . import ops
from ._lib import GEMM_NT, GEMM_NN, GEMM_TN
from .engine_base import EngineBase

EXCLUDE_CLASS_IDX = 120         # NTU's UNDEFINED class, hard-coded at train/train_unimodal.py:102,198,212
POOL_ROWS = 8                   # F.adaptive_avg_pool1d(tgt, 8) (model/cnn.py:94)
CNN_MIN_H, CNN_MAX_H = 8, 1024  # the pooled-head chain's widest hidden (csrc/afft.hip); the GEMMs take any
CNN_MAX_CLASSES = 1023          # n_class + 1 head outputs <= 1024 (csrc/afft.hip), n_class - 1 <= 1023 seg classes (csrc/cnn.hip)
SEG_CHAIN_MAX_H = 256           # csrc/cnn.hip: the widest tile of tile_mma.h

SUPCON_BASE_T = 0.07            # SupConLoss's default base_temperature (loss/spc.py:69)

CNN_LIVE_PREFIXES = ("input_embed.", "fc_seg.", "fc.", "fc_len.")


CHAIN_MIN_ROWS = 8 * 1142        # the smallest measured B * S at which the chain route was ahead


def chain_pays(B, S, H, Kseg):
    """True where the training step runs the chain route (r3d_afft_head_step + r3d_cnn_seg_step), False: the composed
    launches.  Measured on one MI355X at hidden 128, 122 classes (tools/cnn_step_speed.py, profiles/cnn_step_speed.json),
    the whole graphed step, medians of 7 alternating rounds, chain against composed: 0.134 ms against 0.093 at (B, S) =
    (8, 16), 0.435 against 0.411 at (16, 256), 1.069 against 1.089 at (8, 1142).  The chain loses on short batches -- two
    workgroups of the row-tile kernel are a longer serial path than the composed launches they replace -- and is 1.8 %
    ahead at 9136 rows, so it is taken from that many rows on and the composed launches below (the crossing between 4096
    and 9136 rows was not located).  Other hidden sizes and class counts were not timed and follow the same rule."""
    return B * S >= CHAIN_MIN_ROWS


def is_live(name):
    return name.startswith(CNN_LIVE_PREFIXES)


def check_cnn_shape(H, n_query=POOL_ROWS, n_class=2, erank_weight=0.0, B=1, S=1, input_dim=1):
    """Raises ValueError naming the limit unless the engine runs this model.  Host-only, nothing is enqueued."""
    if not (CNN_MIN_H <= H <= CNN_MAX_H) or H % 8:
        raise ValueError(f"hidden {H}: the CNN baseline takes {CNN_MIN_H} <= hidden <= {CNN_MAX_H} with hidden % 8 == 0 (the "
                         f"pooled-head kernels hold a head weight row of at most {CNN_MAX_H} floats in one wave's registers)")
    if n_query != POOL_ROWS:
        raise ValueError(f"n_query {n_query}: the CNN model pools to {POOL_ROWS} rows (model/cnn.py:94), so its anticipation "
                         f"outputs only match targets of n_query == {POOL_ROWS} rows")
    if not 2 <= n_class <= CNN_MAX_CLASSES:
        raise ValueError(f"n_class {n_class}: the CNN baseline takes 2 <= n_class <= {CNN_MAX_CLASSES} (fc_seg has n_class - 1 "
                         f"outputs, the pooled-head kernels take n_class + 1 <= {CNN_MAX_CLASSES + 1} head outputs)")
    if B < 1 or S < 1 or B * S * input_dim >= 2 ** 31:
        raise ValueError(f"batch {B} x {S} frames x input_dim {input_dim}: at least one frame and B * S * input_dim < 2^31 "
                         f"(int element offsets of the embedding GEMM)")
    if erank_weight:
        raise ValueError(f"erank_weight {erank_weight}: the effective-rank penalty needs a fuser's token matrix; the CNN "
                         f"model has none")


class _Shape:
    def __init__(self, eng, B, S, train):
        dev, H, K = eng.device, eng.H, eng.K
        N, BQ = B * S, B * POOL_ROWS
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)     # noqa: E731
        self.B, self.S, self.N, self.BQ = B, S, N, BQ
        self.x, self.pooled = f(N, H), f(BQ, H)
        self.actdur = f(BQ, K + 1)
        self.seg = f(N, eng.Kseg)
        self.loss = torch.zeros(4, dtype=torch.float32, device=dev)
        self.loss_ws = torch.zeros(ops.losses_ws_floats(B, S, POOL_ROWS), dtype=torch.float32, device=dev)
        self.counts = torch.zeros(4, dtype=torch.int64, device=dev)
        if train:
            self.d_actdur, self.d_seg = torch.zeros(BQ, K + 1, dtype=torch.float32, device=dev), f(N, eng.Kseg)
            self.d_x0, self.d_pre = f(N, H), f(N, H)
            self._f, self._dev = f, dev
            # allocated by the first step that uses them: d_pooled and d_x on the composed route only, the rest with
            # supcon_weight > 0 only
            self.d_pooled = self.d_x = self.d_extra = self.sc_ws = self.sc_loss = None

    def composed_bufs(self):
        if self.d_x is None:
            self.d_pooled, self.d_x = self._f(self.BQ, self.d_x0.shape[1]), self._f(*self.d_x0.shape)

    def supcon_bufs(self, chain, wide=False):
        if self.sc_ws is None:
            self.sc_ws = self._f(ops.supcon_ws_floats(self.N, self.d_x0.shape[1], True, wide=wide))
            self.sc_loss = torch.zeros(1, dtype=torch.float32, device=self._dev)
        if chain and self.d_extra is None:
            self.d_extra = self._f(*self.d_x0.shape)


class CnnEngine(EngineBase):
    _Shape = _Shape
    defer_tail = True                       # a training forward() leaves everything behind x to losses() on the chain route
    wide_supcon = False                     # --wide_supcon: the contrastive term runs the kernel's wide route (hidden > 256, the
                                            # composed route); set before the first training step with supcon_weight > 0

    def __init__(self, module, device):
        self.H, self.Q, self.K = module.hidden_dim, POOL_ROWS, module.n_class
        self.D = module.input_embed.in_features
        check_cnn_shape(self.H, module.n_query, self.K, input_dim=self.D)          # (before anything is enqueued)
        self._init_engine(module, device, is_live)
        self.Kseg = module.fc_seg.out_features
        self.pad_idx = module.src_pad_idx
        self._erank_weight = 0.0
        self.supcon_weight = 0.0            # --supcon_weight: total loss += weight * SupConLoss over the 'supcon' rows (x)
        self.supcon_temperature = 0.07      # --temperature
        # the step's two branches as two launches (csrc/afft.hip, csrc/cnn.hip) where both admit the shape and chain_pays();
        # None: by shape, True: wherever admitted, False: the composed launches
        self.use_seg_chain = None
        self.ride_loss_reduce = True        # losses(tick=True) on the chain: the AdamW launch reduces the loss partials

    @property
    def erank_weight(self):
        return self._erank_weight

    @erank_weight.setter
    def erank_weight(self, v):
        check_cnn_shape(self.H, POOL_ROWS, self.K, erank_weight=float(v))

    def _admit(self, B, S, train):
        check_cnn_shape(self.H, POOL_ROWS, self.K, B=B, S=S, input_dim=self.D)

    def chain_admitted(self):
        return ops.cnn_seg_supported(self.H, self.Kseg) and ops.afft_head_supported(self.H, POOL_ROWS, self.K + 1)

    def _chain(self, w):
        if self.use_seg_chain is not None and not self.use_seg_chain:
            return False
        if not self.chain_admitted():
            return False
        return True if self.use_seg_chain else chain_pays(w.B, w.S, self.H, self.Kseg)

    # ------------------------------------------------------------------------------------------------------
    def _tail_fwd(self, w, chain):
        a = self.arena
        ops.gemm(GEMM_NT, w.x, a.p("fc_seg.weight"), w.seg, bias=a.p("fc_seg.bias"), ws=self.ws)
        if chain:
            ops.afft_head_fwd(w.x, self.w_head, self.b_head, w.pooled, w.actdur, w.B, w.S, POOL_ROWS)
        else:
            ops.avgpool_rows_fwd(w.x, w.pooled, w.B, w.S, POOL_ROWS)
            ops.gemm(GEMM_NT, w.pooled, self.w_head, w.actdur, bias=self.b_head, ws=self.ws)

    def forward(self, feats, depth=None, labels=None, mode="train", training=False, need_grad=True):
        """feats [B,S,D] f32.  depth / labels: accepted for FusionEngine's signature and never read.  Returns views: seg
        [B,S,K-1], action [B,8,K], duration [B,8], supcon [B,S,H] (= x).  A training forward on the chain route with
        defer_tail set enqueues the embedding GEMM alone: the other outputs are valid after losses()."""
        a, H, K = self.arena, self.H, self.K
        assert feats.is_cuda and feats.dtype == torch.float32
        B, S = feats.shape[0], feats.shape[1]
        N = B * S
        x_rgb = feats.reshape(N, -1)
        assert x_rgb.shape[1] == self.D and x_rgb.is_contiguous()
        w = self._shape(B, S, need_grad)
        self._loss_pending = None          # (a pending loss reduction never survives into another step)
        chain = self._chain(w)
        ops.gemm(GEMM_NT, x_rgb, a.p("input_embed.weight"), w.x, bias=a.p("input_embed.bias"), act=1, ws=self.ws)
        deferred = bool(chain and self.defer_tail and need_grad and mode == "train")
        if not deferred:
            self._tail_fwd(w, chain)
        self.last = dict(w=w, x_rgb=x_rgb, drop=False, mode=mode, tp=None, chain=chain, deferred=deferred, chained=False)
        return dict(seg=w.seg.view(B, S, self.Kseg), action=w.actdur[:, :K].view(B, POOL_ROWS, K),
                    duration=w.actdur[:, K].view(B, POOL_ROWS), supcon=w.x.view(B, S, H))

    # ------------------------------------------------------------------------------------------------------
    def _supcon_kw(self):
        return dict(temperature=self.supcon_temperature, base_temperature=SUPCON_BASE_T, ignore_index=self.pad_idx,
                    normalize=True, wide=self.wide_supcon)

    def losses(self, past_label, target, target_dur, with_grad=True, val_mode=False, tick=False):
        """The 3 losses + counters of train_unimodal.py:188-225 (exclude index 120).  Composed: one launch, fills d_seg /
        d_actdur.  Chain (a deferred training forward): r3d_afft_head_step + r3d_cnn_seg_step, which also leave d_pre; with
        tick the reduction of the loss partials rides in adamw().  With supcon_weight > 0 (training only) the supervised
        contrastive loss of the L2-normalised 'supcon' rows over the per-frame labels, padded frames ignored, is added:
        w.sc_loss holds it and loss[3] gains weight times it."""
        st = self.last
        w, K, a = st["w"], self.K, self.arena
        self._loss_pending = None
        supcon = bool(self.supcon_weight and with_grad and not val_mode)
        if supcon and not ops.supcon_supported(self.H, wide=self.wide_supcon):      # (before anything of this step's losses is enqueued)
            raise ValueError(f"hidden {self.H}: --supcon_weight on the CNN model contrasts its 'supcon' rows x [B*S, hidden], "
                             f"and the supervised contrastive kernels take a width <= 256 (--wide_supcon: <= 2048)")
        lab = past_label.reshape(-1)
        st["supcon_labels"] = lab if supcon else None
        if st["deferred"] and with_grad and not val_mode:
            st["deferred"] = False
            ops.afft_head_step(w.x, self.w_head, self.b_head, w.pooled, w.actdur, w.B, w.S, POOL_ROWS, past_label, target,
                               target_dur, self.pad_idx, EXCLUDE_CLASS_IDX, w.d_actdur, w.d_x0, w.loss_ws,
                               dur_den=self.dur_den, tick_a=self.step_t if tick else None)
            if supcon:
                w.supcon_bufs(True, self.wide_supcon)
                ops.supcon_fwd(w.x, lab, w.N, w.N, w.sc_ws, w.sc_loss, **self._supcon_kw())
                ops.supcon_bwd(w.x, lab, w.N, w.N, w.sc_ws, w.d_extra, gscale=self.supcon_weight, add=False,
                               **self._supcon_kw())
            ops.cnn_seg_step(w.x, a.p("fc_seg.weight"), a.p("fc_seg.bias"), lab, self.pad_idx, EXCLUDE_CLASS_IDX, w.d_seg,
                             w.d_pre, w.loss_ws, seg=w.seg, d_x0=w.d_x0, d_extra=w.d_extra if supcon else None)
            st["chained"] = True
            job = ops.loss_finalize_job(w.loss_ws, w.B, w.S, POOL_ROWS, True, self.dur_den, w.loss, w.counts)
            if tick and self.ride_loss_reduce:
                self._loss_pending = (job, w if supcon else None)
            else:
                ops.losses_finalize(job)
                if supcon:
                    w.loss[3:4].add_(w.sc_loss, alpha=self.supcon_weight)
            return w.loss, w.counts
        if st["deferred"]:                  # (forward deferred its tail and no chain step follows)
            st["deferred"] = False
            self._tail_fwd(w, st["chain"])
        ops.losses_fwd_bwd_kseg(None if val_mode else w.seg, w.actdur[:, :K], w.actdur[:, K:], K + 1, past_label, target,
                                target_dur, w.B, w.S, POOL_ROWS, K, self.Kseg, self.pad_idx, EXCLUDE_CLASS_IDX, w.loss,
                                w.counts, val_mode=val_mode, dur_den=self.dur_den,
                                d_seg=w.d_seg if with_grad else None, d_act=w.d_actdur[:, :K] if with_grad else None,
                                d_dur=w.d_actdur[:, K:] if with_grad else None, ld_ddur=K + 1, ws=w.loss_ws,
                                tick_a=self.step_t if tick else None)
        if supcon:
            w.supcon_bufs(False, self.wide_supcon)
            ops.supcon_fwd(w.x, lab, w.N, w.N, w.sc_ws, w.sc_loss, **self._supcon_kw())
            w.loss[3:4].add_(w.sc_loss, alpha=self.supcon_weight)
        return w.loss, w.counts

    # ------------------------------------------------------------------------------------------------------
    def backward(self, d_seg=None, d_actdur=None, fused_adamw=None, adamw_next=False, d_supcon=None):
        """Adjoint of forward(); gradients land in the grad arena (written, not accumulated).  d_supcon (optional
        [B,S,H]): a gradient on the 'supcon' output (= x), added in front of the ReLU gate.  After a chain losses() only the
        three weight gradients are left."""
        assert fused_adamw is None
        st = self.last
        w, a, H, ws = st["w"], self.arena, self.H, self.ws
        B, S, N = w.B, w.S, w.N

        def wgrad(dy, x, gw, gb):
            ops.gemm(GEMM_TN, dy, x, gw, bias_grad=gb, ws=ws)

        if st["chained"]:
            assert d_seg is None and d_actdur is None and d_supcon is None, \
                "gradients handed in by the caller take the composed route (clear defer_tail before forward())"
        else:
            assert not st["deferred"], "backward() follows losses() or a forward() with defer_tail cleared"
            if d_seg is not None and d_seg.data_ptr() != w.d_seg.data_ptr():
                w.d_seg.copy_(d_seg)
            if d_actdur is not None and d_actdur.data_ptr() != w.d_actdur.data_ptr():
                w.d_actdur.copy_(d_actdur)
            # ---- heads and pooling back to x, then the segmentation head, then through the ReLU
            w.composed_bufs()
            ops.gemm(GEMM_NN, w.d_actdur, self.w_head, w.d_pooled, ws=ws)
            ops.avgpool_rows_bwd(w.d_pooled, w.d_x0, B, S, POOL_ROWS)
            if d_supcon is not None:
                ops.add_rowbcast(w.d_x0, d_supcon.reshape(N, H).contiguous(), N, w.d_x0)
            if st.get("supcon_labels") is not None:
                ops.supcon_bwd(w.x, st["supcon_labels"], N, N, w.sc_ws, w.d_x0, gscale=self.supcon_weight, add=True,
                               **self._supcon_kw())
            ops.gemm(GEMM_NN, w.d_seg, a.p("fc_seg.weight"), w.d_x, res1=w.d_x0, ws=ws)
            ops.posenc_bwd(w.d_x, w.d_pre, gate=w.x)
        wgrad(w.d_seg, w.x, a.g("fc_seg.weight"), a.g("fc_seg.bias"))
        wgrad(w.d_actdur, w.pooled, self.gw_head, self.gb_head)
        wgrad(w.d_pre, st["x_rgb"], a.g("input_embed.weight"), a.g("input_embed.bias"))

    # ------------------------------------------------------------------------------------------------------
    def adamw(self, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, tick_dropout=False, ticked=False,
              skip_depth=False, prefill_dropout=False, before_flat=None):
        """One fused launch over the live prefix of the arena (main_nturgbd.py:140; train_unimodal.py:230).  A loss
        reduction left pending by a chain losses(tick=True) rides as one more workgroup."""
        self.set_lr(lr)
        if not ticked:
            ops.tick(self.step_t, None)     # (no dropout: nothing else to advance)
        pending, self._loss_pending = self._loss_pending, None
        job, sc_w = pending if pending is not None else (None, None)
        self._adamw_flat(0, self.arena.n_live, weight_decay, betas, eps, grad_scale, loss_fin=job)
        if sc_w is not None:
            sc_w.loss[3:4].add_(sc_w.sc_loss, alpha=self.supcon_weight)

    def train_step(self, feats, depth, past_label, target_dur, target, lr, weight_decay, training=True):
        """forward + losses + backward + AdamW, all enqueued, no host sync.  Returns (loss[4], counts[4]) on device.
        depth: accepted for FusionEngine's signature, never read (may be None)."""
        self.set_lr(lr)
        self.forward(feats, None, past_label, "train", training)
        loss, counts = self.losses(past_label, target, target_dur, tick=True)
        self.backward()
        self.adamw(lr, weight_decay, ticked=True)
        return loss, counts
