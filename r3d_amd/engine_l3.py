"""Host-side sequencing of the L3 query model (reference model/futr_unsupervised_temp3.py) and of its loop's loss
(train/train_unsupervised.py) on one MI355X.

The RGB embedding + sinusoidal encoding is the decoder's MEMORY (the DETR encoder is constructed but bypassed).  The model's
own branch is `l3_attention`, an nn.MultiheadAttention(batch_first=True) the reference calls AFTER 'b t c -> t b c': its
batch is the S frame indices and its sequence the B clips, so for every frame and head the B rows { b S + t } attend to one
another (csrc/attention_xclip.hip reads them in place).  Its output + a sinusoidal table is `l3`; adaptive_avg_pool1d(l3,
n_query) is the decoder's per-clip QUERY (an activation: its gradient returns into the branch) and fc_l3(l3) the `l3`
logits.  Heads: action / duration on the n_query decoder rows, seg = fc_seg(memory) with n_class outputs.

The loss (train_unsupervised.py:300-362): focal loss L_3 and temporal cluster loss L_c on the l3 logits, L_seg / L_act /
L_dur from the loss launch (exclude_class_idx None = -1 here), and csrc/l3mix.hip forms m, the weights a, b, c and the total
on the device; a and b are handed to the focal and cluster backward launches as device scalars, so the step reads nothing
back and a new epoch needs no new capture (the warm-up factor wf is a device scalar like the learning rate; the graph key holds
the dropout state, so a run captures once with dropout on and once after validate() has left the model in eval()).

Same flat arenas, workspaces and method surface (forward / losses / backward / adamw / train_step) as engine_unsup; the step
is composed launch by launch on one stream.  Dead parameters (transformer.encoder.*, query_attention.*) keep grad None and
get no AdamW update."""
import torch

from . import ops
from ._lib import GEMM_NT, GEMM_NN, GEMM_TN
from .decoder_composed import DROP_SCALE, decoder_buffers, decoder_forward, decoder_backward
from .engine import check_hidden, max_clip_len
from .engine_base import DROP_P, EngineBase

LIVE_PREFIXES = ("input_embed.", "l3_attention.", "transformer.decoder.", "pos_embedding", "fc_seg.", "fc.", "fc_len.",
                 "fc_l3.")
L3_PAD, L3_EXCLUDE = 47, 48       # cal_performance_focal(l3_logits, query_label, 47, 48) (train_unsupervised.py:306)
VAL_L3_PAD = 48                   # validate() calls it with pad 48 (:163)
MAX_CLIPS = 64                    # the cross-clip attention holds the B x B scores of a (frame, head) in LDS
MAX_QUERY_NUM = 256               # the cluster kernel's width
MAX_SEG_CLASSES = 1023


def is_live(name):
    return name.startswith(LIVE_PREFIXES)


def check_l3_shape(H, heads, Q, query_num, n_class):
    """Raises ValueError unless the engine runs the model at some batch; each refusal names the limit."""
    check_hidden(H, heads)
    dh = H // heads
    if dh > 128:
        raise ValueError(f"head width {dh} (hidden {H} / {heads} heads) > 128: the cross-clip attention's limit")
    if Q * dh > 1024 or not ops.mha_core_supported(Q, Q, dh, True):
        raise ValueError(f"{Q} queries at head width {dh}: the attention core holds n_query * head width <= 1024 outputs per wave")
    if not 1 <= query_num <= MAX_QUERY_NUM:
        raise ValueError(f"query_num {query_num}: the cluster loss kernel takes rows of 1 to {MAX_QUERY_NUM} logits")
    if not 1 <= n_class <= MAX_SEG_CLASSES:
        raise ValueError(f"n_class {n_class}: the loss kernels take 1 to {MAX_SEG_CLASSES} classes")


def check_l3_batch(B, S, H, heads, Q, max_pos_len, train):
    """Raises ValueError unless a batch of B clips of S frames runs; checked before anything is enqueued."""
    if not 1 <= B <= MAX_CLIPS:
        raise ValueError(f"{B} clips: the cross-clip attention attends over the clips of a batch, 1 to {MAX_CLIPS} of them")
    if S <= 0:
        raise ValueError(f"clip length {S}: at least one frame")
    if S > max_pos_len:
        raise ValueError(f"clip length {S} > max_pos_len {max_pos_len}: the rows of the positional tables")
    if B * S * 3 * H >= 2 ** 31:
        raise ValueError(f"{B} clips x {S} frames at hidden {H}: the cross-clip attention indexes B * S * 3 * hidden < 2^31")
    longest = max_clip_len(H, heads, Q, max_pos_len, train)
    if S > longest:
        raise ValueError(f"clip length {S} > {longest}: the cross-attention core keeps {Q} x S scores per head in LDS")


class _Shape:
    def __init__(self, eng, B, S, train):
        dev, H, Q, K, C = eng.device, eng.H, eng.Q, eng.K, eng.C
        N, BQ = B * S, B * Q
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)     # noqa: E731
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)     # noqa: E731
        self.B, self.S, self.N, self.BQ = B, S, N, BQ
        self.rgb, self.mem = f(N, H), f(N, H)
        self.xqkv, self.xo, self.l3pre, self.l3 = f(N, 3 * H), f(N, H), f(N, H), f(N, H)
        self.qpos, self.l3log, self.seg = f(BQ, H), f(N, C), f(N, eng.Kseg)
        decoder_buffers(self, eng, Q, "core", train, dict(pe_rgb=N * H))
        self.actdur = f(BQ, K + 1)
        # losses: loss3 = (seg, action, duration, their sum); l3 / lc device scalars; mix = (m, a, b, c, total)
        self.loss3, self.loss_l3, self.loss_lc, self.mix = f(4), f(1), f(1), f(5)
        self.loss_ws = z(ops.losses_ws_floats(B, S, Q))
        self.loss_ws_q = z(ops.losses_ws_floats(B, Q, Q))          # validate(): the loss launch over the Q action rows
        self.counts = z(4, dt=torch.int64)
        self.l3_counts = z(2, dt=torch.int64)
        self.l3_flags, self.l2_flags = z(N, dt=torch.uint8), z(N, dt=torch.uint8)
        self.focal_ws = f(N)
        self.clu_ws = f(ops.tcluster_ws_floats(B, S, C))
        self.mix_ws = z(ops.l3mix_ws_ints(N), dt=torch.int32)
        self.runs = [z(B * S, dt=torch.int32) for _ in range(3)] + [z(B, dt=torch.int32)]      # first, last, starts, count
        if train:
            self.d_actdur, self.d_seg, self.d_l3log = z(BQ, K + 1), f(N, eng.Kseg), f(N, C)
            self.d_mem, self.d_qpos, self.d_qtmp = f(N, H), f(BQ, H), f(BQ, H)
            self.d_pool, self.d_l3, self.d_xo, self.d_xqkv, self.d_rgb_pre = f(N, H), f(N, H), f(N, H), f(N, 3 * H), f(N, H)


class L3Engine(EngineBase):
    _Shape = _Shape

    def __init__(self, module, device):
        self.H, self.Q, self.K = module.hidden_dim, module.n_query, module.n_class
        self.heads, self.L = module.n_head, module.num_decoder_layers
        self.C = module.fc_l3.out_features                        # query_num
        self.Kseg = module.fc_seg.out_features                    # n_class (not n_class - 1)
        check_l3_shape(self.H, self.heads, self.Q, self.C, self.Kseg)
        self._init_engine(module, device, is_live)
        self.dh = self.H // self.heads
        self.pad_idx = module.src_pad_idx
        self.D = module.input_embed.in_features
        self.pe = module.pos_enc.pos_table[0]
        self.pe_l3 = module.positional_embedding_l3.to(self.device).contiguous()
        self.max_pos_len = min(module.pos_embedding.shape[1], self.pe.shape[0], self.pe_l3.shape[0])
        self.dropout_enabled = bool(getattr(module, "r3d_dropout_enabled", True))
        self.wf_t = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._wf_host = None

    def _admit(self, B, S, train):
        check_l3_batch(B, S, self.H, self.heads, self.Q, self.max_pos_len, train)

    # ------------------------------------------------------------------------------------------------------
    def forward(self, feats, labels, mode="train", training=False, need_grad=True):
        """feats [B, S, D] f32, labels [B, S] int64 (train mode only: the decoder's key-padding mask).
        futr_unsupervised_temp3.py:72-143.  Returns views: l3 [B, S, query_num], seg [B, S, n_class], action [B, Q, K],
        duration [B, Q]."""
        a, Q, K, heads = self.arena, self.Q, self.K, self.heads
        B, S = feats.shape[0], feats.shape[1]
        N, BQ = B * S, B * Q
        assert feats.is_cuda and feats.dtype == torch.float32
        w = self._shape(B, S, need_grad)                         # (the admission of the batch comes first)
        x = feats.reshape(N, self.D)
        assert x.is_contiguous()
        drop = training and need_grad and self.dropout_enabled
        if drop:
            ops.dropout_mask(w.drop_pool, DROP_P, self.drop_seed, self.drop_offset)
        dm = (lambda k: w.drop[k]) if drop else (lambda k: None)
        key_labels = None
        if mode == "train":
            assert labels.dtype == torch.int64 and labels.is_cuda and labels.is_contiguous()
            key_labels = labels
        ws = self.ws
        # ---- memory: relu(x W^T + b) + pos_table, dropout (:87-93)
        ops.gemm(GEMM_NT, x, a.p("input_embed.weight"), w.rgb, bias=a.p("input_embed.bias"), act=1, ws=ws)
        ops.posenc_fwd(w.rgb, self.pe, S, w.mem, drop_mask=dm("pe_rgb"), drop_scale=DROP_SCALE)
        # ---- l3 branch: attention over the clips of each frame (:99-104), no mask, no dropout
        ops.gemm(GEMM_NT, w.mem, a.p("l3_attention.in_proj_weight"), w.xqkv, bias=a.p("l3_attention.in_proj_bias"), ws=ws)
        ops.xclip_fwd(w.xqkv, w.xo, B, S, heads)
        ops.gemm(GEMM_NT, w.xo, a.p("l3_attention.out_proj.weight"), w.l3pre, bias=a.p("l3_attention.out_proj.bias"), ws=ws)
        ops.posenc_fwd(w.l3pre, self.pe_l3, S, w.l3)
        ops.avgpool_rows_fwd(w.l3, w.qpos, B, S, Q)                                          # the decoder's query (:110)
        ops.gemm(GEMM_NT, w.l3, a.p("fc_l3.weight"), w.l3log, bias=a.p("fc_l3.bias"), ws=ws)         # (:139)
        ops.gemm(GEMM_NT, w.mem, a.p("fc_seg.weight"), w.seg, bias=a.p("fc_seg.bias"), ws=ws)        # (:134)
        # ---- decoder, post-norm: Q queries per clip, query_pos = w.qpos, memory + pos as keys and values
        decoder_forward(self, w, w.qpos, BQ, w.mem, key_labels, drop)
        ops.gemm(GEMM_NT, w.tgtF, self.w_head, w.actdur, bias=self.b_head, ws=ws)
        self.last = dict(w=w, x=x, drop=drop, mode=mode, key_labels=key_labels)
        return dict(l3=w.l3log.view(B, S, self.C), seg=w.seg.view(B, S, self.Kseg), action=w.actdur[:, :K].view(B, Q, K),
                    duration=w.actdur[:, K].view(B, Q))

    # ------------------------------------------------------------------------------------------------------
    def set_wf(self, wf):
        """the loop's warm-up factor (get_warmup_factor(epoch, 0, 30, 60)): a device scalar, written once per epoch"""
        if self._wf_host != float(wf):
            self.wf_t.fill_(float(wf))
            self._wf_host = float(wf)

    def losses(self, past_label, target, target_dur, query_label, with_grad=True, tick=False):
        """The five losses of train_unsupervised.py:300-362, the mix and -- with_grad -- every logit gradient: d_seg and
        d_actdur scaled by c, d_l3log = a dL_3 + b dL_c.  Returns (mix[5] = m, a, b, c, total; loss3[4]; loss_l3[1];
        loss_lc[1]; counts[4]; l3_counts[2]) on the device; nothing is read back."""
        w, K, B, S = self.last["w"], self.K, self.last["w"].B, self.last["w"].S
        assert query_label.dtype == torch.int64 and query_label.is_cuda and query_label.is_contiguous()
        assert query_label.numel() == w.N
        ta = self.step_t if tick else None
        tb = self.drop_offset if (tick and self.last["drop"]) else None
        first, last, starts, count = w.runs
        ops.label_runs(query_label.view(B, S), first, last, starts, count)
        ops.tcluster_fwd(w.l3log, B, S, starts, last, count, w.clu_ws, w.loss_lc)
        ops.focal_rows(w.l3log, query_label.view(-1), L3_PAD, exclude_idx=L3_EXCLUDE, ws=w.focal_ws, loss_out=w.loss_l3,
                       flags=w.l3_flags, counts=w.l3_counts)
        ops.losses_fwd_bwd_kseg(w.seg, w.actdur[:, :K], w.actdur[:, K:], K + 1, past_label, target, target_dur, B, S, self.Q, K,
                                self.Kseg, self.pad_idx, -1, w.loss3, w.counts,
                                d_seg=w.d_seg if with_grad else None, d_act=w.d_actdur[:, :K] if with_grad else None,
                                d_dur=w.d_actdur[:, K:] if with_grad else None, ld_ddur=K + 1, ws=w.loss_ws, tick_a=ta, tick_b=tb)
        ops.l3mix(w.seg, past_label.view(-1), w.l3_flags, self.pad_idx, w.loss_l3, w.loss_lc, w.loss3, self.wf_t, w.mix_ws,
                  w.mix, d_seg=w.d_seg if with_grad else None, d_actdur=w.d_actdur if with_grad else None, l2_flags=w.l2_flags)
        if with_grad:
            ops.focal_rows(w.l3log, query_label.view(-1), L3_PAD, exclude_idx=L3_EXCLUDE, d_pred=w.d_l3log, d_loss=w.mix[1:2])
            ops.tcluster_bwd(w.l3log, B, S, starts, last, count, w.clu_ws, w.d_l3log, d_loss=w.mix[2:3], add=True)
        return w.mix, w.loss3, w.loss_l3, w.loss_lc, w.counts, w.l3_counts

    # ------------------------------------------------------------------------------------------------------
    def backward(self):
        """Adjoint of forward() from d_seg, d_actdur and d_l3log; gradients land in the grad arena (written, not accumulated)."""
        st = self.last
        w, a, Q, heads, ws = st["w"], self.arena, self.Q, self.heads, self.ws
        B, S, BQ = w.B, w.S, w.BQ
        drop = st["drop"]

        def wgrad(dy, x, gw, gb, **kw):
            ops.gemm(GEMM_TN, dy, x, gw, bias_grad=gb, ws=ws, **kw)

        # ---- heads, decoder
        wgrad(w.d_actdur, w.tgtF, self.gw_head, self.gb_head)
        ops.gemm(GEMM_NN, w.d_actdur, self.w_head, w.d_tgtF, ws=ws)
        decoder_backward(self, w, w.qpos, BQ, w.mem, st["key_labels"], drop)      # (the query is an activation: w.d_qpos)
        # ---- d l3 = the pool's adjoint (decoder query) + fc_l3's input gradient
        ops.avgpool_rows_bwd(w.d_qpos, w.d_pool, B, S, Q)
        wgrad(w.d_l3log, w.l3, a.g("fc_l3.weight"), a.g("fc_l3.bias"))
        ops.gemm(GEMM_NN, w.d_l3log, a.p("fc_l3.weight"), w.d_l3, res1=w.d_pool, ws=ws)
        # ---- the cross-clip attention's out-projection, core and in-projection
        wgrad(w.d_l3, w.xo, a.g("l3_attention.out_proj.weight"), a.g("l3_attention.out_proj.bias"))
        ops.gemm(GEMM_NN, w.d_l3, a.p("l3_attention.out_proj.weight"), w.d_xo, ws=ws)
        ops.xclip_bwd(w.xqkv, w.d_xo, w.d_xqkv, B, S, heads)
        wgrad(w.d_xqkv, w.mem, a.g("l3_attention.in_proj_weight"), a.g("l3_attention.in_proj_bias"))
        # ---- d memory = cross-attention K/V + seg head + in-projection; through the encoding's dropout and the ReLU
        wgrad(w.d_seg, w.mem, a.g("fc_seg.weight"), a.g("fc_seg.bias"))
        ops.gemm(GEMM_NN, w.d_seg, a.p("fc_seg.weight"), w.d_mem, res1=w.d_mp, ws=ws)
        ops.gemm(GEMM_NN, w.d_xqkv, a.p("l3_attention.in_proj_weight"), w.d_mem, accumulate=True, ws=ws)
        ops.posenc_bwd(w.d_mem, w.d_rgb_pre, drop_mask=w.drop["pe_rgb"] if drop else None, drop_scale=DROP_SCALE, gate=w.rgb)
        wgrad(w.d_rgb_pre, st["x"], a.g("input_embed.weight"), a.g("input_embed.bias"))

    # ------------------------------------------------------------------------------------------------------
    def _tick_counter(self, tick_dropout):
        return self.drop_offset if (self.last and self.last["drop"]) else None      # (whatever the caller says)

    def train_step(self, feats, past_label, target_dur, target, query_label, lr, weight_decay, wf, training=True,
                   betas=(0.9, 0.999), eps=1e-8, acc=None):
        """forward + losses + backward + AdamW, all enqueued on the current stream, no host sync.  acc: (float64 [6], int64 [6])
        device accumulators of an epoch -- total, L_3, L_seg, L_act, L_dur, L_c and the six counters -- added to inside the step."""
        self.set_lr(lr)
        self.set_wf(wf)
        self.forward(feats, past_label, "train", training)
        out = self.losses(past_label, target, target_dur, query_label, tick=True)
        self.backward()
        self.adamw(lr, weight_decay, betas=betas, eps=eps, ticked=True)
        if acc is not None:
            mix, loss3, l_l3, l_lc, counts, l3_counts = out
            acc[0][0:1] += mix[4:5]
            acc[0][1:2] += l_l3
            acc[0][2:5] += loss3[:3]
            acc[0][5:6] += l_lc
            acc[1][:4] += counts
            acc[1][4:] += l3_counts
        return out

    def train_step_graphed(self, feats, past_label, target_dur, target, query_label, lr, weight_decay, wf, training=True,
                           betas=(0.9, 0.999), eps=1e-8, acc=None):
        """train_step replayed from a captured graph: one capture per (batch shape, AdamW hyper-parameters, dropout state); lr
        and wf are device scalars, so they change without a new capture.  The batch is copied into the capture's own buffers."""
        B, S = feats.shape[0], feats.shape[1]
        key = (B, S, float(weight_decay), tuple(betas), float(eps), bool(training and self.dropout_enabled), acc is not None)
        self.set_lr(lr)
        self.set_wf(wf)
        return self._replay(key, (feats, past_label, target_dur, target, query_label), lambda bufs: self.train_step(
            *bufs, lr, weight_decay, wf, training, betas, eps, acc), tuple(acc or ()))
