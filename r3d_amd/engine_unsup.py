"""Host-side sequencing of the depth-as-query model (reference model/futr_unsupervised_depth.py) on one MI355X.

The second model file BASELINE.json's north star names for the per-modality encoder embeddings: the RGB embedding
(+ sinusoidal PositionalEncoding, model/extras/position.py:15-35) is the decoder's MEMORY (the DETR encoder is
constructed but bypassed, transformer.py:77-78) and the depth embedding 160*120 -> H + LayerNorm + ReLU (+ the same
encoding) is its per-clip QUERY -- S queries per clip, different for every clip, so unlike the token-fusion model the
query-side self-attention depends on the data and its gradient flows back into the depth projection.  The S decoder
outputs are average-pooled to n_query rows before the anticipation heads (futr_unsupervised_depth.py:134).

Same flat arenas, workspaces, C ABI and method surface (forward / losses / backward / adamw / train_step) as
engine.FusionEngine, so r3d_amd.train_proposed_depth.train() drives either model; every product is a launch of
libr3d_hip.so (GEMMs with prologues / epilogues, the attention core, LayerNorm, the loss kernel, fused AdamW, plus the
positional-encoding and pooling kernels of csrc/posenc.hip).  This variant is composed launch by launch (no paired /
seam / tail fusions): it is a coverage row of SURVEY.md 8(a) A2/A3, not the headline workload.
"""
import torch

from . import attention, ops
from ._lib import GEMM_NT, GEMM_NN, GEMM_TN
from .decoder_composed import DROP_SCALE, decoder_buffers, decoder_forward, decoder_backward
from .engine import check_hidden
from .engine_base import DROP_P, EXCLUDE_CLASS_IDX, EngineBase


# Shape admission (as engine.py's): every clip brings S queries, so both decoder attentions run Lq = Lk = S and the core's
# limits (S * head width <= 1024 outputs per wave, S x S scores in 160 KiB of LDS) bound the clip length itself.  Checked on
# the host before anything is enqueued; tests/test_query_admission_cpu.py pins them.  long_clips (opts --long_clips, read by
# the models into r3d_long_clips) adds the tiled core (csrc/attention_tiled.hip) for the shapes past those limits.
QUERY_ROUTES = ("core", "tiled")        # (never "splitk": S queries)


def query_attention_route(S, H, heads, train, long_clips):
    """The route (attention.pick) of both decoder attentions of an S-frame clip: "core", "tiled" (only with long_clips) or
    None (refused)."""
    return attention.pick(S, S, H // heads, train, QUERY_ROUTES if long_clips else QUERY_ROUTES[:1])


def check_query_engine_shape(H, heads, long_clips=False):
    """Raises ValueError unless the engine runs hidden H with `heads` attention heads at some training clip length."""
    check_hidden(H, heads)
    dh = H // heads
    if query_attention_route(1, H, heads, True, long_clips) is None:      # (the bound only tightens as S grows)
        raise ValueError(f"head width {dh} (hidden {H} / {heads} heads): no clip length trains -- the attention core's "
                         f"backward needs S * head width <= 1024 outputs per wave and its key chunks in 160 KiB of LDS")


def check_query_clip_shape(S, H, heads, max_pos_len, train, long_clips=False):
    """Raises ValueError unless a clip of S frames runs (train: with the backward, whose attention core needs more LDS).
    max_pos_len: the rows of pos_embedding (and, label-query, of positional_embedding_l3)."""
    if S <= 0:
        raise ValueError(f"clip length {S}: at least one frame")
    if S > max_pos_len:
        raise ValueError(f"clip length {S} > max_pos_len {max_pos_len}: the rows of the positional tables")
    dh = H // heads
    if query_attention_route(S, H, heads, train, long_clips) is None:
        hint = "" if long_clips else attention.long_clips_hint(S, S, dh, train, QUERY_ROUTES)
        raise ValueError(f"clip length {S} at head width {dh}: the decoder's attention cores run {S} queries x {S} keys, past "
                         f"the {'backward' if train else 'forward'} core's S * head width <= 1024 outputs per wave or its "
                         f"S x S scores in 160 KiB of LDS" + hint)


def max_query_clip_len(H, heads, max_pos_len, train, long_clips=False):
    """The longest clip check_query_clip_shape admits (0: none; the bound tightens monotonically with S)."""
    return attention.longest(lambda S: query_attention_route(S, H, heads, train, long_clips) is not None, max_pos_len)


LIVE_PREFIXES = ("input_embed.", "depth_projection.", "depth_layernorm.", "pos_embedding", "transformer.decoder.",
                 "fc_seg.", "fc.", "fc_len.", "query_embed.")     # (query_embed: the label-query variant, model/futr_proposed.py)


def is_live(name):
    """This model has no fuser, so these prefixes select exactly the parameters that receive a gradient (checked against
    the reference fixture's live set)."""
    return name.startswith(LIVE_PREFIXES)


class _Shape:
    def __init__(self, eng, B, S, train):
        dev, H, Q, K, heads = eng.device, eng.H, eng.Q, eng.K, eng.heads
        N, BQ = B * S, B * Q
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)     # noqa: E731
        self.B, self.S, self.N, self.BQ = B, S, N, BQ
        self.rgb, self.mem = f(N, H), f(N, H)
        self.dep_pre, self.dep, self.qpos = f(N, H), f(N, H), f(N, H)
        self.mean_d, self.rstd_d = f(N), f(N)
        decoder_buffers(self, eng, S, query_attention_route(S, H, heads, train, eng.long_clips), train,
                        dict(pe_rgb=N * H, pe_dep=N * H))
        self.pooled = f(BQ, H)
        self.actdur = f(BQ, K + 1)
        self.seg = f(N, eng.Kseg)
        self.loss = f(4)
        self.loss_ws = torch.zeros(ops.losses_ws_floats(B, S, Q), dtype=torch.float32, device=dev)
        self.counts = torch.zeros(4, dtype=torch.int64, device=dev)
        if train:
            self.d_actdur, self.d_seg = torch.zeros(BQ, K + 1, dtype=torch.float32, device=dev), f(N, eng.Kseg)
            self.d_pooled = f(BQ, H)
            self.d_mem, self.d_qpos, self.d_qtmp = f(N, H), f(N, H), f(N, H)
            self.d_rgb_pre, self.d_dep, self.d_dep_pre = f(N, H), f(N, H), f(N, H)


class UnsupDepthEngine(EngineBase):
    _Shape = _Shape

    def __init__(self, module, device):
        self.H, self.Q, self.K = module.hidden_dim, module.n_query, module.n_class
        self.heads, self.L = module.n_head, module.num_decoder_layers
        self.long_clips = bool(getattr(module, "r3d_long_clips", False))       # (opts --long_clips: the tiled attention route)
        check_query_engine_shape(self.H, self.heads, self.long_clips)
        self._init_engine(module, device, is_live)
        self.dh = self.H // self.heads
        self.pad_idx = module.src_pad_idx
        # label_query: model/futr_proposed.py -- the decoder query is nn.Embedding(label indices) + a sinusoidal table
        # (:103-106), the memory carries no positional encoding (:92-97) and fc_seg has n_class - 1 outputs (:38)
        self.label_query = not hasattr(module, "depth_projection")
        self.D = module.input_embed.in_features
        self.P = None if self.label_query else module.depth_projection.in_features
        self.Kseg = module.fc_seg.out_features
        self.pe = module.pos_enc.pos_table[0]                     # [3000, H] sinusoid buffer (position.py:19-27)
        self.pe_depth = None if self.label_query else module.pos_enc_depth.pos_table[0]
        self.pe_l3 = module.positional_embedding_l3.to(self.device).contiguous() if self.label_query else None
        self.max_pos_len = min(t.shape[0] for t in (module.pos_embedding[0], self.pe, self.pe_depth, self.pe_l3) if t is not None)
        self.dropout_enabled = bool(getattr(module, "r3d_dropout_enabled", True))

    def _admit(self, B, S, train):
        check_query_clip_shape(S, self.H, self.heads, self.max_pos_len, train, self.long_clips)

    # ------------------------------------------------------------------------------------------------------
    def forward(self, feats, depth, labels, mode="train", training=False, need_grad=True):
        """feats [B,S,D] f32, depth [B,S,...] f32 (flattened to [N,P]), labels [B,S] int64 (train mode only).
        futr_unsupervised_depth.py:85-163.  Returns views: seg [B,S,K], action [B,Q,K], duration [B,Q]."""
        a, H, Q, K = self.arena, self.H, self.Q, self.K
        B, S = feats.shape[0], feats.shape[1]
        N = B * S
        assert feats.is_cuda and depth.is_cuda and feats.dtype == torch.float32
        x_rgb = feats.reshape(N, -1)
        assert x_rgb.shape[1] == self.D and x_rgb.is_contiguous()
        if self.label_query:                                       # `depth` holds the label indices of the queries [B, S]
            assert depth.dtype == torch.int64 and depth.numel() == N and depth.is_contiguous()
            x_dep = depth.reshape(N)
        else:
            assert depth.dtype == torch.float32
            x_dep = depth.reshape(N, -1)
            assert x_dep.shape[1] == self.P and x_dep.is_contiguous(), (x_dep.shape, self.P)
        w = self._shape(B, S, need_grad)
        drop = training and need_grad and self.dropout_enabled
        if drop:
            ops.dropout_mask(w.drop_pool, DROP_P, self.drop_seed, self.drop_offset)
        dsc = DROP_SCALE
        dm = (lambda k: w.drop[k]) if drop else (lambda k: None)
        key_labels = None
        if mode == "train":                                     # get_pad_mask (:89,161-162) inside the attention kernel
            assert labels.dtype == torch.int64 and labels.is_cuda and labels.is_contiguous()
            key_labels = labels
        ws = self.ws
        # ---- RGB embedding: relu(x W^T + b) + pos_table, dropout (:93-99) -> decoder memory
        ops.gemm(GEMM_NT, x_rgb, a.p("input_embed.weight"), w.rgb, bias=a.p("input_embed.bias"), act=1, ws=ws)
        if self.label_query:
            w.mem = w.rgb                                          # (futr_proposed.py:92-97: no encoding on the memory)
            ops.embed_gather_fwd(a.p("query_embed.weight"), x_dep, self.pe_l3, S, w.qpos)      # (:103-106)
        else:
            ops.posenc_fwd(w.rgb, self.pe, S, w.mem, drop_mask=dm("pe_rgb"), drop_scale=dsc)
        # ---- depth embedding: relu(LN(x W^T + b)) + pos_table, dropout (:107-115) -> decoder query
        d = None if self.label_query else ops.gemm(GEMM_NT, x_dep, a.p("depth_projection.weight"), w.dep_pre, bias=a.p("depth_projection.bias"), ws=ws,
                     defer_reduce=True)                      # (split-K: raw slabs, the LayerNorm launch sums them + bias)
        if d is None:
            pass
        elif d.splitk > 1:
            ops.layernorm_fwd(ws.buf, a.p("depth_layernorm.weight"), a.p("depth_layernorm.bias"), w.dep, w.mean_d, w.rstd_d,
                              relu=True, nsplit=d.splitk, bias=a.p("depth_projection.bias"), pre_out=w.dep_pre, rows=N, H=H)
        else:
            ops.layernorm_fwd(w.dep_pre, a.p("depth_layernorm.weight"), a.p("depth_layernorm.bias"), w.dep, w.mean_d,
                              w.rstd_d, relu=True)
        if not self.label_query:
            ops.posenc_fwd(w.dep, self.pe_depth, S, w.qpos, drop_mask=dm("pe_dep"), drop_scale=dsc)
        # ---- segmentation head on the memory (:148; transformer.py:128 returns it untouched)
        ops.gemm(GEMM_NT, w.mem, a.p("fc_seg.weight"), w.seg, bias=a.p("fc_seg.bias"), ws=ws)
        # ---- decoder, post-norm (transformer.py:281-330): S queries per clip, query_pos = w.qpos (an activation)
        decoder_forward(self, w, w.qpos, N, w.mem, key_labels, drop)
        # ---- adaptive average pooling of the S outputs to n_query rows (:134) + anticipation heads (:140-144)
        ops.avgpool_rows_fwd(w.tgtF, w.pooled, B, S, Q)
        ops.gemm(GEMM_NT, w.pooled, self.w_head, w.actdur, bias=self.b_head, ws=ws)
        self.last = dict(w=w, x_rgb=x_rgb, x_dep=x_dep, drop=drop, mode=mode, tp=None, key_labels=key_labels)
        return dict(seg=w.seg.view(B, S, self.Kseg), action=w.actdur[:, :K].view(B, Q, K), duration=w.actdur[:, K].view(B, Q))

    # ------------------------------------------------------------------------------------------------------
    def losses(self, past_label, target, target_dur, with_grad=True, val_mode=False, tick=False):
        """The 3 losses + counters of train_proposed_depth.py:171-213 in one launch; fills d_seg / d_actdur."""
        w, K = self.last["w"], self.K
        if self.label_query:
            raise NotImplementedError("the fused loss kernel belongs to train_proposed_depth.py's composition; the label-query "
                                      "model's loop (train/train_unsupervised.py) is out of scope -- use the autograd bridge")
        ta = self.step_t if tick else None
        tb = self.drop_offset if (tick and self.last["drop"]) else None
        ops.losses_fwd_bwd(None if val_mode else w.seg, w.actdur[:, :K], w.actdur[:, K:], K + 1, past_label, target,
                           target_dur, w.B, w.S, self.Q, K, self.pad_idx, EXCLUDE_CLASS_IDX, w.loss, w.counts,
                           val_mode=val_mode, dur_den=self.dur_den,
                           d_seg=w.d_seg if with_grad else None, d_act=w.d_actdur[:, :K] if with_grad else None,
                           d_dur=w.d_actdur[:, K:] if with_grad else None, ld_ddur=K + 1, ws=w.loss_ws, tick_a=ta, tick_b=tb)
        return w.loss, w.counts

    # ------------------------------------------------------------------------------------------------------
    def backward(self, d_seg=None, d_actdur=None, fused_adamw=None, adamw_next=False):
        """Adjoint of forward(); gradients land in the grad arena (written, not accumulated).  (adamw_next: accepted for
        FusionEngine's signature; this engine has no parallel parameter-gradient branch.)"""
        assert fused_adamw is None
        st = self.last
        w, a, H, Q, ws = st["w"], self.arena, self.H, self.Q, self.ws
        B, S, N = w.B, w.S, w.N
        self._copy_in(w, d_seg, d_actdur)
        drop = st["drop"]
        dsc = DROP_SCALE
        dmf = (lambda k: w.drop[k]) if drop else (lambda k: None)

        def ln_bwd(dy, x, mean, rstd, gname, bname, dx, **kw):
            ops.layernorm_bwd(dy, x, mean, rstd, a.p(gname), a.p(bname), dx, a.g(gname), a.g(bname), ws=ws, **kw)

        def wgrad(dy, x, gw, gb, **kw):
            ops.gemm(GEMM_TN, dy, x, gw, bias_grad=gb, ws=ws, **kw)

        # ---- heads, pooling
        wgrad(w.d_actdur, w.pooled, self.gw_head, self.gb_head)
        ops.gemm(GEMM_NN, w.d_actdur, self.w_head, w.d_pooled, ws=ws)
        ops.avgpool_rows_bwd(w.d_pooled, w.d_tgtF, B, S, Q)
        # ---- decoder: the query is an activation, its gradient (w.d_qpos) reaches the depth projection / the lookup
        decoder_backward(self, w, w.qpos, N, w.mem, st["key_labels"], drop)
        # ---- memory: decoder part + segmentation head part; through the encoding's dropout and the ReLU (:97-99)
        wgrad(w.d_seg, w.mem, a.g("fc_seg.weight"), a.g("fc_seg.bias"))
        ops.gemm(GEMM_NN, w.d_seg, a.p("fc_seg.weight"), w.d_mem, res1=w.d_mp, ws=ws)
        ops.posenc_bwd(w.d_mem, w.d_rgb_pre, drop_mask=None if self.label_query else dmf("pe_rgb"), drop_scale=dsc, gate=w.rgb)
        wgrad(w.d_rgb_pre, st["x_rgb"], a.g("input_embed.weight"), a.g("input_embed.bias"))
        if self.label_query:                                       # the lookup's adjoint (futr_proposed.py:103)
            ops.embed_gather_bwd(w.d_qpos, st["x_dep"], a.g("query_embed.weight"))
            return
        # ---- query: through the encoding's dropout, ReLU + LayerNorm (:110-115), into the depth projection (:109)
        ops.posenc_bwd(w.d_qpos, w.d_dep, drop_mask=dmf("pe_dep"), drop_scale=dsc)
        ln_bwd(w.d_dep, w.dep_pre, w.mean_d, w.rstd_d, "depth_layernorm.weight", "depth_layernorm.bias", w.d_dep_pre,
               relu=True)
        ops.gemm(GEMM_TN, w.d_dep_pre, st["x_dep"], a.g("depth_projection.weight"), ws=ws)
        ops.rowmod_sum(w.d_dep_pre, 1, a.g("depth_projection.bias").view(1, H))

    # ------------------------------------------------------------------------------------------------------
    def train_step(self, feats, depth, past_label, target_dur, target, lr, weight_decay, training=True):
        """forward + losses + backward + AdamW, all enqueued, no host sync.  Returns (loss[4], counts[4]) on device."""
        self.forward(feats, depth, past_label, "train", training)
        loss, counts = self.losses(past_label, target, target_dur, tick=True)
        self.backward()
        self.adamw(lr, weight_decay, ticked=True)
        return loss, counts
