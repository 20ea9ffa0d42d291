"""Host-side sequencing of the build-defined three-modality (RGB + depth + gaze) token-fusion model
(model/futr_safuser_tokenfusion3.py) on one MI355X: one engine per model, as engine_afft.py and engine_l3.py are.

Front: the RGB embedding GEMM and the bf16x3 depth projection as engine_afft's front runs them (one paired launch where it
applies, split-K slabs left for the seam), then either

  seam route      ONE launch (csrc/fuse3_seam.hip: r3d_embed_fuse3_fwd) turns the two slab sets and `gaze` into the three
                  finished embeddings, the exchanged token rows x0 [3N, H] and h1 = norm1(x0); its adjoint
                  r3d_embed_fuse3_bwd is one launch too;
  composed route  the same arithmetic from existing launches: layernorm_fwd x 2 (depth with its slab sums, gaze), the tiny
                  gaze product (a GEMM), r3d_token_exchange3_fwd, layernorm_fwd; mirrored in the backward.

`seam_pays(N, H)` picks the route on the host (M3Engine.use_seam forces one).  The rest of the fuser block are the launches
cmfuser3.CMFuser3 makes over the 3N token rows: the qkv GEMM, r3d_attn3_fwd, proj + residual, norm2, fc1 with GELU (its
pre-activation kept), fc2 with both residuals, fuser.norm, r3d_triple_mean_fwd.  Selection: the train-mode mask is a constant,
computed once; eval mode runs three r3d_colabssum launches + r3d_token_select as CMFuser3.select does; `last_idx` keeps the
selected indices readable.  The decoder is decoder_composed's (the launches FusionEngine._decoder_unfused makes: mha_core_*,
layernorm_*; query_pos = the query_embed parameter), heads and losses r3d_losses_fwd_bwd; any number of decoder layers.
The backward mirrors the forward; weight gradients are GEMMs with column-sum epilogues; the depth weight gradient and AdamW
follow engine_afft.

Rank penalty (erank_weight, erank_route) on the fused tokens [N = B S, H]: the ops / erank calls of
FusionEngine._erank_forward / _erank_backward -- the in-LDS Jacobi where erank_fits, the blocked Jacobi on the orientation
with the fewer columns otherwise, erank.ErankTall for route "tall" -- on the step's own stream, without a warm start.

Every method only enqueues on the current stream: a training step can be captured as one hipGraph (train_step_graphed).

Live parameters: the two-modality model's (engine.LIVE_PREFIXES) plus gaze_projection.* and gaze_layernorm.*.  Dead
parameters (transformer.encoder.*, l3_attention.*, query_attention.*, fc_l3.*, fuser.modality_token, fuser.projection.*,
fuser.fusion_conv.*) keep grad None and get no AdamW update, weight decay included.  With three tokens the -inf-diagonal
softmax has two logits, so the Q and K rows of attn.qkv.weight receive real gradients."""
import torch

from . import ops
from ._lib import GEMM_NT, GEMM_NN, GEMM_TN
from .decoder_composed import DROP_SCALE, decoder_buffers, decoder_forward, decoder_backward
from .engine import ERANK_ROUTES, SEAM_MAX_H, check_hidden, check_erank_shape, live_rule, max_clip_len
from .engine_base import DROP_P, EXCLUDE_CLASS_IDX, EngineBase

M3_LIVE_EXTRA = ("gaze_projection.", "gaze_layernorm.")
is_live = live_rule(M3_LIVE_EXTRA)
M3_MAX_GAZE = ops.FUSE3_MAX_GAZE
M3_MAX_CLASSES = 1023           # the loss kernels' class limit
M3_MAX_HEAD_WIDTH = 128         # r3d_attn3_* (two channels per lane) and the decoder attention cores


SEAM_PAYS_AT = frozenset({(128, 128), (256, 1024)})         # (N = B S, H) measured ahead, see seam_pays


def seam_pays(N, H):
    """True where the front's seam runs as the one-launch kernels of csrc/fuse3_seam.hip, False: the composed launches.
    The rule follows the measurement of tools/m3_step_speed.py (profiles/m3_step_speed.json) shape by shape -- the seam alone,
    forward + backward with the finalize launch of its LayerNorm partials, each form replayed as a graph on one MI355X, seam
    against composed: 17.0 us against 46.1 at (B, S, H) = (8, 16, 128) and 42.0 against 87.9 at (16, 16, 1024), so the seam is
    the route there (the graphed step agrees: 0.486 against 0.531 ms and 2.38 against 2.49); 236.9 against 149.0 at
    (8, 1142, 128), where it LOSES -- its backward leaves one (dgamma, dbeta) partial per frame for three LayerNorms, and the
    finalize launch reduces them with 2 H / 64 workgroups per LayerNorm (12 in all at hidden 128), each walking all 9136
    frames (the 8.4 ms step does not separate the routes) -- so long clips keep the composed launches.  A shape that was not timed keeps the composed route; M3Engine.use_seam forces either (the suite runs both)."""
    return (N, H) in SEAM_PAYS_AT


def check_m3_args(seg=True, anticipate=True, input_type="i3d_transcript", parallel=False, pixel_shard=False):
    """Raises ValueError for what the three-modality engine does not run; host-only."""
    if not seg or not anticipate:
        raise ValueError("args.seg and args.anticipate must both be on: the three-modality step implements the two-modality "
                         "model's three losses (segmentation, anticipation, duration)")
    if input_type != "i3d_transcript":
        raise ValueError(f"input_type {input_type!r}: only 'i3d_transcript' is built (the 'gt' embedding branch is not on "
                         f"the RGB + depth + gaze path)")
    if pixel_shard:
        raise ValueError("--pixel_shard: the three-modality model runs on one GPU (the sharded depth projection is not built "
                         "for M3Engine)")
    if parallel:
        raise ValueError("the three-modality model runs on one GPU: data-parallel steps (gradient buckets, the duration "
                         "denominator exchange) are not built for M3Engine")


def check_m3_shape(H, n_head, n_query, n_class, gaze_dim, erank_route="jacobi"):
    """Raises ValueError naming the limit unless the engine runs the model at some batch; host arithmetic only."""
    check_hidden(H, n_head)
    if H > SEAM_MAX_H:
        raise ValueError(f"hidden {H} > {SEAM_MAX_H}: the three-modality seam holds a channel row in one wave's registers")
    dh = H // n_head
    if dh > M3_MAX_HEAD_WIDTH:
        raise ValueError(f"head width {dh} (hidden {H} / {n_head} heads) > {M3_MAX_HEAD_WIDTH}: the three-token attention "
                         f"and the decoder attention cores hold a head in one wave")
    if n_query < 1 or n_query * dh > 1024 or not ops.mha_core_supported(n_query, n_query, dh, True):
        raise ValueError(f"{n_query} queries at head width {dh}: the attention core holds n_query * head width <= 1024 "
                         f"outputs per wave")
    if not 1 <= gaze_dim <= M3_MAX_GAZE:
        raise ValueError(f"gaze_dim {gaze_dim}: the seam takes 1 to {M3_MAX_GAZE} gaze inputs per frame")
    if not 1 <= n_class <= M3_MAX_CLASSES:
        raise ValueError(f"n_class {n_class}: the loss kernels take 1 to {M3_MAX_CLASSES} classes")
    if erank_route not in ERANK_ROUTES:
        raise ValueError(f"erank_route {erank_route!r}: one of {ERANK_ROUTES}")


def check_m3_batch(B, S, H, n_head, n_query, max_pos_len, train, erank_weight=0.0, erank_route="jacobi"):
    """Raises ValueError unless a batch of B clips of S frames runs; checked before anything is enqueued."""
    if B < 1 or S < 1:
        raise ValueError(f"batch {B} x {S} frames: at least one clip of at least one frame")
    if S > max_pos_len:
        raise ValueError(f"clip length {S} > max_pos_len {max_pos_len}: the rows of pos_embedding")
    if 3 * B * S * H >= 2 ** 31:
        raise ValueError(f"{B} clips x {S} frames at hidden {H}: the token rows index 3 * B * S * hidden < 2^31")
    longest = max_clip_len(H, n_head, n_query, max_pos_len, train)
    if S > longest:
        raise ValueError(f"clip length {S} > {longest}: the cross-attention core keeps {n_query} x S scores per head in LDS")
    if erank_weight != 0.0 and train:
        check_erank_shape(B, S, H, erank_route)


class _Shape:
    """Activation / gradient workspace for one (B, S, train) shape; rgb, dep, gaze and fused are the names rankstream reads."""

    def __init__(self, eng, B, S, train):
        dev, H, Q, K, heads = eng.device, eng.H, eng.Q, eng.K, eng.heads
        N, BQ = B * S, B * Q
        R = 3 * N
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)     # noqa: E731
        self.B, self.S, self.N, self.BQ, self.R = B, S, N, BQ, R
        self.rgb, self.dep, self.dep_pre, self.gaze, self.gz_pre = f(N, H), f(N, H), f(N, H), f(N, H), f(N, H)
        self.mean_d, self.rstd_d, self.mean_g, self.rstd_g = f(N), f(N), f(N), f(N)
        self.sums = torch.empty(3, H, dtype=torch.float64, device=dev)
        self.idx = torch.empty(3, H // 4, dtype=torch.int64, device=dev)
        self.mask = f(3, H)
        self.x0, self.h1, self.m1, self.r1 = f(R, H), f(R, H), f(R), f(R)
        self.qkv, self.probs, self.att = f(R, 3 * H), f(N * heads * 6), f(R, H)
        self.x1, self.h2, self.m2, self.r2 = f(R, H), f(R, H), f(R), f(R)
        self.u, self.f1, self.x3 = f(R, 4 * H), f(R, 4 * H), f(R, H)
        self.y, self.mf, self.rf, self.fused = f(R, H), f(R), f(R), f(N, H)
        self.seg = f(N, K)
        decoder_buffers(self, eng, Q, "core", train, dict(x0=R * H))
        self.actdur = f(BQ, K + 1)
        self.loss = torch.zeros(4, dtype=torch.float32, device=dev)
        self.counts = torch.zeros(4, dtype=torch.int64, device=dev)
        self.loss_ws = torch.zeros(ops.losses_ws_floats(B, S, Q), dtype=torch.float32, device=dev)
        if train:
            self.d_actdur, self.d_seg = torch.zeros(BQ, K + 1, dtype=torch.float32, device=dev), f(N, K)
            self.d_fused2 = f(N, H)
            self.d_y, self.d_x3, self.d_u, self.d_h2, self.d_x1 = f(R, H), f(R, H), f(R, 4 * H), f(R, H), f(R, H)
            self.d_att, self.d_qkv, self.d_h1, self.d_x0 = f(R, H), f(R, 3 * H), f(R, H), f(R, H)
            self.d_rgb, self.d_rgb_pre, self.d_dep, self.d_dep_pre, self.d_gz, self.d_gz_pre = (f(N, H) for _ in range(6))
            self.lnp_seam = dict(n1=f(2 * N * H), dep=f(2 * N * H), gz=f(2 * N * H))     # one (dgamma, dbeta) pair per frame


class M3Engine(EngineBase):
    _Shape = _Shape
    rank_penalty = True

    def __init__(self, module, device):
        args = module.args
        check_m3_args(seg=bool(getattr(args, "seg", True)), anticipate=bool(getattr(args, "anticipate", True)),
                      input_type=getattr(args, "input_type", "i3d_transcript"))          # (before anything is allocated)
        self.H, self.Q, self.K = module.hidden_dim, module.n_query, module.n_class
        self.heads, self.L, self.G = module.n_head, module.num_decoder_layers, module.gaze_dim
        check_m3_shape(self.H, self.heads, self.Q, self.K, self.G)
        self._init_engine(module, device, is_live)
        self.dh = self.H // self.heads
        self.pad_idx = module.src_pad_idx
        self.P, self.D = module.depth_projection.in_features, module.input_embed.in_features
        self.max_pos_len = module.pos_embedding.shape[1]
        self.ws_side = ops.GemmWorkspace(self.device)
        self.use_seam = None                    # None: seam_pays(N, H); True / False: forced
        self.pair_embeddings = True             # both input projections in one launch (ops.gemm_bf3_nt_pair) where it applies
        self.depth_prec = 1                     # the two depth-projection GEMMs on the bf16 matrix cores (exact 3-way split)
        self.dropout_enabled = bool(getattr(module, "r3d_dropout_enabled", True))
        self._erank_weight, self._erank_route = 0.0, "jacobi"
        self.erank_max_sweeps = 30
        self.train_mask = None
        self.last_idx = None

    def refuse_data_parallel(self):
        """parallel.DataParallelStep asks this of an engine before it hooks into it: this one runs on one GPU"""
        check_m3_args(parallel=True)

    @property
    def erank_weight(self):
        return self._erank_weight

    @erank_weight.setter
    def erank_weight(self, v):
        self._erank_weight = float(v)

    @property
    def erank_route(self):
        return self._erank_route

    @erank_route.setter
    def erank_route(self, v):
        if v not in ERANK_ROUTES:
            raise ValueError(f"erank_route {v!r}: one of {ERANK_ROUTES}")
        self._erank_route = str(v)

    # ------------------------------------------------------------------------------------------------------
    def _shape(self, B, S, train):
        # (admitted on every call, not only before the first allocation: the penalty's weight and route change between steps)
        check_m3_batch(B, S, self.H, self.heads, self.Q, self.max_pos_len, train, self._erank_weight, self._erank_route)
        return super()._shape(B, S, train)

    def _seam(self, w):
        return seam_pays(w.N, self.H) if self.use_seam is None else bool(self.use_seam)

    def _train_mask(self):
        """token_fusion's train-mode scores are the constant |d mean / dx|: the selection is the tie rule alone, the same at
        every batch shape (r3d_token_select orders equal scores by index) -- computed once."""
        if self.train_mask is None:
            H = self.H
            idx = torch.empty(3, H // 4, dtype=torch.int64, device=self.device)
            mask = torch.empty(3, H, dtype=torch.float32, device=self.device)
            ops.token_select(H // 4, idx, mask, score_f=torch.full((3, H), 1.0 / H, dtype=torch.float32, device=self.device))
            self.train_mask = (idx, mask)
        return self.train_mask

    # ------------------------------------------------------------------------------------------------------
    def forward(self, feats, depth, labels, mode="train", training=False, need_grad=True, gaze=None):
        """feats [B,S,D] f32, depth [B,S,...] f32 (flattened to [N,P]), gaze [B,S,gaze_dim] f32, labels [B,S] int64 (train
        mode: the decoder's key padding mask).  Returns views into the workspace: seg [B,S,K], action [B,Q,K], duration [B,Q]."""
        if gaze is None:
            raise ValueError("the three-modality model needs the gaze track: forward(..., gaze=[B, S, gaze_dim])")
        a, H, Q, K, heads, G = self.arena, self.H, self.Q, self.K, self.heads, self.G
        B, S = feats.shape[0], feats.shape[1]
        N, R = B * S, 3 * B * S
        assert feats.is_cuda and depth.is_cuda and gaze.is_cuda
        assert feats.dtype == torch.float32 and depth.dtype == torch.float32 and gaze.dtype == torch.float32
        x_rgb, x_dep, x_gz = feats.reshape(N, -1), depth.reshape(N, -1), gaze.reshape(N, -1)
        assert x_rgb.shape[1] == self.D and x_dep.shape[1] == self.P and x_gz.shape[1] == G, (x_rgb.shape, x_dep.shape, x_gz.shape)
        assert x_rgb.is_contiguous() and x_dep.is_contiguous() and x_gz.is_contiguous()
        w = self._shape(B, S, need_grad)                        # (the admission of the batch comes first)
        drop = bool(training and need_grad and self.dropout_enabled)
        if drop:
            ops.dropout_mask(w.drop_pool, DROP_P, self.drop_seed, self.drop_offset)
        dsc = DROP_SCALE
        dm = (lambda k: w.drop[k]) if drop else (lambda k: None)
        key_labels = None
        if mode == "train":
            assert labels.dtype == torch.int64 and labels.is_cuda and labels.is_contiguous()
            key_labels = labels
        ws = self.ws
        pre = "fuser.blocks.0."
        p = a.p
        seam = self._seam(w) and mode == "train"              # (the one-launch seam takes a mask known before the embeddings)
        # ---- the two input projections (:179,195); bias / ReLU / LayerNorm belong to what follows
        dr = d = None
        if seam and self.depth_prec == 1 and self.pair_embeddings:      # (raw RGB slabs: only the seam sums them)
            pr = ops.gemm_bf3_nt_pair(x_dep, p("depth_projection.weight"), w.dep_pre, self.ws,
                                      x_rgb, p("input_embed.weight"), w.rgb, self.ws_side)
            if pr is not None:
                d, dr = pr
        if dr is None:
            dr = ops.gemm(GEMM_NT, x_rgb, p("input_embed.weight"), w.rgb, bias=p("input_embed.bias"), act=1,
                          ws=self.ws_side, defer_reduce=seam, prec=self.depth_prec)
        if d is None:
            d = ops.gemm(GEMM_NT, x_dep, p("depth_projection.weight"), w.dep_pre, bias=p("depth_projection.bias"),
                         ws=self.ws, defer_reduce=True, prec=self.depth_prec)
        # (composed route: the RGB GEMM reduced its own slabs -- bias and ReLU are in its epilogue)
        rgb_src, ns_r = (self.ws_side.buf, dr.splitk) if (seam and dr.splitk > 1) else (w.rgb, 0)
        if d.splitk > 1:
            dep_src, ns_d, bias_d = self.ws.buf, d.splitk, p("depth_projection.bias")
        else:
            dep_src, ns_d, bias_d = w.dep_pre, 1, None
        if seam:
            idx, mask = self._train_mask()
            ops.embed_fuse3_fwd(rgb_src, ns_r, p("input_embed.bias"), dep_src, ns_d, bias_d, p("depth_layernorm.weight"),
                                p("depth_layernorm.bias"), x_gz, p("gaze_projection.weight"), p("gaze_projection.bias"),
                                p("gaze_layernorm.weight"), p("gaze_layernorm.bias"), mask, dm("x0"), dsc,
                                p(pre + "norm1.weight"), p(pre + "norm1.bias"), w.rgb, w.dep_pre, w.mean_d, w.rstd_d, w.dep,
                                w.gz_pre, w.mean_g, w.rstd_g, w.gaze, w.x0, w.h1, w.m1, w.r1)
        else:
            # ---- composed: finish the three embeddings, select, exchange, norm1
            if d.splitk > 1:                    # (first: it drains the deferred split-K slabs in self.ws)
                ops.layernorm_fwd(dep_src, p("depth_layernorm.weight"), p("depth_layernorm.bias"), w.dep, w.mean_d, w.rstd_d,
                                  relu=True, nsplit=ns_d, bias=bias_d, pre_out=w.dep_pre, rows=N, H=H)
            else:
                ops.layernorm_fwd(w.dep_pre, p("depth_layernorm.weight"), p("depth_layernorm.bias"), w.dep, w.mean_d,
                                  w.rstd_d, relu=True)
            ops.gemm(GEMM_NT, x_gz, p("gaze_projection.weight"), w.gz_pre, bias=p("gaze_projection.bias"), ws=ws)
            ops.layernorm_fwd(w.gz_pre, p("gaze_layernorm.weight"), p("gaze_layernorm.bias"), w.gaze, w.mean_g, w.rstd_g,
                              relu=True)
            if mode == "train":
                idx, mask = self._train_mask()
            else:
                ops.colabssum(w.rgb, w.sums[0])
                ops.colabssum(w.dep, w.sums[1])
                ops.colabssum(w.gaze, w.sums[2])
                ops.token_select(H // 4, w.idx, w.mask, score_sum=w.sums, count=float(N))
                idx, mask = w.idx, w.mask
            ops.token_exchange3_fwd(w.rgb, w.dep, w.gaze, mask, w.x0, drop_mask=self._dm2(dm("x0"), R, H), drop_scale=dsc)
            ops.layernorm_fwd(w.x0, p(pre + "norm1.weight"), p(pre + "norm1.bias"), w.h1, w.m1, w.r1)
        self.last_idx = idx
        # ---- the fuser block over the 3N token rows (cmfuser3._Fuser3Fn.forward), fuser.norm, the triple mean
        ops.gemm(GEMM_NT, w.h1, p(pre + "attn.qkv.weight"), w.qkv, ws=ws)
        ops.attn3_fwd(w.qkv, w.probs, w.att, heads)
        ops.gemm(GEMM_NT, w.att, p(pre + "attn.proj.weight"), w.x1, bias=p(pre + "attn.proj.bias"), res1=w.x0, ws=ws)
        ops.layernorm_fwd(w.x1, p(pre + "norm2.weight"), p(pre + "norm2.bias"), w.h2, w.m2, w.r2)
        ops.gemm(GEMM_NT, w.h2, p(pre + "mlp.mlp.0.weight"), w.f1, bias=p(pre + "mlp.mlp.0.bias"), act=2, pre_out=w.u, ws=ws)
        ops.gemm(GEMM_NT, w.f1, p(pre + "mlp.mlp.2.weight"), w.x3, bias=p(pre + "mlp.mlp.2.bias"), res1=w.x1, res2=w.x0, ws=ws)
        ops.layernorm_fwd(w.x3, p("fuser.norm.weight"), p("fuser.norm.bias"), w.y, w.mf, w.rf)
        ops.triple_mean_fwd(w.y, w.fused)
        er = bool(self._erank_weight != 0.0 and need_grad)
        if er:
            self._erank_forward(w)
        # ---- segmentation head (:228-232) and the decoder (memory = fused, encoder bypassed), post-norm
        ops.gemm(GEMM_NT, w.fused, p("fc_seg.weight"), w.seg, bias=p("fc_seg.bias"), ws=ws)
        decoder_forward(self, w, p("query_embed.weight"), Q, w.fused, key_labels, drop)       # (query_pos: a parameter)
        ops.gemm(GEMM_NT, w.tgtF, self.w_head, w.actdur, bias=self.b_head, ws=ws)
        self.last = dict(w=w, x_rgb=x_rgb, x_dep=x_dep, x_gz=x_gz, mask=mask, idx=idx, drop=drop, mode=mode, seam=seam,
                         erank=er)
        if self.rank_stream is not None:
            for attr, acc in self.rank_stream:
                acc.update(getattr(w, attr), labels, self.pad_idx if labels is not None else None)
        return dict(seg=w.seg.view(B, S, K), action=w.actdur[:, :K].view(B, Q, K), duration=w.actdur[:, K].view(B, Q))

    # ---- effective-rank penalty on the fused tokens: the calls of FusionEngine._erank_forward / _erank_backward -----------
    def _erank_forward(self, w):
        N, H = w.N, self.H
        if self._erank_route == "tall":
            from .erank import ErankTall, fold_pays
            fold = self.erank_fold if self.erank_fold is not None else fold_pays(N, H)
            if getattr(w, "er_tall", None) is None or w.er_tall.fold != fold:
                w.er_tall = ErankTall(N, H, self.device, fold=self.erank_fold,
                                      max_sweeps=30 if ops.erank_fits(2 * H, H) else self.erank_max_sweeps)
                w.er_tall_gout = torch.empty(1, dtype=torch.float32, device=self.device)
            w.er_tall.forward(w.fused)
            return
        if not hasattr(w, "er_sigma"):
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)     # noqa: E731
            w.er_gout = f(1)
            w.er_blk = None
            if ops.erank_fits(N, H):
                w.er_sigma, w.er_stats, w.er_af = f(1, H), f(1, 4), f(1, H, N)
            else:
                # beyond one CU's LDS: the blocked Jacobi on the orientation with the fewer columns (fused^T is handed over
                # as it lies in memory)
                w.er_flip = N < H
                Rr, Cc = (H, N) if w.er_flip else (N, H)
                w.er_blk = ops.ErankBlockedBufs(Rr, Cc, self.device, max_sweeps=self.erank_max_sweeps)
                w.er_sigma, w.er_stats = w.er_blk.sigma.view(1, Cc), w.er_blk.stats.view(1, 4)
        if w.er_blk is not None:
            ops.erank_blocked_into(w.fused, w.er_blk, transposed=w.er_flip)
        else:
            ops.erank_jacobi(w.fused, w.er_sigma, w.er_stats, af_t=w.er_af)

    def _erank_backward(self, w):
        """d_fused2 += d(-erank_weight * erank) / d fused"""
        if self._erank_route == "tall":
            w.er_tall_gout.fill_(-float(self._erank_weight))
            w.er_tall.backward(w.fused, w.er_tall_gout, w.d_fused2, True, self.ws)
            return
        from .erank import ErankBackward
        if not hasattr(w, "er_bwd"):
            w.er_bwd = ErankBackward(w.N, self.H, w.er_blk is not None and w.er_flip, self.device,
                                     ld=w.er_blk.Rp if w.er_blk is not None else None)
        w.er_gout.fill_(-float(self._erank_weight))
        A = w.er_blk.af_t if w.er_blk is not None else w.er_af[0]
        w.er_bwd.run(w.fused, A, w.er_sigma[0], w.er_stats[0], w.er_gout, w.d_fused2, True, self.ws)

    def erank_value(self):
        """Effective rank of the last forward's fused tokens (device scalar; valid when erank_weight != 0)."""
        w = self.last["w"]
        return w.er_tall.stats[0, 0] if self._erank_route == "tall" else w.er_stats[0, 0]

    # ------------------------------------------------------------------------------------------------------
    def losses(self, past_label, target, target_dur, with_grad=True, val_mode=False, tick=False):
        """The 3 losses + counters of train_proposed_depth.py:171-213 in one launch; fills d_seg / d_actdur.  tick=True: the
        launch also advances the optimiser's step counter (and the dropout offset when dropout ran)."""
        w, K = self.last["w"], self.K
        ta = self.step_t if tick else None
        tb = self.drop_offset if (tick and self.last["drop"]) else None
        if with_grad:
            assert hasattr(w, "d_actdur"), "losses(with_grad=True) needs a forward with need_grad=True"
        ops.losses_fwd_bwd(None if val_mode else w.seg, w.actdur[:, :K], w.actdur[:, K:], K + 1, past_label, target,
                           target_dur, w.B, w.S, self.Q, K, self.pad_idx, EXCLUDE_CLASS_IDX, w.loss, w.counts,
                           val_mode=val_mode, d_seg=w.d_seg if with_grad else None,
                           d_act=w.d_actdur[:, :K] if with_grad else None, d_dur=w.d_actdur[:, K:] if with_grad else None,
                           ld_ddur=K + 1, ws=w.loss_ws, tick_a=ta, tick_b=tb)
        return w.loss, w.counts

    # ------------------------------------------------------------------------------------------------------
    def backward(self, d_seg=None, d_actdur=None, fused_adamw=None, adamw_next=False):
        """Adjoint of forward(); gradients land in the grad arena (written, not accumulated)."""
        assert fused_adamw is None
        self.backward_main(d_seg, d_actdur)
        self.backward_depth_wgrad()

    def backward_main(self, d_seg=None, d_actdur=None):
        """Everything of the backward except depth_projection.weight."""
        st = self.last
        w, a, H, heads, ws = st["w"], self.arena, self.H, self.heads, self.ws
        N, R = w.N, w.R
        assert hasattr(w, "d_actdur"), "backward() needs a forward with need_grad=True"
        self._copy_in(w, d_seg, d_actdur)
        drop = st["drop"]
        dsc = DROP_SCALE
        dm = (lambda k, r, c: w.drop[k].view(r, c)) if drop else (lambda k, r, c: None)
        dmf = (lambda k: w.drop[k]) if drop else (lambda k: None)
        pre = "fuser.blocks.0."

        def ln_bwd(dy, x, mean, rstd, gname, bname, dx, **kw):
            ops.layernorm_bwd(dy, x, mean, rstd, a.p(gname), a.p(bname), dx, a.g(gname), a.g(bname), ws=ws, **kw)

        def wgrad(dy, x, gw, gb, **kw):
            ops.gemm(GEMM_TN, dy, x, gw, bias_grad=gb, ws=ws, **kw)

        # ---- heads, decoder (query_embed's gradient: the clips' column sums of the query-position gradients)
        wgrad(w.d_actdur, w.tgtF, self.gw_head, self.gb_head)
        ops.gemm(GEMM_NN, w.d_actdur, self.w_head, w.d_tgtF, ws=ws)
        decoder_backward(self, w, a.p("query_embed.weight"), self.Q, w.fused, None, drop, a.g("query_embed.weight"))
        # ---- d fused = cross-attention K/V + segmentation head (+ the rank penalty)
        wgrad(w.d_seg, w.fused, a.g("fc_seg.weight"), a.g("fc_seg.bias"))
        ops.gemm(GEMM_NN, w.d_seg, a.p("fc_seg.weight"), w.d_fused2, res1=w.d_mp, ws=ws)
        if st["erank"]:
            self._erank_backward(w)
        # ---- the fuser block (cmfuser3._Fuser3Fn.backward)
        ops.triple_mean_bwd(w.d_fused2, w.d_y)
        ln_bwd(w.d_y, w.x3, w.mf, w.rf, "fuser.norm.weight", "fuser.norm.bias", w.d_x3)
        wgrad(w.d_x3, w.f1, a.g(pre + "mlp.mlp.2.weight"), a.g(pre + "mlp.mlp.2.bias"))
        ops.gemm(GEMM_NN, w.d_x3, a.p(pre + "mlp.mlp.2.weight"), w.d_u, aux=w.u, mul=2, ws=ws)          # * GELU'(u)
        wgrad(w.d_u, w.h2, a.g(pre + "mlp.mlp.0.weight"), a.g(pre + "mlp.mlp.0.bias"))
        ops.gemm(GEMM_NN, w.d_u, a.p(pre + "mlp.mlp.0.weight"), w.d_h2, ws=ws)
        ln_bwd(w.d_h2, w.x1, w.m2, w.r2, pre + "norm2.weight", pre + "norm2.bias", w.d_x1, add1=w.d_x3)
        wgrad(w.d_x1, w.att, a.g(pre + "attn.proj.weight"), a.g(pre + "attn.proj.bias"))
        ops.gemm(GEMM_NN, w.d_x1, a.p(pre + "attn.proj.weight"), w.d_att, ws=ws)
        ops.attn3_bwd(w.qkv, w.d_att, w.d_qkv, heads)
        ops.gemm(GEMM_TN, w.d_qkv, w.h1, a.g(pre + "attn.qkv.weight"), ws=ws)
        ops.gemm(GEMM_NN, w.d_qkv, a.p(pre + "attn.qkv.weight"), w.d_h1, ws=ws)
        mask = st["mask"]
        if st["seam"]:
            # norm1 backward (+ both residual gradients), dropout, exchange adjoint, ReLU gates, both LayerNorm adjoints
            ops.embed_fuse3_bwd(w.d_h1, w.x0, w.m1, w.r1, a.p(pre + "norm1.weight"), w.d_x1, w.d_x3, dmf("x0"), dsc, mask,
                                w.rgb, w.dep_pre, w.mean_d, w.rstd_d, a.p("depth_layernorm.weight"),
                                a.p("depth_layernorm.bias"), w.gz_pre, w.mean_g, w.rstd_g, a.p("gaze_layernorm.weight"),
                                a.p("gaze_layernorm.bias"), w.d_rgb_pre, w.d_dep_pre, w.d_gz_pre, w.lnp_seam["n1"],
                                w.lnp_seam["dep"], w.lnp_seam["gz"])
            if not hasattr(w, "ln_group_seam"):
                w.ln_group_seam = ops.LnFinalizeGroup([
                    (w.lnp_seam["n1"], -N, H, a.g(pre + "norm1.weight"), a.g(pre + "norm1.bias")),
                    (w.lnp_seam["dep"], -N, H, a.g("depth_layernorm.weight"), a.g("depth_layernorm.bias")),
                    (w.lnp_seam["gz"], -N, H, a.g("gaze_layernorm.weight"), a.g("gaze_layernorm.bias"))])
            w.ln_group_seam.launch()
        else:
            ln_bwd(w.d_h1, w.x0, w.m1, w.r1, pre + "norm1.weight", pre + "norm1.bias", w.d_x0, add1=w.d_x1, add2=w.d_x3)
            ops.token_exchange3_bwd(w.d_x0, mask, w.d_rgb, w.d_dep, w.d_gz, drop_mask=dm("x0", R, H), drop_scale=dsc)
            ops.posenc_bwd(w.d_rgb, w.d_rgb_pre, gate=w.rgb)              # input_embed's ReLU (:183)
            ln_bwd(w.d_dep, w.dep_pre, w.mean_d, w.rstd_d, "depth_layernorm.weight", "depth_layernorm.bias", w.d_dep_pre,
                   relu=True)
            ln_bwd(w.d_gz, w.gz_pre, w.mean_g, w.rstd_g, "gaze_layernorm.weight", "gaze_layernorm.bias", w.d_gz_pre,
                   relu=True)
        # ---- the embeddings' parameter gradients (depth_projection.weight: backward_depth_wgrad); gaze_projection's is
        # [H, gaze_dim]: the GEMM's scalar path, column sums in its epilogue
        wgrad(w.d_gz_pre, st["x_gz"], a.g("gaze_projection.weight"), a.g("gaze_projection.bias"))
        wgrad(w.d_rgb_pre, st["x_rgb"], a.g("input_embed.weight"), a.g("input_embed.bias"))
        ops.colsum(w.d_dep_pre, a.g("depth_projection.bias"), ws=ws)

    def backward_depth_wgrad(self):
        """depth_projection.weight gradient [H, P] = d_dep_pre^T . depth: the last and largest kernel of the backward."""
        st = self.last
        ops.gemm(GEMM_TN, st["w"].d_dep_pre, st["x_dep"], self.arena.g("depth_projection.weight"), ws=self.ws,
                 prec=self.depth_prec)

    # ------------------------------------------------------------------------------------------------------
    def train_step(self, feats, depth, past_label, target_dur, target, lr, weight_decay, training=True, gaze=None,
                   betas=(0.9, 0.999), eps=1e-8):
        """forward + losses + backward + AdamW, all enqueued, no host sync.  Returns (loss[4], counts[4]) on device."""
        self.set_lr(lr)
        self.forward(feats, depth, past_label, "train", training, gaze=gaze)
        loss, counts = self.losses(past_label, target, target_dur, tick=True)
        self.backward()
        self.adamw(lr, weight_decay, betas=betas, eps=eps, ticked=True)
        return loss, counts

    def train_step_graphed(self, feats, depth, past_label, target_dur, target, lr, weight_decay, training=True, gaze=None,
                           betas=(0.9, 0.999), eps=1e-8):
        """train_step replayed from a captured graph: one capture per (batch shape, AdamW hyper-parameters, dropout state,
        penalty, route, longest clip seen so far); lr is a device scalar.  The batch is copied into the capture's own buffers."""
        B, S = feats.shape[0], feats.shape[1]
        # the step clears the pos_embedding gradient rows [S, mark) a longer earlier batch wrote, `mark` being the high-water
        # mark AS IT STANDS AFTER THIS STEP; a captured step clears the range of its capture, so the mark's value is part of the
        # key: a longer batch seen since then takes a new capture (train()'s _graph_key holds the same value)
        key = (B, S, tuple(depth.shape), float(weight_decay), tuple(betas), float(eps),
               bool(training and self.dropout_enabled), self._erank_weight, self._erank_route, self.use_seam,
               max(self.pos_grad_rows, S))
        self.set_lr(lr)
        return self._replay(key, (feats, depth, past_label, target_dur, target, gaze), lambda bufs: self.train_step(
            *bufs[:5], lr, weight_decay, training, gaze=bufs[5], betas=betas, eps=eps))
