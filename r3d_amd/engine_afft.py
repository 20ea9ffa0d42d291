"""Host-side sequencing of the AFFT baseline (reference model/afft.py) on one MI355X.

The front is the plain SA-Fuser's, on the composed route only (the hidden-128 chain kernels fuse a decoder query branch
this model does not have): both input projections (one paired launch where it applies), the plain seam
(csrc/plainfuse.hip), the V-only product with the token swap, gemm_ln / GEMM + LayerNorm down to ``fused``.  Behind it
the pooled-head chain (csrc/afft.hip): adaptive average pool to n_query rows, the two heads, and in a training step the
anticipation CE, the duration loss and the way back to d_fused in ONE launch of one workgroup per clip.  The backward
then re-uses the plain model's composed launches; every weight gradient but depth_projection's is one grouped launch.

Live parameters: input_embed, depth_projection, depth_layernorm, fuser.blocks.0, fuser.norm, fuser.modality_token, fc,
fc_len.  Everything else the reference constructs (transformer, query_embed, pos_embedding, l3_attention,
query_attention, fc_l3, fc_seg, fuser.projection) gets no gradient and AdamW does not touch it, weight decay included.
The Q and K rows of attn.qkv.weight are live with an exactly zero gradient (the masked two-token softmax is a swap), so
they decay, as in the plain model.

Loss partials: the layout of ops.losses_fwd_bwd with the B*S segmentation units written as zeros and has_seg = 0 in the
reduction; loss[0] and counts[0:2] are therefore 0."""
import torch

from . import ops
from ._lib import GEMM_NT, GEMM_NN, GEMM_TN
from .engine import SEAM_MAX_H, check_hidden
from .engine_base import DROP_P, EXCLUDE_CLASS_IDX, EngineBase

AFFT_LIVE_PREFIXES = ("input_embed.", "depth_projection.", "depth_layernorm.", "fuser.blocks.0.", "fuser.norm.",
                      "fuser.modality_token", "fc.", "fc_len.")
AFFT_MAX_Q = 64                 # csrc/afft.hip: kAfftMaxQ
AFFT_MAX_HEADS = 1024           # ... kAfftMaxHeads (n_class + 1)
AFFT_LDS_BYTES = 152 * 1024     # ... kAfftMaxLds: n_query * (hidden + n_class + 1) floats
AFFT_MAX_ROWS = 2 ** 28         # B * S: unit and row indices of the chain stay in int


def chain_pays(B, S, H, Q):
    """True where the training step's tail runs as the one-launch chain (r3d_afft_head_step); False: the composed launches
    (avgpool_rows_fwd, head GEMM, losses_fwd_bwd, d_pooled GEMM, avgpool_rows_bwd).  Measured on one MI355X at hidden 128,
    8 queries, 17 classes (tools/afft_step_speed.py, profiles/afft_step_speed.json), the tail alone as a replayed graph,
    chain against composed: 19.3 us against 27.6 at (B, S) = (8, 16), 28.0 against 54.3 at (16, 256), 60.4 against 100.9
    at (8, 1142) -- the chain is ahead at every measured shape, from the shortest clip to the longest, so it is the route
    of every shape.  Wider hidden sizes, more queries and more classes were not timed; AfftEngine.use_head_chain = False
    takes the composed launches there (the suite runs both routes)."""
    return True


def is_live(name):
    return name.startswith(AFFT_LIVE_PREFIXES)


def check_afft_args(seg=False, erank_weight=0.0, parallel=False):
    """Raises ValueError for what the AFFT engine does not run; host-only."""
    if seg:
        raise ValueError("args.seg is set: model/afft.py has no 'seg' output (its branch is `if False:`, afft.py:203) and the "
                         "reference's training loop raises KeyError on it; run the AFFT baseline with seg off")
    if erank_weight != 0.0:
        raise ValueError("the effective-rank penalty (erank_weight != 0) is not built for the AFFT baseline: its Jacobi "
                         "backward is wired into FusionEngine's fuser backward only; measure_rank / --erank_report work")
    if parallel:
        raise ValueError("the AFFT baseline runs on one GPU: data-parallel and pixel-sharded steps (gradient buckets, the "
                         "duration denominator exchange, the sharded depth projection) are not built for AfftEngine")


def check_afft_shape(B, S, H, n_head, n_query, n_class):
    """Raises ValueError naming the limit unless the engine runs B clips of S frames at hidden H with n_head attention
    heads, n_query pooled rows and n_class classes.  Host arithmetic only: nothing is enqueued.  max_pos_len does not
    bound S (pos_embedding is sliced and never used, afft.py:165)."""
    check_hidden(H, n_head)
    if H > SEAM_MAX_H:
        raise ValueError(f"hidden {H} > {SEAM_MAX_H}: the plain SA-Fuser's seam kernels hold a channel row in one wave's registers")
    if B < 1 or S < 1:
        raise ValueError(f"batch {B} x {S} frames: at least one clip of at least one frame")
    if B * S > AFFT_MAX_ROWS:
        raise ValueError(f"batch {B} x {S} frames: B * S <= {AFFT_MAX_ROWS} rows (int row indices of the pooled-head chain)")
    if not 1 <= n_query <= AFFT_MAX_Q:
        raise ValueError(f"n_query {n_query}: the pooled-head chain takes 1 <= n_query <= {AFFT_MAX_Q}")
    if not 1 <= n_class < AFFT_MAX_HEADS:
        raise ValueError(f"n_class {n_class}: the pooled-head chain takes n_class + 1 <= {AFFT_MAX_HEADS} head outputs")
    need = 4 * n_query * (H + n_class + 1)
    if need > AFFT_LDS_BYTES:
        raise ValueError(f"n_query {n_query} x (hidden {H} + {n_class + 1} head outputs) floats = {need} bytes: the pooled-head "
                         f"chain keeps a clip's pooled rows and head gradients in LDS, <= {AFFT_LDS_BYTES} bytes")


class _Shape:
    """Activation / gradient workspace for one (B, S, train) shape; rgb, dep and fused under the names rankstream.BUFFERS expects."""

    def __init__(self, eng, B, S, train):
        dev, H, Q, K = eng.device, eng.H, eng.Q, eng.K
        N, BQ = B * S, B * Q
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)     # noqa: E731
        self.B, self.S, self.N, self.BQ = B, S, N, BQ
        self.rgb, self.dep, self.dep_pre = f(N, H), f(N, H), f(N, H)
        self.mean_d, self.rstd_d = f(N), f(N)
        self.x0, self.h1, self.vsw, self.x1, self.h2 = f(2 * N, H), f(2 * N, H), f(2 * N, H), f(2 * N, H), f(2 * N, H)
        self.u, self.f1 = f(2 * N, 4 * H), f(2 * N, 4 * H)
        self.x3, self.y = f(2 * N, H), f(2 * N, H)
        self.m1, self.r1, self.m2, self.r2, self.mf, self.rf = f(2 * N), f(2 * N), f(2 * N), f(2 * N), f(2 * N), f(2 * N)
        self.fused = f(N, H)
        self.pooled = f(BQ, H)
        self.actdur = f(BQ, K + 1)
        self.loss = torch.zeros(4, dtype=torch.float32, device=dev)
        self.counts = torch.zeros(4, dtype=torch.int64, device=dev)
        self.loss_ws = torch.zeros(ops.losses_ws_floats(B, S, Q), dtype=torch.float32, device=dev)
        if train:
            self.d_actdur = torch.zeros(BQ, K + 1, dtype=torch.float32, device=dev)
            self.d_pooled, self.d_fused = f(BQ, H), f(N, H)
            lnw = lambda rows: f(max(ops.layernorm_bwd_ws_floats(rows, H), 4))       # noqa: E731
            self.lnp = dict(nf=lnw(2 * N), n2=lnw(2 * N))
            self.lnp_seam = dict(n1=f(2 * N * H), dep=f(2 * N * H))    # the seam leaves one (dgamma, dbeta) partial per frame
            self.d_x3, self.d_u, self.d_h1, self.d_h2, self.d_x1, self.d_v = (
                f(2 * N, H), f(2 * N, 4 * H), f(2 * N, H), f(2 * N, H), f(2 * N, H), f(2 * N, H))
            self.d_rgb_pre, self.d_dep_pre, self.t_tok = f(N, H), f(N, H), f(N, H)
            self.drop_pool = torch.ones((2 * N * H + 15) // 16 * 16, dtype=torch.uint8, device=dev)
            self.drop = {"x0": self.drop_pool[:2 * N * H]}               # embd_drop: the model's only dropout on the path


class AfftEngine(EngineBase):
    _Shape = _Shape
    fused_loss_flow = True
    plain = True                                # (what rankstream and the tools ask a fuser engine)

    def __init__(self, module, device):
        check_afft_args(seg=bool(getattr(module.args, "seg", False)))          # (before anything is allocated)
        self.H, self.Q, self.K, self.heads = module.hidden_dim, module.n_query, module.n_class, module.n_head
        check_afft_shape(1, 1, self.H, self.heads, self.Q, self.K)
        self._init_engine(module, device, is_live)
        self.pad_idx = module.src_pad_idx
        self.P, self.D = module.depth_projection.in_features, module.input_embed.in_features
        self.ws_side = ops.GemmWorkspace(self.device)
        self.use_gemm_ln = True                 # hidden = 128: Linear + residual + LayerNorm sites as one launch (gemm_ln.hip)
        self.pair_embeddings = True             # both input projections in one launch (ops.gemm_bf3_nt_pair) where it applies
        self.depth_prec = 1                     # the two depth-projection GEMMs on the bf16 matrix cores (exact 3-way split)
        # the training step's tail as ONE launch (csrc/afft.hip) where chain_pays(); None: by shape, True / False: forced
        self.use_head_chain = None
        # fused flows (losses(tick=True) ... adamw(ticked=True)): the loss partials are reduced by one extra workgroup of the
        # AdamW launch -- w.loss / w.counts are valid after adamw(), not after losses()
        self.defer_loss_reduce = False
        self.dropout_enabled = bool(getattr(module, "r3d_dropout_enabled", True))

    # ---- what the engine does not run: refused where the caller asks for it, before any launch ---------------------------
    @property
    def erank_weight(self):
        return 0.0

    @erank_weight.setter
    def erank_weight(self, v):
        check_afft_args(erank_weight=float(v))

    def _refused_parallel(self, v):
        if v is not None:
            check_afft_args(parallel=True)

    grad_hook = property(lambda self: None, _refused_parallel)          # parallel.DataParallelStep sets these
    score_allreduce = property(lambda self: None, _refused_parallel)
    dur_den = property(lambda self: None, _refused_parallel)
    tp = property(lambda self: None, _refused_parallel)

    # ------------------------------------------------------------------------------------------------------
    def _admit(self, B, S, train):
        check_afft_shape(B, S, self.H, self.heads, self.Q, self.K)

    def _gln(self, rows, K):
        return self.use_gemm_ln and ops.gemm_ln_supported(rows, K, self.H)

    def _chain(self, w):
        return chain_pays(w.B, w.S, self.H, self.Q) if self.use_head_chain is None else bool(self.use_head_chain)

    def forward(self, feats, depth, labels, mode="train", training=False, need_grad=True):
        """feats [B,S,D] f32, depth [B,S,...] f32 (flattened to [N,P]), labels [B,S] int64 or None (only the rank stream
        reads them: the model has no key padding mask).  Returns views into the workspace: action [B,Q,K], duration [B,Q]."""
        a, H, Q, K = self.arena, self.H, self.Q, self.K
        B, S = feats.shape[0], feats.shape[1]
        N = B * S
        assert feats.is_cuda and depth.is_cuda and feats.dtype == torch.float32 and depth.dtype == torch.float32
        x_rgb, x_dep = feats.reshape(N, -1), depth.reshape(N, -1)
        assert x_rgb.shape[1] == self.D and x_dep.shape[1] == self.P, (x_rgb.shape, x_dep.shape, self.D, self.P)
        assert x_rgb.is_contiguous() and x_dep.is_contiguous()
        w = self._shape(B, S, need_grad)
        self._loss_pending = None          # (a pending loss reduction never survives into another step)
        drop = bool(training and need_grad and self.dropout_enabled)
        if drop:
            if self._drop_ready is w:     # the previous step's AdamW launch already filled the pool for this offset
                self._drop_ready = None
            else:
                ops.dropout_mask(w.drop_pool, DROP_P, self.drop_seed, self.drop_offset)
        dsc = 1.0 / (1.0 - DROP_P)
        pre = "fuser.blocks.0."
        # ---- the two input projections (:154,170); bias / ReLU / LayerNorm are the seam's
        dr = d = None
        if self.depth_prec == 1 and self.pair_embeddings:
            pr = ops.gemm_bf3_nt_pair(x_dep, a.p("depth_projection.weight"), w.dep_pre, self.ws,
                                      x_rgb, a.p("input_embed.weight"), w.rgb, self.ws_side)
            if pr is not None:
                d, dr = pr
        if dr is None:
            dr = ops.gemm(GEMM_NT, x_rgb, a.p("input_embed.weight"), w.rgb, bias=a.p("input_embed.bias"), act=1,
                          ws=self.ws_side, defer_reduce=True, prec=self.depth_prec)
        if d is None:
            d = ops.gemm(GEMM_NT, x_dep, a.p("depth_projection.weight"), w.dep_pre, bias=a.p("depth_projection.bias"),
                         ws=self.ws, defer_reduce=True, prec=self.depth_prec)
        rgb_src, ns_r = (self.ws_side.buf, dr.splitk) if dr.splitk > 1 else (w.rgb, 0)
        if d.splitk > 1:
            dep_src, ns_d, bias_d = self.ws.buf, d.splitk, a.p("depth_projection.bias")
        else:
            dep_src, ns_d, bias_d = w.dep_pre, 1, None
        # ---- the plain seam: slab sums, ReLU, depth LayerNorm + ReLU, + modality token, embd_drop, norm1 (:40-51,158,171-172)
        ops.plain_fuse_fwd(rgb_src, ns_r, a.p("input_embed.bias"), dep_src, ns_d, bias_d, a.p("depth_layernorm.weight"),
                           a.p("depth_layernorm.bias"), a.p("fuser.modality_token").view(-1), w.drop["x0"] if drop else None,
                           dsc, a.p(pre + "norm1.weight"), a.p(pre + "norm1.bias"), w.rgb, w.dep_pre, w.mean_d, w.rstd_d,
                           w.dep, w.x0, w.h1, w.m1, w.r1)
        # ---- the block in closed form (softmax([[-inf, s], [s, -inf]]) == swap), fuser.norm, token mean (:54-62)
        wv = a.p(pre + "attn.qkv.weight")[2 * H:]
        ops.gemm(GEMM_NT, w.h1, wv, w.vsw, c_row_xor=1, ws=self.ws)        # V of the OTHER modality token
        gln = self._gln(2 * N, H) and self._gln(2 * N, 4 * H)
        if gln:
            ops.gemm_ln_fwd([dict(a=w.vsw, w=a.p(pre + "attn.proj.weight"), bias=a.p(pre + "attn.proj.bias"), res1=w.x0,
                                  pre=w.x1, gamma=a.p(pre + "norm2.weight"), beta=a.p(pre + "norm2.bias"), y=w.h2, mean=w.m2,
                                  rstd=w.r2)])
        else:
            ops.gemm(GEMM_NT, w.vsw, a.p(pre + "attn.proj.weight"), w.x1, bias=a.p(pre + "attn.proj.bias"), res1=w.x0,
                     ws=self.ws)
            ops.layernorm_fwd(w.x1, a.p(pre + "norm2.weight"), a.p(pre + "norm2.bias"), w.h2, w.m2, w.r2)
        ops.gemm(GEMM_NT, w.h2, a.p(pre + "mlp.mlp.0.weight"), w.f1, bias=a.p(pre + "mlp.mlp.0.bias"), act=2, pre_out=w.u,
                 ws=self.ws)
        if gln:
            ops.gemm_ln_fwd([dict(a=w.f1, w=a.p(pre + "mlp.mlp.2.weight"), bias=a.p(pre + "mlp.mlp.2.bias"), res1=w.x1,
                                  res2=None, pre=w.x3, gamma=a.p("fuser.norm.weight"), beta=a.p("fuser.norm.bias"), y=w.y,
                                  mean=w.mf, rstd=w.rf, pair_out=w.fused)])
        else:
            ops.gemm(GEMM_NT, w.f1, a.p(pre + "mlp.mlp.2.weight"), w.x3, bias=a.p(pre + "mlp.mlp.2.bias"), res1=w.x1,
                     ws=self.ws)
            ops.layernorm_fwd(w.x3, a.p("fuser.norm.weight"), a.p("fuser.norm.bias"), w.y, w.mf, w.rf, pair_out=w.fused)
        # ---- pool + heads (:190-201); a deferred training step leaves them to the chain launch in losses()
        deferred = bool(self.defer_tail and need_grad and mode == "train")
        if not deferred:
            ops.afft_head_fwd(w.fused, self.w_head, self.b_head, w.pooled, w.actdur, B, S, Q)
        self.last = dict(w=w, x_rgb=x_rgb, x_dep=x_dep, drop=drop, mode=mode, tail_done=False, deferred=deferred)
        if self.rank_stream is not None:
            for attr, acc in self.rank_stream:
                acc.update(getattr(w, attr), labels, self.pad_idx if labels is not None else None)
        return dict(action=w.actdur[:, :K].view(B, Q, K), duration=w.actdur[:, K].view(B, Q))

    # ------------------------------------------------------------------------------------------------------
    def losses(self, past_label, target, target_dur, with_grad=True, val_mode=False, tick=False):
        """The anticipation CE, the duration loss and their counters (train_proposed_depth.py:184-213 without the seg
        branch).  with_grad and not val_mode: also d_actdur and d_fused -- one launch with pool and heads (csrc/afft.hip),
        or the composed launches where chain_pays() says so.  tick=True: the launch advances the step counter (and the
        dropout offset when dropout ran)."""
        st = self.last
        w, K, Q = st["w"], self.K, self.Q
        self._loss_pending = None
        ta = self.step_t if tick else None
        tb = self.drop_offset if (tick and st["drop"]) else None
        if with_grad and not val_mode:
            assert hasattr(w, "d_actdur"), "losses(with_grad=True) needs a forward with need_grad=True"
            if self._chain(w):
                ops.afft_head_step(w.fused, self.w_head, self.b_head, w.pooled, w.actdur, w.B, w.S, Q, past_label, target,
                                   target_dur, self.pad_idx, EXCLUDE_CLASS_IDX, w.d_actdur, w.d_fused, w.loss_ws,
                                   tick_a=ta, tick_b=tb)
                if self.defer_loss_reduce and tick:      # reduced (into the caller's running sums too) by the AdamW launch
                    acc = self.loss_acc if self.loss_acc is not None else (None, None)
                    self._loss_pending = ops.loss_finalize_job(w.loss_ws, w.B, w.S, Q, False, None, w.loss, w.counts,
                                                               acc_loss=acc[0], acc_counts=acc[1])
                else:
                    ops.losses_finalize(ops.loss_finalize_job(w.loss_ws, w.B, w.S, Q, False, None, w.loss, w.counts))
            else:
                ops.avgpool_rows_fwd(w.fused, w.pooled, w.B, w.S, Q)
                ops.gemm(GEMM_NT, w.pooled, self.w_head, w.actdur, bias=self.b_head, ws=self.ws)
                ops.losses_fwd_bwd(None, w.actdur[:, :K], w.actdur[:, K:], K + 1, past_label, target, target_dur, w.B, w.S, Q,
                                   K, self.pad_idx, EXCLUDE_CLASS_IDX, w.loss, w.counts, d_act=w.d_actdur[:, :K],
                                   d_dur=w.d_actdur[:, K:], ld_ddur=K + 1, ws=w.loss_ws, tick_a=ta, tick_b=tb)
                ops.gemm(GEMM_NN, w.d_actdur, self.w_head, w.d_pooled, ws=self.ws)
                ops.avgpool_rows_bwd(w.d_pooled, w.d_fused, w.B, w.S, Q)
            st["tail_done"] = True
            return w.loss, w.counts
        if st["deferred"]:
            st["deferred"] = False
            ops.afft_head_fwd(w.fused, self.w_head, self.b_head, w.pooled, w.actdur, w.B, w.S, Q)     # (forward deferred it)
        ops.losses_fwd_bwd(None, w.actdur[:, :K], w.actdur[:, K:], K + 1, past_label, target, target_dur, w.B, w.S, Q, K,
                           self.pad_idx, EXCLUDE_CLASS_IDX, w.loss, w.counts, val_mode=val_mode,
                           d_act=w.d_actdur[:, :K] if with_grad else None, d_dur=w.d_actdur[:, K:] if with_grad else None,
                           ld_ddur=K + 1, ws=w.loss_ws, tick_a=ta, tick_b=tb)
        return w.loss, w.counts

    # ------------------------------------------------------------------------------------------------------
    def _build_groups(self, w):
        a, H, N = self.arena, self.H, w.N
        pre = "fuser.blocks.0."
        P = [dict(a=w.d_actdur, b=w.pooled, c=self.gw_head, bias_grad=self.gb_head),
             dict(a=w.d_x3, b=w.f1, c=a.g(pre + "mlp.mlp.2.weight"), bias_grad=a.g(pre + "mlp.mlp.2.bias")),
             dict(a=w.d_u, b=w.h2, c=a.g(pre + "mlp.mlp.0.weight"), bias_grad=a.g(pre + "mlp.mlp.0.bias")),
             dict(a=w.d_x1, b=w.vsw, c=a.g(pre + "attn.proj.weight"), bias_grad=a.g(pre + "attn.proj.bias")),
             dict(a=w.d_v, b=w.h1, c=a.g(pre + "attn.qkv.weight")[2 * H:]),        # rows [0, 2H) (Q, K) stay exactly zero
             dict(a=w.d_rgb_pre, b=self.last["x_rgb"], c=a.g("input_embed.weight"), bias_grad=a.g("input_embed.bias"))]
        w.rgb_wgrad_idx = len(P) - 1
        w.wgrad_group = ops.GemmGroup(GEMM_TN, P, tile=1 if H < 256 else 2)
        w.ln_group = ops.LnFinalizeGroup([
            (w.lnp["nf"], 2 * N, H, a.g("fuser.norm.weight"), a.g("fuser.norm.bias")),
            (w.lnp["n2"], 2 * N, H, a.g(pre + "norm2.weight"), a.g(pre + "norm2.bias")),
            (w.lnp_seam["n1"], -N, H, a.g(pre + "norm1.weight"), a.g(pre + "norm1.bias")),
            (w.lnp_seam["dep"], -N, H, a.g("depth_layernorm.weight"), a.g("depth_layernorm.bias"))])
        w.rowsum_group = ops.RowsumGroup([(w.d_dep_pre, None, 1, a.g("depth_projection.bias").view(1, H)),
                                          (w.t_tok, None, 1, a.g("fuser.modality_token").view(1, H))])

    def backward(self, d_seg=None, d_actdur=None, fused_adamw=None, adamw_next=False):
        """Adjoint of forward(); gradients land in the grad arena (written, not accumulated).  d_actdur: head gradients
        handed in by the caller (the autograd route) instead of the ones losses() left."""
        assert d_seg is None and fused_adamw is None
        self.backward_main(d_actdur=d_actdur)
        self.backward_depth_wgrad()

    def backward_main(self, d_seg=None, d_actdur=None):
        st = self.last
        w, a, H, Q, ws = st["w"], self.arena, self.H, self.Q, self.ws
        pre = "fuser.blocks.0."
        if d_actdur is not None:
            if d_actdur.data_ptr() != w.d_actdur.data_ptr():
                w.d_actdur.copy_(d_actdur)
            ops.gemm(GEMM_NN, w.d_actdur, self.w_head, w.d_pooled, ws=ws)
            ops.avgpool_rows_bwd(w.d_pooled, w.d_fused, w.B, w.S, Q)
        else:
            assert st["tail_done"], "backward() follows losses(with_grad=True) or takes d_actdur"
        if not hasattr(w, "wgrad_group"):
            self._build_groups(w)
        drop = w.drop["x0"] if st["drop"] else None
        dsc = 1.0 / (1.0 - DROP_P)

        def ln_bwd(site, dy, x, mean, rstd, gname, bname, dx, **kw):
            ops.layernorm_bwd(dy, x, mean, rstd, a.p(gname), a.p(bname), dx, a.g(gname), a.g(bname), partial=w.lnp[site], **kw)

        ln_bwd("nf", w.d_fused, w.x3, w.mf, w.rf, "fuser.norm.weight", "fuser.norm.bias", w.d_x3, pair_in=True)
        ops.gemm(GEMM_NN, w.d_x3, a.p(pre + "mlp.mlp.2.weight"), w.d_u, aux=w.u, mul=2, ws=ws)
        ops.gemm(GEMM_NN, w.d_u, a.p(pre + "mlp.mlp.0.weight"), w.d_h2, ws=ws)
        ln_bwd("n2", w.d_h2, w.x1, w.m2, w.r2, pre + "norm2.weight", pre + "norm2.bias", w.d_x1, add1=w.d_x3)
        ops.gemm(GEMM_NN, w.d_x1, a.p(pre + "attn.proj.weight"), w.d_v, c_row_xor=1, ws=ws)     # un-swap
        ops.gemm(GEMM_NN, w.d_v, a.p(pre + "attn.qkv.weight")[2 * H:], w.d_h1, ws=ws)
        # norm1 backward + dropout + token partials + ReLU gates + depth LayerNorm backward: one launch
        ops.plain_fuse_bwd(w.d_h1, w.x0, w.m1, w.r1, a.p(pre + "norm1.weight"), w.d_x1, drop, dsc, w.rgb, w.dep_pre, w.mean_d,
                           w.rstd_d, a.p("depth_layernorm.weight"), a.p("depth_layernorm.bias"), w.d_rgb_pre, w.d_dep_pre,
                           w.lnp_seam["n1"], w.lnp_seam["dep"], w.t_tok)
        # ---- everything that only feeds parameter gradients: three launches
        w.wgrad_group.set_b(w.rgb_wgrad_idx, st["x_rgb"])
        w.wgrad_group.launch()
        w.ln_group.launch()
        w.rowsum_group.launch()

    def backward_depth_wgrad(self):
        """depth_projection.weight gradient [H, P] = d_dep_pre^T . depth: the last and largest kernel of the backward."""
        st = self.last
        ops.gemm(GEMM_TN, st["w"].d_dep_pre, st["x_dep"], self.arena.g("depth_projection.weight"), ws=self.ws,
                 prec=self.depth_prec)

    # ------------------------------------------------------------------------------------------------------
    def adamw(self, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, tick_dropout=False, ticked=False,
              skip_depth=False, prefill_dropout=False, before_flat=None):
        """One fused launch over the live prefix of the arena; the dead parameters are outside it.  ticked: losses(tick=True)
        already advanced the counters.  prefill_dropout: the launch also fills the workspace's dropout pool with the NEXT
        step's masks.  A loss reduction left pending by losses() rides as one more workgroup."""
        assert not skip_depth and before_flat is None
        self.set_lr(lr)
        if not ticked:
            ops.tick(self.step_t, self._tick_counter(tick_dropout))
        st = self.last
        pending, self._loss_pending = self._loss_pending, None
        prefill = prefill_dropout and st is not None and st["drop"] and (ticked or tick_dropout)
        self._adamw_flat(0, self.arena.n_live, weight_decay, betas, eps, grad_scale, loss_fin=pending,
                         prefill=st["w"] if prefill else None)

    def train_step(self, feats, depth, past_label, target_dur, target, lr, weight_decay, training=True):
        """forward + losses + backward + AdamW, all enqueued, no host sync.  Returns (loss[4], counts[4]) on device."""
        self.set_lr(lr)
        keep, self.defer_tail = self.defer_tail, True
        keep_r, self.defer_loss_reduce = self.defer_loss_reduce, True
        try:
            self.forward(feats, depth, past_label, "train", training)
            loss, counts = self.losses(past_label, target, target_dur, tick=True)
        finally:
            self.defer_tail, self.defer_loss_reduce = keep, keep_r
        self.backward(adamw_next=True)
        self.adamw(lr, weight_decay, ticked=True, prefill_dropout=True)
        return loss, counts
