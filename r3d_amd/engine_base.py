"""What every engine shares, whatever its model: the flat parameter arena, the device scalars of a step, the fc | fc_len head
views, the (B, S, train) workspace cache, AdamW over the live prefix of the arena, the graph capture of a whole step -- and
the surface the training loops, optim.FlatAdamW, parallel.py and rankstream.py rely on, declared once with its defaults.
A model's forward / losses / backward sequencing lives in its own engine_*.py; nothing here knows a model."""
import torch

from . import ops

EXCLUDE_CLASS_IDX = 47          # hard-coded at train/train_proposed_depth.py:181,195
DROP_P = 0.1                    # every nn.Dropout on the path (futr_safuser_tokenfusion.py:26; transformer.py:22)


class ParamArena:
    """Flat arenas; live parameters first (AdamW touches only that prefix), depth_projection.weight last among them
    so that everything else forms one contiguous all-reduce bucket that is ready before the big weight gradient.
    live: the model's rule for the parameters that receive a gradient, name -> bool."""

    def __init__(self, named_params, device, live):
        named = list(named_params)
        self.is_live = live
        live = [(n, p) for n, p in named if self.is_live(n)]
        dead = [(n, p) for n, p in named if not self.is_live(n)]

        def key(item):
            n, p = item
            if n == "depth_projection.weight":
                return (3, 0)
            if n in ("fc.weight", "fc_len.weight"):
                return (0, 0 if n == "fc.weight" else 1)        # adjacent: [fc.weight ; fc_len.weight] = [K+1, H]
            if n in ("fc.bias", "fc_len.bias"):
                return (2, 0 if n == "fc.bias" else 1)          # adjacent: [fc.bias ; fc_len.bias] = [K+1]
            if n == "pos_embedding":
                return (2, 9)          # last of the small bucket: only its first S rows ever get a gradient (:190), so a
                                       # data-parallel step all-reduces the bucket up to row S and skips ~1 MB of zeros
            return (1, 0) if p.numel() % 4 == 0 else (2, 2)
        order = sorted(range(len(live)), key=lambda i: (key(live[i]), i))
        live = [live[i] for i in order]
        self.offsets, off = {}, 0
        for n, p in live:
            if n in ("depth_projection.weight", "pos_embedding"):
                off = (off + 3) // 4 * 4
            self.offsets[n] = (off, p.numel(), tuple(p.shape))
            off += p.numel()
        self.n_live = (off + 3) // 4 * 4
        off = self.n_live
        for n, p in dead:
            off = (off + 3) // 4 * 4
            self.offsets[n] = (off, p.numel(), tuple(p.shape))
            off += p.numel()
        self.n_total = (off + 3) // 4 * 4
        big0 = self.offsets["depth_projection.weight"][0] if "depth_projection.weight" in self.offsets else self.n_live
        self.bucket_small = (0, big0)           # (models without a depth projection: everything is the small bucket)
        self.bucket_big = (big0, self.n_live)
        self.params = torch.zeros(self.n_total, dtype=torch.float32, device=device)
        self.grads = torch.zeros(self.n_live, dtype=torch.float32, device=device)
        self.exp_avg = torch.zeros(self.n_live, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(self.n_live, dtype=torch.float32, device=device)
        self.live_names = [n for n, _ in live]
        with torch.no_grad():
            for n, p in named:
                o, k, shp = self.offsets[n]
                self.params[o:o + k].copy_(p.detach().reshape(-1).to(device=device, dtype=torch.float32))
                p.data = self.params[o:o + k].view(shp)
                p.grad = None

    def p(self, name):
        o, k, shp = self.offsets[name]
        return self.params[o:o + k].view(shp)

    def g(self, name):
        o, k, shp = self.offsets[name]
        return self.grads[o:o + k].view(shp)

    def head_views(self, K, H):
        """(w_head, gw_head, b_head, gb_head): the arena lays fc_len behind fc, so [fc.weight ; fc_len.weight] = [K + 1, H]
        is the operand of one head product (16-byte aligned: fc.weight sorts first) and [fc.bias ; fc_len.bias] its bias."""
        a = self
        o_w, o_b = a.offsets["fc.weight"][0], a.offsets["fc.bias"][0]
        assert a.offsets["fc_len.weight"][0] == o_w + K * H and a.offsets["fc_len.bias"][0] == o_b + K and o_w % 4 == 0
        return (a.params[o_w:o_w + (K + 1) * H].view(K + 1, H), a.grads[o_w:o_w + (K + 1) * H].view(K + 1, H),
                a.params[o_b:o_b + K + 1], a.grads[o_b:o_b + K + 1])

    def attach_grads(self, named_params):
        """Expose the arena gradients as p.grad views (after a fused backward) so that any torch optimiser, gradient
        clipping or inspection code sees them.  Parameters the reference leaves without a gradient keep grad=None."""
        for n, p in named_params:
            p.grad = self.g(n) if self.is_live(n) else None


class EngineBase:
    """Base of the eight engines.  The class attributes are the defaults of the shared surface: an engine overrides what it
    implements (some with a property that refuses the setting), and a caller reads them without probing."""
    last = None                     # what the last forward left for losses() / backward(): dict(w=workspace, drop=..., ...)
    # high-water mark of the pos_embedding gradient rows a backward has written: a step only writes its first S rows, so every
    # backward clears rows [S, pos_grad_rows) left by a longer earlier batch (monotone, so a step captured in a hipGraph
    # clears what any step before its capture could have written; train() re-captures when it grows)
    pos_grad_rows = 0
    dur_den = None                  # device scalar set by the data-parallel wrapper: the duration loss's global denominator
    grad_hook = None                # callable(stage) set by the data-parallel wrapper: "small_ready" / "big_ready"
    score_allreduce = None          # callable(sums fp64 [2, H]) -> global row count, set by the data-parallel wrapper
    tp = None                       # parallel.PixelShardedDepth: depth_projection tensor-parallel over pixels
    bn_sync = None                  # parallel.SyncBatchNorm, set by the data-parallel wrapper for the BN-blend variant
    rank_stream = None              # [(workspace attribute, rankstream.StreamingRank)]: fed by every forward while set
    _drop_ready = None              # workspace whose dropout pool already holds the masks of the next forward
    _loss_pending = None            # loss reduction a losses(tick=True) left to the AdamW launch that follows it directly
    loss_acc = None                 # (float64[4], int64[4]) running sums a deferred loss reduction also feeds
    defer_tail = False              # forward -> losses -> backward back to back: forward() leaves its tail to losses()
    fused_loss_flow = False         # the engine runs that flow's fusions: defer_loss_reduce, loss_acc, depth_adamw_fusable()
    rank_penalty = False            # the engine implements the effective-rank penalty: erank_route / erank_fold take effect
    erank_weight = 0.0              # > 0: total loss -= erank_weight * effective_rank(fused token matrix)
    erank_route = "jacobi"          # the penalty's decomposition: one of engine.ERANK_ROUTES
    erank_fold = None               # tall route: "wy" | "column" | None (erank.fold_pays)
    bn = False                      # the BN-blend fuser variant (its BatchNorm statistics are synchronised across ranks)
    vary = False                    # the activation-magnitude fuser variant (its selection scores are all-reduced)

    def _init_engine(self, module, device, live, named_params=None):
        """(after the engine's own admission checks, and after self.K and self.H where the model has the fc | fc_len heads)
        live, named_params: ParamArena's rule and order (default: module.named_parameters())."""
        self.module = module
        self.device = dev = torch.device(device)
        assert dev.type == "cuda", "the HIP engine needs an MI355X device (there is no CPU path)"
        ops._lib.load()
        self.arena = ParamArena(list(module.named_parameters()) if named_params is None else named_params, dev, live)
        self.ws = ops.GemmWorkspace(dev)
        self.shapes, self.graphs = {}, {}
        self.drop_seed = 0x5EED
        self.drop_offset = torch.zeros(1, dtype=torch.int64, device=dev)
        self.lr_t = torch.zeros(1, dtype=torch.float32, device=dev)         # device scalars: a captured graph sees updates
        self.step_t = torch.zeros(1, dtype=torch.int64, device=dev)
        self._lr_host = None
        if "fc_len.weight" in self.arena.offsets:
            self.w_head, self.gw_head, self.b_head, self.gb_head = self.arena.head_views(self.K, self.H)

    # ---- workspaces ---------------------------------------------------------------------------------------------------------
    def _admit(self, B, S, train):
        """Raises ValueError unless the engine runs a batch of B clips of S frames (before anything is allocated or enqueued)."""

    def _shape(self, B, S, train):
        key = (B, S, bool(train))
        if key not in self.shapes:
            self._admit(B, S, train)
            self.shapes[key] = self._Shape(self, B, S, train)
        return self.shapes[key]

    @staticmethod
    def _dm2(m, rows, cols):
        return None if m is None else m.view(rows, cols)

    @staticmethod
    def _copy_in(w, d_seg, d_actdur):
        """logit gradients handed to backward() by the caller (the autograd bridge) into the workspace's own buffers"""
        if d_seg is not None and d_seg.data_ptr() != w.d_seg.data_ptr():
            w.d_seg.copy_(d_seg)
        if d_actdur is not None and d_actdur.data_ptr() != w.d_actdur.data_ptr():
            w.d_actdur.copy_(d_actdur)

    def pos_embedding_grad(self, w):
        """pos_embedding's gradient: the column sums over the clips of d (memory + pos) into its first S rows.  The gradient is
        written, not accumulated, so the rows [S, mark) that a longer earlier batch wrote are zeroed (the reference's
        zero_grad() zeroes them); self.pos_grad_rows is that high-water mark."""
        S, g = w.S, self.arena.g("pos_embedding")
        ops.rowmod_sum(w.d_mp, S, g[0, :S])
        if S < self.pos_grad_rows:
            g[0, S:self.pos_grad_rows].zero_()
        self.pos_grad_rows = max(self.pos_grad_rows, S)

    # ---- the optimiser step -------------------------------------------------------------------------------------------------
    def set_lr(self, lr):
        """True when it enqueued a new value (on the current stream): lr lives in device memory, so a captured graph sees
        scheduler updates, and a caller that launches on another stream orders that stream behind the write."""
        if self._lr_host != float(lr):
            self.lr_t.fill_(float(lr))
            self._lr_host = float(lr)
            return True
        return False

    def _tick_counter(self, tick_dropout):
        """The dropout counter AdamW's own tick launch advances beside the step counter (None: none)."""
        return self.drop_offset if tick_dropout else None

    def _adamw_flat(self, n0, n, weight_decay, betas, eps, grad_scale=1.0, loss_fin=None, prefill=None):
        """One fused launch over the arena elements [n0, n) (the dead parameters lie behind n_live).  loss_fin: a pending loss
        reduction rides as one more workgroup.  prefill: the workspace whose dropout pool the same launch fills with the
        NEXT step's masks (valid while the next forward uses it and the dropout offset is not advanced again)."""
        a = self.arena
        kw = dict(beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay, grad_scale=grad_scale, loss_fin=loss_fin)
        if prefill is not None:
            ops.adamw_flat_dropout(a.params[n0:n], a.grads[n0:n], a.exp_avg[n0:n], a.exp_avg_sq[n0:n], self.lr_t, self.step_t,
                                   prefill.drop_pool, DROP_P, self.drop_seed, self.drop_offset, **kw)
            self._drop_ready = prefill
        else:
            ops.adamw_flat(a.params[n0:n], a.grads[n0:n], a.exp_avg[n0:n], a.exp_avg_sq[n0:n], self.lr_t, self.step_t, **kw)

    def adamw(self, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, tick_dropout=False, ticked=False,
              skip_depth=False, prefill_dropout=False, before_flat=None):
        """One fused launch over the live prefix of the arena.  ticked: losses(tick=True) already advanced the counters in
        this step.  (prefill_dropout is accepted for the loops' calling convention: every forward of an engine that inherits
        this generates its own masks.)"""
        assert not skip_depth and before_flat is None
        self.set_lr(lr)
        if not ticked:
            ops.tick(self.step_t, self._tick_counter(tick_dropout))
        self._adamw_flat(0, self.arena.n_live, weight_decay, betas, eps, grad_scale)

    def depth_adamw_fusable(self):
        """True when depth_projection.weight can be updated inside its weight-gradient kernel at a gain (FusionEngine)."""
        return False

    def _replay(self, key, batch, run, more_state=()):
        """run(bufs) -- a whole training step on the capture's own copies of `batch` -- replayed from a graph, one capture
        per key.  What the warm-up step advances (the parameters, the moments, the counters and more_state) is put back
        before the first replay."""
        g = self.graphs.get(key)
        if g is None:
            self._shape(batch[0].shape[0], batch[0].shape[1], True)       # (admission and allocation outside the capture)
            bufs = [t.clone() for t in batch]
            state = (self.arena.params, self.arena.exp_avg, self.arena.exp_avg_sq, self.step_t, self.drop_offset) + more_state
            snap = [t.clone() for t in state]
            run(bufs)                                                     # warm-up: sizes the GEMM workspaces, sets attributes
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                out = run(bufs)
            for dst, src in zip(state, snap):
                dst.copy_(src)                                            # (undo the warm-up step; a capture runs nothing)
            g = self.graphs[key] = dict(graph=graph, bufs=bufs, out=out)
        for dst, src in zip(g["bufs"], batch):
            dst.copy_(src)
        g["graph"].replay()
        return g["out"]
