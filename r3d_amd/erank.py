"""Effective rank of the fused token matrix as a differentiable op (build-side; the reference only describes the
quantity, README.md:8-14 -- SURVEY.md F1).  erank(X) = exp(-sum p log p), p = sigma / sum(sigma).

forward : batched one-sided Jacobi SVD in HIP (r3d_erank_jacobi), columns resident in one CU's LDS;
backward: dX = U diag(d erank/d sigma) V^T = Af diag(g / sigma^3) (Af^T X) with Af = X V the rotated columns the
          sweep leaves behind -- two MFMA GEMMs and a row scale, no V accumulation.
Matrices that do not fit one CU's LDS (H = 512 / 1024, large batches) take the two-level block-Jacobi kernel with the
columns in HBM (r3d_erank_blocked), same outputs, same backward.  Tall matrices of any row count take route "tall"
(ErankTall: the rows are QR-reduced to [C, C] first, the Jacobi runs on that).  A Gram route (X^T X through the LDS
kernel) is kept as a measurement-only cross-check."""
import torch

from . import ops
from ._lib import GEMM_NN, GEMM_NT, GEMM_TN


class ErankBackward:
    """dX = d(erank)/dX * gout from what the sweep left behind: A = (X V)^T, the rotated columns as rows ([C, R] for the
    decomposed orientation), sigma, stats.  With U^T = diag(1/sigma) A:

        W = U^T X  ->  W <- diag(g / sigma) (2 W - (U^T U) W)  ->  dX = U W

    i.e. U diag(g) V^T with V^T = Sigma^-1 (2 I - U^T U) U^T X: the plain V^T = Sigma^-1 U^T X lets the residual coupling
    of a small column with a large one through amplified by sigma_j / sigma_i; one Neumann term of (U^T U)^-1 removes it to
    first order (measured against fp64 autograd through svdvals: 6-8x closer at sigma_max / sigma_min = 1e4; what remains
    is the fp32 rounding of the rotated columns themselves, ~eps * sigma_max / sigma_i in direction i).  Four GEMMs, three
    row-wise kernels, all enqueued on the current stream; buffers are allocated once (the training step replays it in a
    hipGraph).  flip: the sweep ran on X^T (A is [R, C] for X [R, C]); the same products in the transposed orientation.
    A itself is only read: U^T goes to a buffer of this object's (row stride ld, A's), so a second backward over the same
    sweep -- retain_graph, or the step's backward followed by another -- sees the same A and gives the same gradient."""

    def __init__(self, R, C, flip, device, ld=None):
        self.flip, self.R, self.C = bool(flip), R, C
        k = R if flip else C                       # singular values / rows of A
        n = C if flip else R                       # length of A's rows
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)     # noqa: E731
        self.cg, self.inv, self.w, self.g, self.p = f(k), f(k), f(k, k), f(k, k), f(k, k)
        self.ut = f(k, n if ld is None else ld)[:, :n]

    def run(self, x, a_rows, sigma, stats, gout, out, accumulate, ws):
        """x [R, C]; a_rows [k, len] view (row stride may exceed len; not written); out [R, C]."""
        k = self.R if self.flip else self.C
        ops.erank_bwd_coef2(sigma, stats, gout, self.cg, self.inv, max_rank=min(self.R, self.C))
        ut = self.ut
        assert ut.shape == a_rows.shape and ut.stride(0) == a_rows.stride(0), (ut.shape, ut.stride(), a_rows.stride())
        ops.scale_rows_into(a_rows, self.inv, ut)                          # U^T = diag(1 / sigma) A
        if self.flip:
            ops.gemm(GEMM_NT, ut, x, self.w, ws=ws)                        # U^T X^T            [R, R]
        else:
            ops.gemm(GEMM_NN, ut, x, self.w, ws=ws)                        # U^T X              [C, C]
        ops.gemm(GEMM_NT, ut, ut, self.g, ws=ws)                           # U^T U
        ops.gemm(GEMM_NN, self.g, self.w, self.p, ws=ws)
        ops.erank_bwd_fix(self.w, self.p, self.cg)                         # diag(g / sigma) (2 W - (U^T U) W)
        if self.flip:
            ops.gemm(GEMM_TN, self.w, ut, out, accumulate=accumulate, ws=ws)           # (U W)^T = W^T U^T
        else:
            ops.gemm(GEMM_TN, ut, self.w, out, accumulate=accumulate, ws=ws)           # U W
        assert k == self.w.shape[0]


class _ERank(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        R, C = x.shape
        sigma = torch.empty(1, C, dtype=torch.float32, device=x.device)
        stats = torch.empty(1, 4, dtype=torch.float32, device=x.device)
        af_t = torch.empty(1, C, R, dtype=torch.float32, device=x.device)
        ops.erank_jacobi(x, sigma, stats, af_t=af_t)
        ctx.save_for_backward(x, sigma, stats, af_t)
        return stats[0, 0].clone()

    @staticmethod
    def backward(ctx, gout):
        x, sigma, stats, af_t = ctx.saved_tensors
        R, C = x.shape
        dx = torch.empty_like(x)
        ErankBackward(R, C, False, x.device).run(x, af_t[0], sigma[0], stats[0], gout.contiguous().reshape(1).float(), dx, False,
                                                 ops.GemmWorkspace(x.device))
        return dx


class _ERankBlocked(torch.autograd.Function):
    """Any size: the two-level Jacobi with the columns in HBM (r3d_erank_blocked).  Works on the orientation with the
    fewer columns (the singular values of X and X^T are the same; the gradient is transposed back)."""

    @staticmethod
    def forward(ctx, x):
        R, C = x.shape
        ctx.flip = R < C
        xx = x.t().contiguous() if ctx.flip else x
        sigma, stats, af_t = ops.erank_blocked(xx)
        ctx.save_for_backward(xx, sigma, stats, af_t)
        return stats[0].clone()

    @staticmethod
    def backward(ctx, gout):
        xx, sigma, stats, af_t = ctx.saved_tensors
        R, C = xx.shape
        dx = torch.empty_like(xx)
        ErankBackward(R, C, False, xx.device, ld=af_t.stride(0)).run(xx, af_t[:C], sigma, stats, gout.contiguous().reshape(1).float(),
                                                                     dx, False, ops.GemmWorkspace(xx.device))
        return dx.t().contiguous() if ctx.flip else dx


TALL_MAX_H = 2048                # r3d_qr_append's widest row
TALL_MAX_LANES = 64              # r3d_qr_append / r3d_qr_fold_wy: accumulators per call
FOLDS = ("wy", "column")


def check_tall_shape(N, H):
    """Raises ValueError naming the limit unless the tall route takes an [N, H] matrix.  Host-only."""
    if H < 1 or H > TALL_MAX_H:
        raise ValueError(f"tall rank route at width {H}: the streaming QR folds rows of at most {TALL_MAX_H} columns")
    if N < H:
        raise ValueError(f"tall rank route on [{N}, {H}]: it reduces rows to an [H, H] triangle and needs N >= H")
    if N * H >= 2 ** 31:
        raise ValueError(f"tall rank route on [{N}, {H}]: N * H must stay below 2^31 (the fp32 GEMM's 32-bit offsets)")


# width -> fewest rows at which the blocked fold was timed and won (tools/erank_tall_speed.py part (a))
WY_PAYS_ROWS = {128: 9600, 256: 4096, 512: 4096}


def fold_pays(N, H):
    """The fold ErankTall takes by default for an [N, H] matrix: "wy" (r3d_qr_fold_wy, the blocked compact-WY kernel) or
    "column" (r3d_qr_append, one reflector per column).  Host-only.  Measured on one MI355X (tools/erank_tall_speed.py,
    profiles/erank_tall_speed.json), R.zero_() + the fold at the same lanes, medians of 7 alternating rounds, wy against
    column: 0.276 ms against 0.635 at (9600, 128) with 50 lanes, 0.473 against 0.887 at (18272, 128) with 64, 0.467 against
    1.173 at (4096, 256) with 43, 1.447 against 2.075 at (4096, 512) with 64.  The blocked fold won at every shape timed,
    so it is taken at those widths from the fewest rows timed there on; fewer rows, widths nobody timed and widths the
    blocked kernel refuses take "column"."""
    if N >= WY_PAYS_ROWS.get(H, 2 ** 31) and ops.qr_fold_wy_supported(H):
        return "wy"
    return "column"


BASIS_EPS = 2.0 ** -40           # scale of the identity block that rides the sweep on R (a power of two: undone exactly)


class ErankTall:
    """The rank penalty of a tall matrix X [N, H], N >= H, at any N: the rows are folded into an upper-triangular
    R [H, H] with R^T R = X^T X (`lanes` accumulators, then r3d_qr_merge's tree; no square is formed), the Jacobi runs on
    R -- sigma(X) = sigma(R) -- and the gradient goes back through the [H, H] matrix M = V diag(g / sigma) V^T:

        d erank / dX = U_X diag(g) V^T = X M,       R = U_R Sigma V^T.

    X M multiplies an error of v_i along v_j by sigma_j / sigma_i, so V has to be right to rounding, not to rounding times
    the condition number.  ErankBackward's V^T = Sigma^-1 (2 I - U^T U) U^T R is not (its product U^T R cancels down to
    sigma_i: measured 2e-2 .. 4e-1 of the gradient's scale at sigma_max / sigma_min = 1e4).  So the basis rides the sweep
    itself: the Jacobi decomposes the stacked [eps I; R] (eps = 2^-40: eps^2 is far below fp32 next to any sigma^2 the
    penalty keeps, so sigma and the rotations are those of R), whose rotated columns are [eps V; R V] -- V as the product
    of the sweep's own rotations, each entry rounded relative to itself.  One first-order Gram-Schmidt step in the R^T R
    inner product, larger sigma first (r3d_erank_deflate_mask), then removes what rounding left of v_i along the vectors
    of larger sigma.  All products are the fp32 GEMMs; the cost past the fold is independent of N but for the one
    [N, H] x [H, H] product.  Buffers are allocated once and every call only enqueues on the current stream (the training
    step replays it in a hipGraph).
    Scale: eps is absolute, so unlike the effective rank itself the route asks for data of ordinary size -- sigma_max
    between about 1e-2 and 1e19 (above: qr_stream.hip's fp32 sum of squares overflows).  Then every sigma the penalty keeps
    (> 1e-6 sigma_max) has eps^2 / sigma^2 < 1e-8, below fp32.  LayerNorm / ReLU tokens are far inside; a caller with
    other data scales it first (a common factor changes neither the effective rank nor X times its gradient).
    fold: "wy" | "column" | None (fold_pays(N, H)).  lanes: None -> min(64, ceil(N / tile rows of the fold))."""

    def __init__(self, N, H, device, lanes=None, fold=None, max_sweeps=30):
        check_tall_shape(N, H)
        fold = fold_pays(N, H) if fold is None else fold
        if fold not in FOLDS:
            raise ValueError(f"fold {fold!r}: one of {FOLDS}")
        if fold == "wy" and not ops.qr_fold_wy_supported(H):
            raise ValueError(f"fold 'wy' at width {H}: r3d_qr_fold_wy takes multiples of 16 inside its LDS budget")
        tile = ops.qr_fold_wy_tile_rows(H) if fold == "wy" else ops.qr_append_tile_rows(H)
        if lanes is None:
            lanes = min(TALL_MAX_LANES, -(-N // tile))
        if not 1 <= lanes <= TALL_MAX_LANES:
            raise ValueError(f"lanes {lanes}: 1 .. {TALL_MAX_LANES}")
        self.N, self.H, self.fold, self.lanes, self.max_sweeps = N, H, fold, lanes, max_sweeps
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)     # noqa: E731
        # [eps I; lane 0; lane 1; ...]: the first two blocks are the stacked [2H, H] matrix the sweep decomposes
        self.Z = torch.zeros(lanes + 1, H, H, dtype=torch.float32, device=device)
        self.Z[0] = torch.eye(H, dtype=torch.float32, device=device) * BASIS_EPS
        self.R = self.Z[1:]
        self.blk = None
        if ops.erank_fits(2 * H, H):
            self.sigma, self.stats, self.af = f(1, H), f(1, 4), f(1, H, 2 * H)
        else:
            self.blk = ops.ErankBlockedBufs(2 * H, H, device, max_sweeps=max_sweeps)
            self.sigma, self.stats = self.blk.sigma.view(1, H), self.blk.stats.view(1, 4)
        self.cg, self.inv = f(H), f(H)
        self.unscale = torch.full((H,), 1.0 / BASIS_EPS, dtype=torch.float32, device=device)
        self.ones = torch.ones(H, dtype=torch.float32, device=device)
        self.vt, self.b, self.g, self.lm, self.p, self.vts, self.m = (f(H, H) for _ in range(7))

    @property
    def a_rows(self):
        """[H, 2H] view of the rotated columns the sweep left behind: row i = [eps v_i, R v_i]."""
        return self.blk.af_t if self.blk is not None else self.af[0]

    def forward(self, x):
        """x [N, H] (unit column stride) -> (sigma [1, H], stats [1, 4]); enqueue only."""
        assert tuple(x.shape) == (self.N, self.H), (tuple(x.shape), self.N, self.H)
        self.R.zero_()
        if self.fold == "wy":
            ops.qr_fold_wy(x, self.R)
        else:
            ops.qr_append(x, self.R)
        ops.qr_merge(self.R)
        stacked = self.Z[:2].view(2 * self.H, self.H)
        if self.blk is not None:
            ops.erank_blocked_into(stacked, self.blk)
        else:
            ops.erank_jacobi(stacked, self.sigma, self.stats, af_t=self.af, max_sweeps=self.max_sweeps)
        return self.sigma, self.stats

    def backward(self, x, gout, out, accumulate, ws):
        """out (+)= gout * d erank / dX from the last forward's R, sigma, stats and rotated columns (none of them written:
        a second backward over one forward gives the same bits)."""
        H = self.H
        ops.erank_bwd_coef2(self.sigma[0], self.stats[0], gout, self.cg, self.inv, max_rank=H)
        ops.scale_rows_into(self.a_rows[:, :H], self.unscale, self.vt)     # V^T: the rotations' own product
        ops.gemm(GEMM_NT, self.R[0], self.vt, self.b, ws=ws)               # B = R V
        ops.gemm(GEMM_TN, self.b, self.b, self.g, ws=ws)                   # B^T B = diag(sigma^2) + what is left to remove
        ops.erank_deflate_mask(self.g, self.sigma[0], self.lm)             # I + L
        ops.gemm(GEMM_NN, self.lm, self.vt, self.p, ws=ws)
        ops.erank_bwd_fix(self.vt, self.p, self.ones)                      # V^T <- (I - L) V^T
        ops.scale_rows_into(self.vt, self.cg, self.vts)                    # diag(gout g / sigma) V^T
        ops.gemm(GEMM_TN, self.vts, self.vt, self.m, ws=ws)                # M = V diag(gout g / sigma) V^T
        ops.gemm(GEMM_NN, x, self.m, out, accumulate=accumulate, ws=ws)    # dX (+)= X M


class _ERankTall(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fold):
        N, H = x.shape
        tall = ErankTall(N, H, x.device, fold=fold)
        tall.forward(x)
        ctx.tall = tall
        ctx.save_for_backward(x)
        return tall.stats[0, 0].clone()

    @staticmethod
    def backward(ctx, gout):
        x, = ctx.saved_tensors
        dx = torch.empty_like(x)
        ctx.tall.backward(x, gout.contiguous().reshape(1).float(), dx, False, ops.GemmWorkspace(x.device))
        return dx, None


def effective_rank(x, route="auto", fold=None):
    """x: [R, C] or [B, T, C] (flattened to [B*T, C]) float32 device tensor -> 0-dim tensor (differentiable).
    route: "auto" (LDS-resident kernel when the matrix fits one CU, else the blocked one), "lds", "blocked",
    "tall" (ErankTall: QR-reduce the rows, Jacobi on R; any R >= C with C <= 2048, ValueError otherwise; fold as
    ErankTall's; for data with sigma_max above about 1e-2, see ErankTall), or "gram" (X^T X through the LDS kernel:
    measurement only, squares the condition number)."""
    if x.dim() == 3:
        x = x.reshape(-1, x.shape[-1])
    x = x.contiguous().float()
    R, C = x.shape
    if route == "tall":
        check_tall_shape(R, C)
        return _ERankTall.apply(x, fold)
    if route == "auto":
        route = "lds" if ops.erank_fits(R, C) else "blocked"
    if route == "lds":
        return _ERank.apply(x)
    if route == "blocked":
        return _ERankBlocked.apply(x)
    if route == "gram":
        assert ops.erank_fits(C, C) and not (x.requires_grad and torch.is_grad_enabled())
        g = torch.empty(C, C, dtype=torch.float32, device=x.device)
        ops.gemm(GEMM_TN, x.detach(), x.detach(), g, ws=ops.GemmWorkspace(x.device))
        sigma = torch.empty(1, C, dtype=torch.float32, device=x.device)
        stats = torch.empty(1, 4, dtype=torch.float32, device=x.device)
        ops.erank_jacobi(g, sigma, stats, gram=True)
        return stats[0, 0].clone()
    raise ValueError(route)
