"""Case table of the bf16x3 GEMM kernels (csrc/gemm_bf3.hip: tiles 7 to 12 and the pair launch) for
tests/test_gemm_bf3_cpu.py and tests/test_gemm_bf3_gpu.py.  No torch.cuda here: the table, its operand generators, its
references and the mirrors of the kernels' index arithmetic import and run on a machine without a GPU.  Every operand is
generated from a seed in the table; nothing is read from disk.

The metric.  For a product with fp32 operands A, B and `ref` the float64 product of the same fp32 values, the error of a
result X is componentwise,

    E(X) = max over elements of |X - ref| / S,     S = |A| . |B| in float64

(with alpha, accumulate or a bias S = |alpha| (|A| . |B|) + |C_init| + |bias|; for a ReLU output the pre-activation S,
elements whose reference pre-activation is within the bound of zero being held to |X| <= 2 bound S instead).  The bound
of a case is

    bound = 8 * e32 + 2^-21.

e32 is E of a float32 CPU torch.matmul of the same operands, measured against the float64 reference -- never against a
GPU kernel; 8 is the project's margin for a different summation order (rnn_wide_cases, cnn_cases).  2^-21 is derived: the
kernels split x = h + m + l by truncation, h the top 8 significand bits, m the next 8, l the last 8.  With u = 2^e the
power of two at or below |x|, the remainders x - h and x - h - m are multiples of 2^-23 u below 2^-7 u and 2^-15 u, so
|m| <= (2^-7 - 2^-23) u < 2^-7 |x| and |l| <= (2^-15 - 2^-23) u < 2^-15 |x|, and the three products the kernels drop are
bounded by
    |m_a l_b| + |l_a m_b| + |l_a l_b| <= (2 (2^-7 - 2^-23)(2^-15 - 2^-23) + (2^-15 - 2^-23)^2) u_a u_b
                                       = (2^-21 - 2^-30 - 2^-36 + 3 * 2^-46) u_a u_b < 2^-21 |a b|
(the plain 2 * 2^-22 + 2^-30 of |m| < 2^-7 |x|, |l| < 2^-15 |x| less the 2^-29 the two cross terms give back), which
summed over k is < 2^-21 S.

What the bound cannot hide (asserted by the CPU test from the references alone):
  * a K-tail case (K not a multiple of the tile's BK, or a last split shorter than the others) has POSITIVE operands,
    a, b uniform in [0.5, 1): every product lies in [0.25, 1), so one k-octet (8 products) is at least 8 * 0.25 = 2 against
    S < K -- dropping or duplicating any one octet moves every element by at least 2 / K relative to S -- and the
    case's bound is below 1 / K;
  * every other case has operands of mixed sign on both sides (randn; one row per kernel with exponents spread over
    2^-20 .. 2^20, "wide") and a bound of at most 2^-16: a dropped or mispaired KEPT term of the split (about 2^-16
    relative to |a b| where it is one-sided, as it is for the largest terms of a wide row) does not fit.
A correct kernel that misses its bound is not given a wider factor: the row goes into WIDENED with its figures.

The exactness inputs (EXACT_CASES) are products with no rounding at all -- see exact_operands."""
import functools
from collections import namedtuple

import numpy as np
import torch

NT, TN = 0, 2
BM = {7: 128, 8: 64, 9: 128, 10: 128, 11: 128, 12: 128}       # BM = BN of each tile
BK = {7: 16, 8: 64, 9: 32, 10: 32, 11: 32, 12: 32}            # k per LDS stage (tile 7: per MFMA step)
NT_TILES, TN_TILES = (8, 9, 11), (10, 12)
SLACK = 2.0 ** -21
MARGIN = 8.0
POISON = 0x7FC12345                                           # a NaN with a payload
WIDENED = []                                                  # (case id, measured E, e32, reason)


def cdiv(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------------------------------------
# mirrors of the index arithmetic (COPIES: each says which lines it copies; changed together with them)
# ----------------------------------------------------------------------------------------------------------
def nt_split(tile, K, splitk):
    """(slabs, k_per_split) ops.gemm makes of a forced `splitk` on tiles 8, 9, 11 (r3d_amd/ops.py, gemm(): `q = 64 if
    d.tile == 8 else ...` to `d.splitk < 2`); a single slab means no split, which gemm_bf3_nt_ok refuses."""
    q = 64 if tile == 8 else 32
    kps = cdiv(cdiv(K, splitk), q) * q
    return cdiv(K, kps), kps


def nt_slab_steps(tile, K, kps):
    """Per slab (k values, k-steps, octets of its last k-step): `k_begin`, `k_end`, `nk` of gemm_bf3_nt_kernel and
    gemm_bf3_nt_u_kernel (csrc/gemm_bf3.hip: `const int k_begin = split * pkps;` and the two lines after it)."""
    out = []
    for split in range(cdiv(K, kps)):
        k_begin = split * kps
        k_end = min(K, k_begin + kps)
        nk = cdiv(k_end - k_begin, BK[tile])
        out.append((k_end - k_begin, nk, (k_end - k_begin - (nk - 1) * BK[tile]) // 8))
    return out


def nt_grid(tile, M, N, ns, ns2=0):
    """(tiles G, workgroups launched, workgroups that return at `split >= NG` / `split >= s2.NG2`): launch_bf3_nt_cfg
    (`dim3(8 * tiles * r3d_cdiv(ns + s2.NG2, 8))`) and the kernel's `split = (idx / G) * 8 + (p & 7)`."""
    tiles = cdiv(M, BM[tile]) * cdiv(N, BM[tile])
    groups = cdiv(ns + ns2, 8)
    return tiles, 8 * tiles * groups, tiles * (8 * groups - ns - ns2)


def tn_grid(M, N):
    """(row tiles G, column panels NG, workgroups launched, workgroups that return at `tn >= NG`): launch_gemm_bf3_tn
    (`dim3(8 * tm * r3d_cdiv(tn, 8))`) and gemm_bf3_tn_kernel's `tn = (idx / G) * 8 + (p & 7)`."""
    tm, tn = cdiv(M, 128), cdiv(N, 128)
    return tm, tn, 8 * tm * cdiv(tn, 8), tm * (8 * cdiv(tn, 8) - tn)


def tn_steps(K):
    """(k-steps, k values of the last one): `nk = (K + BK - 1) / BK` of gemm_bf3_tn_kernel"""
    nk = cdiv(K, 32)
    return nk, K - (nk - 1) * 32


def nt_ok(tile, M, N, K, lda, ldb, splitk, kps):
    """the rules of gemm_bf3_nt_ok that need no pointer, and gemm_validate's for split-K"""
    return (splitk > 1 and K % 8 == 0 and lda % 4 == 0 and ldb % 4 == 0 and kps % (32 if tile in (9, 11) else 64) == 0
            and K >= 64 and kps % 16 == 0 and cdiv(K, kps) <= splitk and lda >= K and ldb >= K and M > 0 and N > 0)


def tn_ok(M, N, K, lda, ldb):
    """the rules of gemm_bf3_tn_ok that need no pointer"""
    return K >= 16 and M % 4 == 0 and N % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0 and lda >= M and ldb >= N


def panel_ok(M, N, K, ldb, ldc):
    """wgrad_panel_ok (csrc/gemm_f32.hip) and tile 7's extra rule in r3d_gemm_f32, without the pointers"""
    return K <= 128 and M <= 128 and N >= 2048 and N % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0


def plan_nt(M, N, K):
    """(tile, slabs, k_per_split) r3d_gemm_plan gives an aligned, unpadded NT product with prec == 1, or None where it keeps
    an fp32 tile: the admission rule (`d->prec == 1 && d->layout == R3D_GEMM_NT && (d->K >= 8192 || ...`) and the split
    arithmetic below it in csrc/gemm_f32.hip (`const long t64 = ...` to `if (ns >= 2)`)."""
    if not ((K >= 8192 or (K >= 2048 and M * N >= 256 * 256)) and K % 8 == 0):
        return None
    t64 = cdiv(M, 64) * cdiv(N, 64)
    tl = 8 if t64 <= 16 else 9
    tiles = t64 if tl == 8 else cdiv(M, 128) * cdiv(N, 128)
    ns = 256 // min(tiles, 256)
    ns = max(ns, 2)
    kps = max(cdiv(cdiv(K, ns), 64) * 64, 256)
    ns = cdiv(K, kps)
    return (tl, ns, kps) if ns >= 2 else None


def pair_split(K2, ns1, kps1):
    """(slabs, k_per_split) ops.gemm_bf3_nt_pair gives the second product beside a first one of ns1 slabs, or the reason it
    returns None (r3d_amd/ops.py, gemm_bf3_nt_pair(): `spare = -d1.splitk % 8` to `if d2.splitk < 2`)."""
    if K2 % 8 or K2 < 64:
        return "k2"
    spare = -ns1 % 8
    if spare == 0:
        return "no spare slot"
    kps2 = cdiv(cdiv(K2, spare), 64) * 64
    if kps2 > kps1:
        return "kps2 > kps1"
    ns2 = cdiv(K2, kps2)
    return (ns2, kps2) if ns2 >= 2 else "one slab"


# ----------------------------------------------------------------------------------------------------------
# a. NT tiles 8, 9, 11: forced with ops.gemm(..., prec=1, tile=t, splitk=s)
# ----------------------------------------------------------------------------------------------------------
# pad: lda = ldb = K + pad; off: the operands start `off` floats into their allocation (16-byte aligned, not its start)
# dist: pos (uniform [0.5, 1): the K-tail rows), randn, wide (randn * 2^e, e uniform in -20 .. 20)
NtCase = namedtuple("NtCase", "tile M N K splitk pad off dist tag")
_NT8 = [
    # (M, N, K, splitk, pad, off, dist, what)
    (1, 1, 72, 2, 0, 0, "pos", "min K: slabs 64 + 8, one k-step each, the last a single octet"),
    (63, 40, 128, 2, 4, 12, "randn", "slabs 64 + 64: one k-step, the last slab exactly full"),
    (64, 64, 256, 2, 0, 0, "randn", "one whole tile, two k-steps"),
    (65, 129, 264, 2, 4, 0, "pos", "slabs 192 + 72: three k-steps, then two with a one-octet tail; 2 x 3 tiles"),
    (130, 65, 512, 2, 0, 12, "randn", "four k-steps; 3 x 2 tiles"),
    (64, 257, 200, 2, 4, 0, "pos", "slabs 128 + 72; five column tiles"),
    (64, 40, 328, 5, 0, 0, "pos", "three slabs 128 + 128 + 72"),
    (65, 64, 256, 2, 0, 0, "wide", "exponents over 2^-20 .. 2^20"),
]
_NT9 = [
    (1, 1, 64, 2, 0, 0, "randn", "min K: slabs 32 + 32, one k-step, the last slab exactly full"),
    (63, 40, 72, 3, 4, 12, "pos", "slabs 32 + 32 + 8: the last a single octet"),
    (64, 64, 128, 2, 0, 0, "randn", "two k-steps"),
    (65, 129, 200, 2, 4, 0, "pos", "slabs 128 + 72: four k-steps, then three with a one-octet tail; 1 x 2 tiles"),
    (130, 257, 192, 2, 0, 12, "randn", "three k-steps; 2 x 3 tiles"),
    (128, 128, 256, 2, 4, 0, "randn", "one whole tile, four k-steps"),
    (130, 65, 104, 3, 0, 0, "pos", "slabs 64 + 40: a partial second k-step; 2 x 1 tiles"),
    (65, 64, 128, 2, 0, 0, "wide", "exponents over 2^-20 .. 2^20"),
]
NT_CASES = [NtCase(8, *r[:7], r[7]) for r in _NT8] + [NtCase(t, *r[:7], r[7]) for t in (9, 11) for r in _NT9]

# ----------------------------------------------------------------------------------------------------------
# b. TN tiles 10, 12: C window of ldc = N + 8, alpha = -0.375, accumulate on and off
# ----------------------------------------------------------------------------------------------------------
TnCase = namedtuple("TnCase", "tile M N K pad dist tag")
TN_ALPHA = -0.375
TN_LDC_PAD = 8
_TN = [
    # (M, N, K, pad, dist, what)
    (4, 4, 16, 0, "pos", "min K, M, N: one partial k-step"),
    (64, 128, 24, 4, "pos", "one partial k-step of three octets"),
    (128, 128, 32, 0, "randn", "one whole tile, one whole k-step"),
    (132, 132, 40, 4, "pos", "two k-steps, the second one octet; 2 x 2 tiles, the ragged ones four wide"),
    (128, 1028, 64, 0, "randn", "nine column panels: the second group of 8, seven workgroups return"),
    (132, 128, 96, 4, "randn", "three k-steps"),
    (64, 132, 100, 0, "pos", "four k-steps, the last four deep (half an octet)"),
    (4, 1028, 32, 4, "randn", "four rows, nine panels"),
    (132, 4, 64, 0, "randn", "four columns, two row tiles"),
    (128, 132, 64, 4, "wide", "exponents over 2^-20 .. 2^20"),
]
TN_CASES = [TnCase(t, *r[:5], r[5]) for t in TN_TILES for r in _TN]

# ----------------------------------------------------------------------------------------------------------
# c. AdamW epilogue of tiles 10, 12: (K, M, N), parameter and moments in [M, N + 8] buffers
# ----------------------------------------------------------------------------------------------------------
AdamCase = namedtuple("AdamCase", "tile K M N")
ADAM_SHAPES = [(40, 132, 132), (64, 128, 256), (16, 4, 1028)]
ADAM_CASES = [AdamCase(t, *s) for t in TN_TILES for s in ADAM_SHAPES]
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-3, grad_scale=0.25, alpha=0.5, lr=1e-3)
# (exp_avg, exp_avg_sq, parameter): rtol, atol of test_gemm_bf16x3_weight_gradient_tiled_with_adamw_epilogue
ADAM_TOL = dict(exp_avg=(1e-6, 1e-9), exp_avg_sq=(1e-6, 1e-12), parameter=(1e-6, 1e-7))

# ----------------------------------------------------------------------------------------------------------
# d. the pair launch: K1 = 8200 (33 or 26 slabs on tile 8), the second product with its own padded leading dimensions
# ----------------------------------------------------------------------------------------------------------
PairCase = namedtuple("PairCase", "M N K1 K2 pad2")
PAIR_K1 = 8200
PAIR_CASES = [PairCase(M, N, PAIR_K1, K2, 4 + 4 * (i % 2)) for (M, N) in ((8, 40), (70, 100), (130, 132))
              for i, K2 in enumerate((72, 136, 1792))]
# r3d_gemm_bf3_nt_pair called directly: (M, N, K1, K2, k_per_split of the second, what)
PAIR_DIRECT = [(8, 40, 8200, 1792, 64, "33 + 28 slabs: the second product fills a further group of 8"),
               (8, 40, 8192, 136, 64, "32 slabs: the first product ends on a group of 8")]
# ops.gemm_bf3_nt_pair returns None: (K1, K2, pair_split's reason); all at (M, N) = (8, 40)
PAIR_NONE = [(8192, 136, "no spare slot"), (8200, 2048, "kps2 > kps1"), (8200, 76, "k2"), (8200, 56, "k2")]


def case_id(c):
    n = type(c).__name__
    if n == "NtCase":
        return f"nt-t{c.tile}-{c.M}x{c.N}x{c.K}-sk{c.splitk}-p{c.pad}-o{c.off}-{c.dist}"
    if n == "TnCase":
        return f"tn-t{c.tile}-{c.M}x{c.N}x{c.K}-p{c.pad}-{c.dist}"
    if n == "AdamCase":
        return f"adam-t{c.tile}-{c.M}x{c.N}x{c.K}"
    if n == "PairCase":
        return f"pair-{c.M}x{c.N}-{c.K1}+{c.K2}"
    return f"{c.kind}-t{c.tile}-{c.side}-{c.M}x{c.N}x{c.K}-sk{c.splitk}"


def is_tail(c):
    """K is not a multiple of the tile's BK, or the last slab is shorter than the others"""
    if type(c).__name__ == "TnCase":
        return c.K % 32 != 0
    ns, kps = nt_split(c.tile, c.K, c.splitk)
    return c.K % BK[c.tile] != 0 or c.K != ns * kps


# ----------------------------------------------------------------------------------------------------------
# operands and references (host, seeded, cached: shared among the tests and never modified)
# ----------------------------------------------------------------------------------------------------------
def operand(rows, cols, dist, seed):
    g = torch.Generator().manual_seed(seed)
    if dist == "pos":
        return (torch.rand(rows, cols, generator=g) * 0.5 + 0.5).float()
    x = torch.randn(rows, cols, generator=g)
    if dist == "wide":
        x = x * torch.pow(2.0, torch.randint(-20, 21, (rows, cols), generator=g).float())
    return x.float()


Problem = namedtuple("Problem", "A B ref S e32 bound")


@functools.lru_cache(maxsize=None)
def problem(layout, M, N, K, dist, seed):
    """A, B (NT: [M, K], [N, K]; TN: [K, M], [K, N]), the float64 product, S = |A| . |B|, e32 and the bound"""
    sa, sb = ((M, K), (N, K)) if layout == NT else ((K, M), (K, N))
    A, B = operand(*sa, dist, seed), operand(*sb, dist, seed + 1)
    if layout == NT:
        ref, S, c32 = A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t(), A @ B.t()
    else:
        ref, S, c32 = A.double().t() @ B.double(), A.double().abs().t() @ B.double().abs(), A.t() @ B
    e32 = float(((c32.double() - ref).abs() / S).max())
    return Problem(A, B, ref, S, e32, MARGIN * e32 + SLACK)


def seed_of(c):
    return 1000 * c.tile + c.M + 3 * c.N + 7 * c.K


def case_problem(c):
    return problem(TN if type(c).__name__ == "TnCase" else NT, c.M, c.N, c.K, c.dist, seed_of(c))


def pair_problems(c):
    """the two products of a pair: K1 ends in a short slab (a K-tail case: positive operands); the second is a tail case
    where K2 is not a multiple of its 64-deep slabs"""
    ns1 = plan_nt(c.M, c.N, c.K1)[1]
    ns2, kps2 = pair_split(c.K2, ns1, plan_nt(c.M, c.N, c.K1)[2])
    d2 = "pos" if c.K2 != ns2 * kps2 else "randn"
    return problem(NT, c.M, c.N, c.K1, "pos", 11 + c.M), problem(NT, c.M, c.N, c.K2, d2, 13 + c.M + c.K2), d2


def pair_direct_problems(row):
    """[(problem, K, dist, is a K-tail case)] of the two products of a PAIR_DIRECT row"""
    M, N, K1, K2, kps2, _ = row
    _, ns1, kps1 = plan_nt(M, N, K1)
    out = []
    for K, tail, seed in ((K1, K1 != ns1 * kps1, 21), (K2, K2 % kps2 != 0, 22)):
        dist = "pos" if tail else "randn"
        out.append((problem(NT, M, N, K, dist, seed), K, dist, tail))
    return out


def bias_of(N, seed):
    return (torch.randn(N, generator=torch.Generator().manual_seed(seed)) * 0.25).float()


# ----------------------------------------------------------------------------------------------------------
# exactness: products without any rounding
# ----------------------------------------------------------------------------------------------------------
# kind   select  one operand is a 0/1 selection matrix, the other arbitrary finite fp32 (random sign, exponent -40 .. 40, 23
#                random mantissa bits; every 11th element all-ones mantissa, a power of two, a bf16 value): the output is the
#                selected elements.  With the arbitrary values in A this checks h, m, l of A and the pairings h.h, m.h, l.h;
#                in B, h.m and h.l.
#        short   each dot product has ONE nonzero pair, both values with 12-bit significands whose last four bits are not all
#                zero: h and m nonzero, l zero.  The 24-bit product is exact and so is every partial sum of
#                m.m + h.m + m.h + h.h (all multiples of the product's last bit and below its top).
#        single  the same with bf16-representable values: only h.h is nonzero
# side   which operand holds the arbitrary / dense values; the other is the (scaled) selection
ExactCase = namedtuple("ExactCase", "kind tile side M N K splitk")
_EX_SHAPES = {8: (65, 264, 264, 2), 9: (130, 128, 128, 2), 11: (65, 136, 136, 2),       # NT: N = K
              10: (128, 132, 128, 1), 12: (128, 260, 128, 1), 7: (128, 2048, 128, 1)}    # TN: K = M = 128
EXACT_CASES = [ExactCase(kind, t, side, *_EX_SHAPES[t]) for t in (7, 8, 9, 10, 11, 12) for kind in ("select", "short", "single")
               for side in ("A", "B")]


def _sel(i, K):
    return (37 * i + 11) % K


def _fp32(sign, expo, mant):
    return ((sign.astype(np.uint32) << 31) | ((expo + 127).astype(np.uint32) << 23) | mant.astype(np.uint32)).view(np.float32)


def exact_values(kind, rows, cols, seed):
    rng = np.random.default_rng(seed)
    n = rows * cols
    sign = rng.integers(0, 2, n)
    if kind == "select":
        expo, mant = rng.integers(-40, 41, n), rng.integers(0, 1 << 23, n)
        mant[0::11] = 0x7FFFFF
        mant[1::11] = 0
        mant[2::11] &= 0x7F0000
    elif kind == "short":
        expo = rng.integers(-20, 21, n)
        mant = ((rng.integers(0, 128, n) << 4) | rng.integers(1, 16, n)) << 12
    else:
        expo, mant = rng.integers(-20, 21, n), rng.integers(0, 128, n) << 16
    return _fp32(sign, expo, mant).reshape(rows, cols)


@functools.lru_cache(maxsize=None)
def exact_operands(c):
    """(A, B, want) as float32 numpy arrays in the layout's shapes; want = the float64 product (asserted representable by
    the CPU test).  The selection has one nonzero per output row (side B) or column (side A) of the product."""
    nt = c.tile in NT_TILES
    dense_rows, other = (c.M, c.N) if c.side == "A" else (c.N, c.M)
    dense = exact_values(c.kind, dense_rows, c.K, 17 * c.tile + len(c.kind))             # [rows, K]
    sel = np.zeros((other, c.K), np.float32)
    scale = np.ones(other, np.float32) if c.kind == "select" else exact_values(c.kind, other, 1, 5 + c.tile)[:, 0]
    sel[np.arange(other), _sel(np.arange(other), c.K)] = scale
    A, B = (dense, sel) if c.side == "A" else (sel, dense)                               # NT shapes: [M, K], [N, K]
    want = A.astype(np.float64) @ B.astype(np.float64).T
    if not nt:
        A, B = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)                      # TN shapes: [K, M], [K, N]
    return A, B, want


def split3(x):
    """the truncation split of split3_pair (csrc/gemm_bf3.hip) in numpy float32"""
    x = np.asarray(x, np.float32)
    h = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r = x - h
    m = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return h, m, r - m


def six_terms(a, b):
    """a * b as the kernels evaluate one nonzero pair: the six kept products in mfma_bf3's order ("small terms first"),
    each exact, added to an fp32 accumulator.  Returns (result, smallest nonzero |intermediate|)."""
    (ah, am, al), (bh, bm, bl) = split3(a), split3(b)
    acc = np.zeros(np.broadcast(a, b).shape, np.float32)
    small = np.inf
    for x, y in ((ah, bl), (al, bh), (am, bm), (ah, bm), (am, bh), (ah, bh)):
        p = x.astype(np.float64) * y.astype(np.float64)
        acc = (acc.astype(np.float64) + p).astype(np.float32)
        for v in (p, acc):
            nz = np.abs(v[v != 0])
            if nz.size:
                small = min(small, float(nz.min()))
    return acc, small
