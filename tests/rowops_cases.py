"""Case tables, inputs, float64 references and bounds of tests/test_rowops_cpu.py and tests/test_rowops_gpu.py: every
kernel instance and branch that csrc/rowops.hip can launch (LayerNorm forward / backward, their multi-job launches, the
batched finalize, the column / row-modulo sums single and batched, the broadcast add).

Inputs: operands randn, gamma 1 + 0.2 randn, beta 0.1 randn, dropout keep-masks Bernoulli(0.9) with drop_scale 1 / 0.9.

LayerNorm sites.  WIDTHS (every side of the EPL instance switches at 128 / 512 / 1024, the lane boundary, the admitted
maximum 2048) at 5 rows; ROWS (one block; 256 blocks of 4 rows; rows_per_block 8, 12 and 20; ragged last blocks) at H in
{8, 72}.  A case with pair_out / pair_in runs at the even neighbour r + (r & 1).  Every site runs forward, then backward
on the kernel's own mean / rstd, under three option sets: a bit pattern from PATTERNS, its complement, and a third with
no dx2 and every matrix an aligned slice.  So each flag in FLAGS is on and off at every site, and the pattern list is
chosen so that every pair of flags that can coexist does somewhere (tests/test_rowops_cpu.py asserts both).  Layouts:
dense; "aligned": each matrix the column slice [:, 4:4 + H] of a NaN-filled buffer whose rows are 16-byte multiples;
"misaligned": the same with ONE matrix (x, dy or dx in turn) moved to column 5.  Output buffers carry two guard rows.

ReLU units within rounding of the kink may land on either side.  As tests/tcn_cases.py does, they are identified from the
float64 oracle -- |gamma xhat + beta| <= KINK max|.| -- and dy and dy2 are zeroed there (under pair_in, at the pair's
row), so neither side contributes.  A condition, not a tolerance: the share stays below 1% of a case's elements
(measured: 0 to 9 units per case, at most 3e-5 of its elements).

Bounds.  y, mean, rstd, pre_out, pair mean: rtol 1e-4, atol 1e-5 element-wise; dx, dx2: rtol 1e-3, atol 1e-4 -- those of
tests/test_kernels_gpu.py, none wider.  dgamma, dbeta and every sum over rows (colsum, rowmod_sum, RowsumGroup, finalize):
max(8 e32, 2e-6 max|ref|) per case and tensor, e32 = max|f32 - f64| of the tests/rowops_oracle.py restatement run in
float32 on the same operands; 8 is the project's margin for another summation order.  All of it is computed on the CPU.
tests/test_rowops_cpu.py asserts 8 e32 <= bound element-wise for the fixed bounds too, so none is tighter than float32
allows.  No case had to be made milder.  Measured e32 per family (tests/test_rowops_cpu.py prints them):
  LayerNorm sites     y 0 .. 9.6e-7, mean 0 .. 1.2e-7, rstd 1.8e-8 .. 1.7e-5 (H = 1: rstd = 316), pair 0 .. 4.6e-7,
                      dx 0 .. 2.2e-6, dx2 0 .. 2.5e-6, dgamma 0 .. 3.6e-5, dbeta 0 .. 4.1e-5 (autograd's sums, 4100 rows)
  split-K input       pre_out 0 (one slab) .. 2.4e-6, y 3.5e-7 .. 1.1e-6, mean .. 1.0e-7, rstd .. 8.0e-8, pair .. 8.1e-7
  multi-job sites     y .. 7.6e-7, dx, dx2 .. 1.0e-6, dgamma .. 9.0e-6, dbeta .. 7.2e-6
  colsum              0 (one row) .. 3.5e-4 (4100 rows in one chain); rowmod_sum 0 .. 3.1e-4
  RowsumGroup         0 .. 2.4e-4
  finalize            0 (one pair) .. 6.9e-5 (1030 pairs)
add_rowbcast is one float32 add: compared with a tolerance of zero."""
import functools
import itertools

import torch

from tests import rowops_oracle as RO

MARGIN, SUM_FLOOR = 8.0, 2e-6
KINK, KINK_CAP = 1e-5, 0.01
FWD_TOL, DX_TOL = (1e-4, 1e-5), (1e-3, 1e-4)            # (rtol, atol)
DROP_SCALE = 1.0 / 0.9

WIDTHS = [1, 2, 63, 64, 65, 128, 129, 136, 512, 513, 1024, 1025, 2048]
WIDTH_ROWS = 5
ROWS = [1, 3, 4, 5, 1024, 1025, 2049, 4100]
ROW_WIDTHS = [8, 72]

BITS = ["dy2", "pair_in", "relu", "add1", "add2", "dgamma_none", "defer"]
FLAGS = BITS + ["dx2_mask", "dx2_nomask", "strided", "misaligned"]
EXCLUSIVE = {frozenset(("dx2_mask", "dx2_nomask"))}
# one 8-bit pattern per site (bit 7: which of the pair takes the mask; the misaligned layout alternates with the site);
# the third case of site i takes pattern i + 1 rotated by 3
PATTERNS = [0x00, 0x53, 0x2c, 0x95, 0x6a, 0x36, 0xc9, 0x1b, 0xe4, 0x71, 0x8e, 0x47, 0xb8, 0x0f, 0xf0, 0x33, 0xcc, 0x5a, 0xa5, 0x69, 0x96]


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


def even(r):
    return r + (r & 1)


def sites():
    """[(rows, H)]: the widths at WIDTH_ROWS, then the row counts at each of ROW_WIDTHS in turn"""
    return [(WIDTH_ROWS, H) for H in WIDTHS] + [(r, ROW_WIDTHS[i % 2]) for i, r in enumerate(ROWS)]


def _options(bits, dx2, layout, off):
    o = {n: bool(bits >> i & 1) for i, n in enumerate(BITS)}
    o.update(dx2=dx2, layout=layout, off=off)
    return o


def flags_of(o):
    """the FLAGS that case options o switch on"""
    f = {n for n in BITS if o[n]}
    if o["dx2"]:
        f.add("dx2_" + o["dx2"])
    if o["layout"] != "dense":
        f.add("strided")
    if o["layout"] == "misaligned":
        f.add("misaligned")
    return f


def ln_cases():
    """[(id, rows, H, options, site index)]: three per site"""
    out = []
    S = sites()
    assert len(PATTERNS) == len(S)
    for i, (rows, H) in enumerate(S):
        p = PATTERNS[i]
        q = PATTERNS[(i + 1) % len(S)]
        q = ((q << 3) | (q >> 4)) & 0x7f
        swap = bool(p & 0x80)
        off = ("x", "dy", "dx")[i % 3]
        lay = ("misaligned", "dense") if i % 2 == 0 else ("dense", "misaligned")
        trio = [_options(p & 0x7f, "nomask" if swap else "mask", lay[0], off),
                _options(~p & 0x7f, "mask" if swap else "nomask", lay[1], off),
                _options(q, None, "aligned", off)]
        for k, o in enumerate(trio):
            r = even(rows) if o["pair_in"] else rows
            out.append((f"r{r}-H{H}-{'abc'[k]}", r, H, o, i))
    return out


LN_CASES = ln_cases()
LN_IDS = [c[0] for c in LN_CASES]


def layout_of(o, name, H):
    """(ld, c0) of matrix `name` under options o; None: dense"""
    if o["layout"] == "dense":
        return None
    ld = (H + 3) // 4 * 4 + 8
    return (ld, 5 if (o["layout"] == "misaligned" and name == o["off"]) else 4)


def elem_ok(err, ref, tol, margin=1.0):
    """margin |err| <= atol + rtol |ref| element-wise; returns the largest ratio"""
    lim = tol[1] + tol[0] * ref.abs()
    return float((margin * err / lim).max()) if err.numel() else 0.0


def sum_bound(f32, f64):
    e32 = float((f32.double() - f64).abs().max()) if f64.numel() else 0.0
    return max(MARGIN * e32, SUM_FLOOR * float(f64.abs().max())), e32


def _ln_build(rows, H, o, s):
    """inputs (float32, CPU), the float64 reference `ref`, the float32 restatement `ref32`, the kink share"""
    x, gamma, beta = rnd(rows, H, seed=s + 1), 1 + 0.2 * rnd(H, seed=s + 2), 0.1 * rnd(H, seed=s + 3)
    drows = rows // 2 if o["pair_in"] else rows
    t = dict(x=x, gamma=gamma, beta=beta, dy=rnd(drows, H, seed=s + 4),
             dy2=rnd(drows, H, seed=s + 5) if o["dy2"] else None,
             add1=rnd(rows, H, seed=s + 6) if o["add1"] else None, add2=rnd(rows, H, seed=s + 7) if o["add2"] else None,
             mask=(torch.rand(rows, H, generator=torch.Generator().manual_seed(s + 8)) < 0.9).to(torch.uint8) if o["dx2"] == "mask" else None)
    near = 0
    if o["relu"]:
        with torch.no_grad():
            v = RO.ln_fwd(x, gamma, beta, torch.float64)["v"]
        k = v.abs() <= KINK * float(v.abs().max())
        near = int(k.sum())
        if o["pair_in"]:
            k = k.view(rows // 2, 2, H).any(1)
        t["dy"] = t["dy"].masked_fill(k, 0.0)
        if t["dy2"] is not None:
            t["dy2"] = t["dy2"].masked_fill(k, 0.0)
    kw = dict(dy2=t["dy2"], pair_in=o["pair_in"], relu=o["relu"], add1=t["add1"], add2=t["add2"], mask=t["mask"], drop_scale=DROP_SCALE)
    ref, ref32 = {}, {}
    for dtype, dst in ((torch.float64, ref), (torch.float32, ref32)):
        with torch.no_grad():
            f = RO.ln_fwd(x, gamma, beta, dtype, relu=o["relu"], pair=o["pair_in"])
        dst.update({n: f[n] for n in ("y", "mean", "rstd")})
        if o["pair_in"]:
            dst["pair"] = f["pair"]
        b = RO.ln_bwd(t["dy"], x, gamma, beta, dtype, **kw)
        dst.update(dx=b["dx"], dgamma=b["dgamma"], dbeta=b["dbeta"])
        if o["dx2"]:
            dst["dx2"] = b["dx2"]
    return dict(rows=rows, H=H, o=o, t=t, kw=kw, ref=ref, ref32=ref32, kink_share=near / float(rows * H))


@functools.lru_cache(maxsize=None)
def ln_problem(cid):
    _, rows, H, o, _ = LN_CASES[LN_IDS.index(cid)]
    return _ln_build(rows, H, o, 1000 * LN_IDS.index(cid))


LN_FWD_TENSORS = ("y", "mean", "rstd", "pair")
LN_SUM_TENSORS = ("dgamma", "dbeta")


def ln_tol(name):
    return FWD_TOL if name in LN_FWD_TENSORS or name == "pre" else DX_TOL


# ---------------------------------------------------------------------------------------------------------------------
# split-K forward input
# ---------------------------------------------------------------------------------------------------------------------
SPLITK_NSPLIT = [1, 5, 8, 9, 16, 17]
SPLITK_H = [128, 264]
SPLITK_ROWS = 10                                  # 3 blocks of 4 rows, the last ragged; paired: 5 units, 2 blocks
SPLITK_VARIANTS = list(itertools.product([False, True], repeat=3))        # (bias, pre_out, pair_out)


@functools.lru_cache(maxsize=None)
def splitk_problem(nsplit, H, bias, relu, pair):
    s = 77000 + 100 * nsplit + H
    x, b = rnd(nsplit, SPLITK_ROWS, H, seed=s), (rnd(H, seed=s + 1) if bias else None)
    gamma, beta = 1 + 0.2 * rnd(H, seed=s + 2), 0.1 * rnd(H, seed=s + 3)
    out = {}
    with torch.no_grad():
        for dtype, k in ((torch.float64, "ref"), (torch.float32, "ref32")):
            f = RO.ln_fwd(x, gamma, beta, dtype, nsplit=nsplit, bias=b, relu=relu, pair=pair)
            out[k] = {n: f[n] for n in ("pre", "y", "mean", "rstd") + (("pair",) if pair else ())}
    return dict(x=x, bias=b, gamma=gamma, beta=beta, **out)


# ---------------------------------------------------------------------------------------------------------------------
# multi-job launches: jobs of equal width, unequal row counts
# ---------------------------------------------------------------------------------------------------------------------
MULTI_ROWS = (8, 1030, 64, 2)                     # 2, 129 (rows_per_block 8, ragged), 16 and 1 blocks
MULTI_H = [128, 264]
# per job: options of its forward / backward
MULTI_OPTS = [dict(dy2=True, add1=True), dict(relu=True, add2=True), dict(pair_in=True), dict(dx2="mask", dy2=True, add2=True)]


def _deferred(**on):
    """dense options with the finalize deferred, plus what `on` switches on"""
    o = dict(dict.fromkeys(BITS, False), dx2=None, layout="dense", off="x")
    o.update(on, defer=True)
    return o


def multi_cases():
    return [(n, H) for H in MULTI_H for n in (1, 2, 3, 4)]


@functools.lru_cache(maxsize=None)
def multi_job(j, H):
    """job j of the multi-job table at width H, as an ln_problem-shaped dict"""
    return _ln_build(MULTI_ROWS[j], H, _deferred(**MULTI_OPTS[j]), 55000 + 10 * H + 100 * j)


# ---------------------------------------------------------------------------------------------------------------------
# batched finalize: rows = -n means n partial pairs
# ---------------------------------------------------------------------------------------------------------------------
FIN_PAIRS = [1, 2, 4, 12, 13, 15, 16, 17, 31, 32, 33, 1030]      # around the 4-wave x 4-chain loop (p + 12 < blocks)
FIN_WIDTHS = [8, 1032, 72]                                      # cycled over the jobs: widths mixed under one max_H
FIN_LN = [(4, 8), (1030, 72), (4100, 8)]                        # rows > 0: one block (a no-op), 129 and 205 blocks


@functools.lru_cache(maxsize=None)
def fin_ln_problem(rows, H):
    """a plain LayerNorm site whose backward leaves its partial pairs for the batched finalize"""
    return _ln_build(rows, H, _deferred(), 66000 + rows + H)


def fin_jobs():
    return [(n, FIN_WIDTHS[i % 3]) for i, n in enumerate(FIN_PAIRS)]


@functools.lru_cache(maxsize=None)
def fin_problem(n, H):
    ws = rnd(n, 2, H, seed=88000 + n)
    r64, r32 = RO.finalize(ws, torch.float64), RO.finalize(ws, torch.float32)
    return dict(ws=ws, ref=dict(dgamma=r64[0], dbeta=r64[1]), ref32=dict(dgamma=r32[0], dbeta=r32[1]))


# ---------------------------------------------------------------------------------------------------------------------
# RowsumGroup: (rows, cols, mod, src2, how)
#   rows: an int, or "16m" / "16m+3" (16 mod and 16 mod + 3: the 16 row-lanes all busy, and a ragged turn)
#   how:  "vec" (16-byte path: cols % 4 == 0, every ld % 4 == 0, pointers on 16 bytes; ld > cols throughout), "cols" (cols % 4
#         != 0), "odd_ld1" / "odd_ld2" / "odd_ldd", "off_src1" / "off_src2" / "off_dst" (that pointer 4 bytes past a 16-byte
#         boundary): the three ways onto the scalar path, each alone
# ---------------------------------------------------------------------------------------------------------------------
RS_MODS, RS_COLS = [1, 5, 8, 37], [1, 17, 64, 136, 272, 513]
RS_GROUPS = [
    [(4100, 64, 1, False, "vec")],
    [("16m", 136, 5, True, "vec"), (7, 17, 8, False, "cols")],
    [("16m+3", 272, 37, True, "vec"), (1, 513, 5, True, "cols"), (4100, 1, 1, False, "cols")],
    [(4100, 136, 8, True, "off_src2"), (7, 64, 37, False, "vec"), ("16m", 272, 1, True, "odd_ld1"), ("16m+3", 64, 5, False, "off_dst")],
    [(1, 64, 1, True, "vec"), (4100, 17, 37, True, "cols"), ("16m+3", 513, 8, False, "cols"), ("16m", 64, 8, True, "odd_ld2"),
     (7, 136, 5, False, "off_src1")],
    [("16m", 64, 37, False, "odd_ldd"), (7, 272, 8, True, "vec"), ("16m+3", 136, 1, False, "vec"), (1, 17, 37, False, "cols"),
     (4100, 513, 5, True, "cols"), ("16m+3", 1, 8, True, "cols")],
]
RS_HOWS = ["vec", "cols", "odd_ld1", "odd_ld2", "odd_ldd", "off_src1", "off_src2", "off_dst"]


def rs_rows(rows, mod):
    return {"16m": 16 * mod, "16m+3": 16 * mod + 3}.get(rows, rows)


def rs_layout(cols, how):
    """{src1 | src2 | dst: (ld, c0)}; c0 is counted from a 16-byte aligned buffer start"""
    ld = (cols + 3) // 4 * 4 + 8
    lay = {n: [ld, 4] for n in ("src1", "src2", "dst")}
    if how.startswith("odd_ld"):
        lay[{"1": "src1", "2": "src2", "d": "dst"}[how[-1]]][0] = ld + 5
    if how.startswith("off_"):
        lay[how[4:]][1] = 5
    return {n: tuple(v) for n, v in lay.items()}


def rs_takes_vector_path(cols, src2, how):
    """the kernel's own flag, restated from the layout"""
    lay = rs_layout(cols, how)
    names = ["src1", "dst"] + (["src2"] if src2 else [])
    return cols % 4 == 0 and all(lay[n][0] % 4 == 0 and lay[n][1] % 4 == 0 for n in names)


@functools.lru_cache(maxsize=None)
def rs_problem(g, k):
    rows, cols, mod, src2, how = RS_GROUPS[g][k]
    rows = rs_rows(rows, mod)
    s = 99000 + 100 * g + 10 * k
    x1, x2 = rnd(rows, cols, seed=s), (rnd(rows, cols, seed=s + 1) if src2 else None)
    return dict(rows=rows, cols=cols, mod=mod, how=how, x1=x1, x2=x2, ref=RO.rowmod_sum(x1, x2, mod, torch.float64),
                ref32=RO.rowmod_sum(x1, x2, mod, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# colsum / rowmod_sum / add_rowbcast
# ---------------------------------------------------------------------------------------------------------------------
SUM_ROWS = [1, 64, 65, 129, 2048, 2049, 4100]       # colsum: 1, 1, 2, 3, 32, 32 (of 65 rows, last short) and 32 chunks
COLSUM_COLS = [1, 63, 64, 65, 513]
ROWMOD_MODS, ROWMOD_COLS = [1, 5, 4200], [17, 257]


@functools.lru_cache(maxsize=None)
def colsum_problem(rows, cols):
    x, out0 = rnd(rows, cols, seed=rows * 7 + cols), rnd(cols, seed=rows * 7 + cols + 1)
    return dict(x=x, out0=out0, ref=RO.colsum(x, torch.float64), ref32=RO.colsum(x, torch.float32),
                ref_acc=RO.colsum(x, torch.float64, out0), ref32_acc=RO.colsum(x, torch.float32, out0))


@functools.lru_cache(maxsize=None)
def rowmod_problem(rows, cols, mod):
    x, out0 = rnd(rows, cols, seed=rows * 11 + cols + mod), rnd(mod, cols, seed=rows * 11 + cols + mod + 1)
    return dict(x=x, out0=out0, ref=RO.rowmod_sum(x, None, mod, torch.float64), ref32=RO.rowmod_sum(x, None, mod, torch.float32),
                ref_acc=RO.rowmod_sum(x, None, mod, torch.float64, out0), ref32_acc=RO.rowmod_sum(x, None, mod, torch.float32, out0))


# (rows, cols, mod, x present, in place, strided)
BCAST_CASES = [(24, 40, 8, True, False, False), (24, 40, 8, False, False, False), (24, 40, 8, True, True, True), (24, 40, 24, True, False, True),
               (1030, 260, 8, True, False, True), (1030, 260, 1030, True, True, False), (1030, 260, 1030, False, False, True),
               (1030, 260, 8, True, True, False)]
BCAST_GRID_ELEMENTS = 1024 * 256                     # past it the kernel's grid-stride loop takes a second turn


# ---------------------------------------------------------------------------------------------------------------------
# the block-count rule, as engine.py's as_rowsum and the batched finalize kernel state it
# ---------------------------------------------------------------------------------------------------------------------
def blocks_as_rowsum(rows):
    rpb = max(4, ((rows + 255) // 256 + 3) // 4 * 4)
    return (rows + rpb - 1) // rpb


def blocks_finalize_kernel(rows):
    rpb = ((rows + 255) // 256 + 3) // 4 * 4
    if rpb < 4:
        rpb = 4
    return -rows if rows < 0 else (rows + rpb - 1) // rpb
