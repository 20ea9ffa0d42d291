"""The effective-rank Jacobi over every shape the rank penalty admits: the kernel instances of r3d_erank_jacobi_warm (the LDS
kernel) and r3d_erank_blocked_t (the two-level kernel, columns in HBM), and the training-step shapes that reach them.
tests/test_erank_admission_cpu.py checks every row's plan and route against the host-side queries (ops.erank_plan,
ops.erank_fits, engine.check_erank_shape) and that the rows reach every instance the plan query can return;
tests/test_erank_shapes_gpu.py runs every row against float64.

MATRICES -- one [R, C] matrix through the kernel directly.  Columns:
  route    -- "lds" (ops.erank_jacobi), "warm" (ops.erank_jacobi_warm: the right basis rides along) or "blocked"
              (ops.erank_blocked_into);
  plan     -- the instance the launcher takes, as ops.erank_plan reports it: for "lds" / "warm" (level, G, NCH, EXACT) --
              level 0 is the general pair order, 1 the level order; for "blocked" (b, NCH, EXACT, nreal, nblk);
  spectrum -- "sep": singular values prescribed through QR, linspace(0.2, 2.0) (well separated); "clu": clusters of four
              0.1 % apart, sigma_max / sigma_min = 1e4 (tests/test_kernels_gpu.py::test_erank_clustered_and_ill_conditioned_spectra);
  layout   -- "plain" (contiguous), "ld" (row stride ld > C: a column slice of a wider matrix), "xt" (blocked: the kernel is
              handed X^T, x_transposed), ("batch", n, extra) (LDS: n matrices, batch stride padded by `extra` rows).

STEPS -- one training step of futr_safuser_tokenfusion.FUTR (Q = 8, one decoder layer, n_class 17) with erank_weight 0.05.
The fused token matrix is [N = B * S, H].  Columns:
  route  -- "lds" (one CU's LDS) or "blocked"; flip -- the blocked sweep runs on fused^T (N < H);
  plan   -- as above, of the matrix the sweep decomposes ([N, H], or [H, N] when flipped);
  warm   -- erank_warm_start is set; used -- the warm basis is actually taken (ops.erank_fits_warm);
  chain  -- the backward goes through the fused hidden-128 chain kernel (the penalty's gradient is handed over as d_extra);
  check  -- "model": every parameter gradient against the float64 CPU oracle; "fused": the effective rank and the penalty's
            gradient with respect to the fused tokens only (against float64 autograd through svdvals of w.fused);
  refuse -- None (admitted) or a fragment of the ValueError message."""
import collections

Matrix = collections.namedtuple("Matrix", "R C route plan spectrum layout why")
Step = collections.namedtuple("Step", "B S H heads pad route flip plan warm used chain check refuse why")

K = 17
Q = 8
LAM = 0.05


def _m(R, C, route, plan, spectrum="sep", layout="plain", why=""):
    return Matrix(R, C, route, tuple(plan), spectrum, layout, why)


MATRICES = [
    # ---- LDS kernel, level order (power-of-two C in 32..128, R a multiple of 64 up to 512)
    _m(64, 32, "lds", (1, 8, 2, 1), why="level order, 8 lanes, NCH 2"),
    _m(128, 64, "lds", (1, 8, 4, 1), why="level order, 8 lanes, NCH 4"),
    _m(128, 128, "lds", (1, 8, 4, 1), "clu", why="level order on a clustered spectrum"),
    _m(256, 128, "lds", (1, 8, 8, 1), why="level order, 8 lanes, NCH 8 (R / 64 = 4)"),
    _m(512, 64, "lds", (1, 16, 8, 1), why="level order, 16 lanes (R / 64 = 8)"),
    _m(64, 128, "lds", (1, 8, 2, 1), layout=("batch", 3, 5), why="level order, batch of 3, padded batch stride"),
    # ---- LDS kernel, general order, 16-lane groups (C >= 33)
    _m(8, 1024, "lds", (0, 16, 1, 0), why="R << C: rank 8, 1016 sigma must come out 0"),
    _m(16, 2048, "lds", (0, 16, 1, 0), why="widest LDS matrix: rank 16 of 2048 columns"),
    _m(63, 33, "lds", (0, 16, 1, 1), why="EXACT with R not a multiple of 4, odd C (dummy player)"),
    _m(100, 50, "lds", (0, 16, 2, 0), why="G16 NCH 2"),
    _m(128, 96, "lds", (0, 16, 2, 1), why="G16 NCH 2 EXACT, C not a power of two"),
    _m(192, 128, "lds", (0, 16, 4, 0), why="R / 64 = 3 has no level-order instance: general order"),
    _m(255, 99, "lds", (0, 16, 4, 1), why="G16 NCH 4 EXACT, R % 4 = 3, odd C"),
    _m(316, 128, "lds", (0, 16, 8, 0), why="the LDS byte bound exactly at C = 128"),
    _m(316, 128, "lds", (0, 16, 8, 0), "clu", why="LDS byte bound, clustered spectrum"),
    _m(512, 48, "lds", (0, 16, 8, 1), why="G16 NCH 8 EXACT"),
    _m(600, 64, "lds", (0, 16, 0, 0), why="G16 generic NCH 0 (any length)"),
    _m(600, 64, "lds", (0, 16, 0, 0), "clu", why="G16 NCH 0 on a clustered spectrum"),
    _m(100, 50, "lds", (0, 16, 2, 0), layout=("batch", 2, 3), why="general order, batch of 2, padded batch stride"),
    _m(130, 70, "lds", (0, 16, 4, 0), layout="ld", why="row stride ld > C"),
    # ---- LDS kernel, 64-lane groups (C <= 32)
    _m(40, 24, "lds", (0, 64, 1, 0), why="G64 NCH 1"),
    _m(256, 24, "lds", (0, 64, 1, 1), why="G64 NCH 1 EXACT"),
    _m(300, 17, "lds", (0, 64, 2, 0), why="G64 NCH 2, odd C"),
    _m(512, 20, "lds", (0, 64, 2, 1), why="G64 NCH 2 EXACT"),
    _m(1000, 31, "lds", (0, 64, 4, 0), why="G64 NCH 4, odd C"),
    _m(1024, 30, "lds", (0, 64, 4, 1), why="G64 NCH 4 EXACT"),
    _m(1500, 16, "lds", (0, 64, 8, 0), why="G64 NCH 8"),
    _m(2048, 12, "lds", (0, 64, 8, 1), why="G64 NCH 8 EXACT"),
    _m(4000, 8, "lds", (0, 64, 0, 0), why="G64 generic NCH 0"),
    _m(4000, 8, "lds", (0, 64, 0, 0), "clu", why="G64 NCH 0 on a clustered spectrum"),
    _m(10000, 3, "lds", (0, 64, 0, 0), why="10000-long columns, C = 3 (dummy player)"),
    # ---- LDS kernel carrying the right basis (warm start; never the level order)
    _m(20, 33, "warm", (0, 16, 1, 0), why="warm G16 NCH 1, R < C"),
    _m(50, 40, "warm", (0, 16, 2, 0), why="warm G16 NCH 2"),
    _m(64, 64, "warm", (0, 16, 2, 1), why="warm G16 NCH 2 EXACT (basis chunks included)"),
    _m(128, 96, "warm", (0, 16, 4, 0), why="warm G16 NCH 4"),
    _m(192, 64, "warm", (0, 16, 4, 1), why="warm G16 NCH 4 EXACT"),
    _m(200, 64, "warm", (0, 16, 8, 0), why="warm G16 NCH 8: cfg2-like tokens"),
    _m(448, 64, "warm", (0, 16, 8, 1), why="warm G16 NCH 8 EXACT"),
    _m(480, 40, "warm", (0, 16, 0, 0), why="warm G16 NCH 0"),
    _m(70, 30, "warm", (0, 64, 1, 0), why="warm G64 NCH 1"),
    _m(400, 20, "warm", (0, 64, 2, 0), why="warm G64 NCH 2"),
    _m(800, 24, "warm", (0, 64, 4, 0), why="warm G64 NCH 4"),
    _m(1500, 16, "warm", (0, 64, 8, 0), why="warm G64 NCH 8"),
    _m(3000, 8, "warm", (0, 64, 0, 0), why="warm G64 NCH 0"),
    # ---- two-level (blocked) kernel
    _m(130, 70, "blocked", (16, 1, 0, 5, 6), why="b 16 NCH 1, odd nreal (dummy block)"),
    _m(100, 5, "blocked", (16, 1, 0, 1, 2), why="C < b: one real block and the dummy"),
    _m(256, 100, "blocked", (16, 1, 1, 7, 8), why="b 16 NCH 1 EXACT, odd nreal"),
    _m(300, 200, "blocked", (16, 2, 0, 13, 14), why="b 16 NCH 2, odd nreal"),
    _m(512, 512, "blocked", (16, 2, 1, 32, 32), "clu", why="b 16 NCH 2 EXACT, clustered (19 sweeps measured)"),
    _m(509, 40, "blocked", (16, 2, 1, 3, 4), why="EXACT with R % 4 = 1 (zero row tail)"),
    _m(1000, 64, "blocked", (16, 4, 0, 4, 4), why="b 16 NCH 4"),
    _m(1024, 100, "blocked", (16, 4, 1, 7, 8), why="b 16 NCH 4 EXACT"),
    _m(1196, 128, "blocked", (16, 8, 0, 8, 8), why="b 16 NCH 8, last R with 16-column blocks"),
    _m(1197, 128, "blocked", (8, 8, 0, 16, 16), why="b 8 NCH 8 with R != 2048, first R with 8-column blocks"),
    _m(1197, 128, "blocked", (8, 8, 0, 16, 16), "clu", why="8-column blocks, clustered"),
    _m(2048, 256, "blocked", (8, 8, 1, 32, 32), why="b 8 NCH 8 EXACT"),
    _m(2396, 100, "blocked", (8, 0, 0, 13, 14), why="b 8 generic NCH 0, last R with 8-column blocks"),
    _m(2397, 60, "blocked", (4, 0, 0, 15, 16), why="4-column blocks, first R"),
    _m(2500, 64, "blocked", (4, 0, 0, 16, 16), "clu", why="4-column blocks, clustered"),
    _m(4796, 30, "blocked", (4, 0, 0, 8, 8), why="4-column blocks, last R"),
    _m(4797, 33, "blocked", (2, 0, 0, 17, 18), why="2-column blocks, first R, odd nreal"),
    _m(5000, 32, "blocked", (2, 0, 0, 16, 16), "clu", why="2-column blocks, clustered"),
    _m(9596, 64, "blocked", (2, 0, 0, 32, 32), why="the blocked bound exactly"),
    _m(600, 150, "blocked", (16, 4, 0, 10, 10), layout="xt", why="input handed transposed (x_transposed)"),
    _m(700, 90, "blocked", (16, 4, 0, 6, 6), layout="ld", why="row stride ld > C"),
]


def _s(B, S, H, heads=8, pad="tail", route="lds", flip=False, plan=(), warm=False, used=False, chain=False, check="model",
       refuse=None, why=""):
    return Step(B, S, H, heads, pad, route, flip, tuple(plan), warm, used, chain, check, refuse, why)


STEPS = [
    _s(79, 4, 128, plan=(0, 16, 8, 0), why="last LDS row count at H = 128 (N = 316), composed path (B Q % 16 != 0)"),
    _s(78, 4, 128, plan=(0, 16, 8, 0), chain=True, why="the largest N <= 316 the chain takes (N = 312): LDS on the chain"),
    _s(4, 79, 128, plan=(0, 16, 8, 0), why="the LDS boundary with long clips, composed path"),
    _s(10, 32, 128, route="blocked", plan=(16, 2, 0, 8, 8), chain=True,
       why="N = 320, first blocked row at H = 128, on the chain (penalty gradient as d_extra)"),
    _s(5, 64, 128, route="blocked", plan=(16, 2, 0, 8, 8), why="N = 320 blocked on the composed path"),
    _s(4, 700, 64, route="blocked", plan=(4, 0, 0, 16, 16), check="fused", why="4-column blocks in the step"),
    _s(8, 1199, 128, route="blocked", plan=(2, 0, 0, 64, 64), chain=True, check="fused",
       why="2-column blocks near the bound, on the chain"),
    _s(11, 872, 2048, 16, route="blocked", plan=(2, 0, 0, 1024, 1024), check="fused",
       why="admission corner: 9592 x 2048, 1024 blocks"),
    _s(1, 8, 1024, why="wide LDS: rank <= 8, 1016 sigma must be 0", plan=(0, 16, 1, 0)),
    _s(2, 8, 2048, 16, plan=(0, 16, 1, 0), why="widest LDS token matrix (16 x 2048)"),
    _s(2, 9, 2048, 16, route="blocked", flip=True, plan=(8, 8, 1, 3, 4), why="flip at H = 2048, odd nreal (dummy block)"),
    _s(1, 933, 2048, 16, pad="none", route="blocked", flip=True, plan=(8, 8, 1, 117, 118), check="fused",
       why="longest admitted clip at H = 2048, flipped, odd nreal"),
    _s(1, 520, 512, pad="none", route="blocked", plan=(16, 4, 0, 32, 32), why="no flip, N just above H"),
    _s(4, 50, 64, plan=(0, 16, 8, 0), warm=True, used=True, why="warm start on 200 x 64"),
    _s(3, 100, 128, plan=(0, 16, 8, 0), warm=True, used=False,
       why="warm requested, erank_fits but not erank_fits_warm: falls back to the cold LDS kernel"),
    _s(3, 300, 128, pad=(1, 150, 300), route="blocked", plan=(16, 4, 0, 8, 8), why="ragged clips: padded frames in the tokens"),
    _s(8, 1200, 128, refuse="rank penalty", why="N = 9600 > 9596"),
    _s(11, 873, 2048, 16, refuse="rank penalty", why="N = 9603 > 9596"),
]

# byte bounds the plan query must flip at: (C, last R on the LDS kernel), blocked block-size thresholds (last R with b,
# b), the blocked bound
LDS_BOUNDS = [(128, 316)]
BLOCK_BOUNDS = [(1196, 16), (2396, 8), (4796, 4), (9596, 2)]


def plan_key(p, route):
    """ops.erank_plan's dict -> the table's plan tuple."""
    if route == "blocked":
        return (p["b"], p["nch"], p["exact"], p["nreal"], p["nblk"])
    return (p["level"], p["G"], p["nch"], p["exact"])


def instance(p):
    """The kernel instance of a plan: (route, template arguments) -- nreal / nblk are runtime sizes."""
    if p["blocked"]:
        return ("blocked", p["b"], p["nch"], p["exact"])
    return ("warm" if p["warm"] else "lds", p["level"], p["G"], p["nch"], p["exact"])


def matrix_id(m):
    lay = m.layout if isinstance(m.layout, str) else f"batch{m.layout[1]}"
    return f"{m.route}-{m.R}x{m.C}-{m.spectrum}-{lay}"


def step_id(s):
    p = s.pad if isinstance(s.pad, str) else "ragged"
    return f"B{s.B}-S{s.S}-H{s.H}x{s.heads}-{p}" + ("-warm" if s.warm else "") + ("-chain" if s.chain else "")
