"""Case tables and tolerances of the tall rank route (r3d_amd.erank.ErankTall, csrc/qr_fold_wy.hip):
tests/test_erank_tall_cpu.py checks the oracle and the admission on the host, tests/test_erank_tall_gpu.py runs the rows.

FOLD_H / FOLD_N / FOLD_LANES -- the blocked fold kernel alone.  H: one panel, three panels (not a power of two), the two
  widths the models use, and the widest the kernel admits (appended at run time: the LDS budget decides it).  n: one row, less
  than a panel, less than a tile, several tiles' worth at small H, and two tiles + 7 (appended per H: the tile depends on
  it).  lanes 3 and 8 leave lanes without rows (n = 1) and lanes with fewer rows than H.
ROUTE -- ErankTall against float64 at (N, H): N barely above H, N = H, the first N past the Jacobi's LDS kernel, a
  generic-length N, the blocked Jacobi on R (H = 256) and the first N past the Jacobi's row limit; each with the "sep"
  and "clu" spectra of tests/erank_cases.py and with both folds.
STEPS -- training steps with erank_weight 0.05 on the tall route: (B, S, H, heads, pad, chain, why); chain: the backward goes
  through the hidden-128 chain kernel (None: not asserted).

Tolerances.  Effective rank: the project's rule |d| < 5e-3 max(1, er / 50).  Gradient error / scale: 3e-3 at kernel level
(tests/test_erank_shapes_gpu.py's bound for the clustered spectrum), 1e-2 for steps.  The float32 numpy restatement of the
route (erank_tall_oracle.route with dtype float32: LAPACK QR and SVD) lands at 1e-6 on the separated spectrum and at
2.8e-4 .. 4.8e-4 on the clustered one, |d erank| / erank < 4e-7: the reference's own working-precision error sits ~7x inside 3e-3.
Fold kernel: singular values of the merged R against float64 svdvals of X, relative to sigma_max, within the larger of
SIGMA_FACTOR x the float32 restatement's error on the same input and lanes and SIGMA_FLOOR = four fp32 roundings (the
floor decides nearly every case: see there); ||R^T R - X^T X||_F / ||X^T X||_F within gram_tol(n, H)."""
import collections

import numpy as np

ER_TOL = 5e-3
GRAD_TOL_KERNEL = 3e-3
GRAD_TOL_STEP = 1e-2
SIGMA_FACTOR = 8.0
# The fold's sigma bound is max(SIGMA_FACTOR x the restatement's error, SIGMA_FLOOR), and the floor decides it in nearly
# every case, n > 1 included: the float32 restatement (LAPACK QR on the host BLAS) lands between 4e-9 and 6e-8 of sigma_max,
# below ONE fp32 rounding (2^-24 = 6e-8), and at n = 1 it does no arithmetic at all (2e-16).  It gets there by means an
# fp32 kernel does not have: its norms are accumulated in higher precision, rows a lane does not have are exact zeros (the
# kernel and the unchanged r3d_qr_merge run every reflector and leave rounding residue of order eps sigma_max where a
# singular value is 0), and independent entry roundings average out in sigma.  What does not average out in fp32 is what a
# reflector shares over a whole row of R: its sum of squares, the square root, the reciprocal and tau, one rounding each.
# So the floor is four roundings of sigma_max, 4 x 2^-24 = 2.4e-7 -- from the format and the formula, not from the kernel's
# figures -- and the issue's 8 x holds wherever it is the larger of the two.
SIGMA_FLOOR = 4.0 * 2.0 ** -24
LAM = 0.05

FOLD_H = [16, 48, 128, 256]
FOLD_N = [1, 15, 64, 333]
FOLD_LANES = [1, 3, 8]

ROUTE = [(74, 64), (128, 128), (320, 128), (600, 128), (2048, 256), (9600, 128)]
SPECTRA = ["sep", "clu"]
FOLDS = ["wy", "column"]

Step = collections.namedtuple("Step", "B S H heads pad chain why")
STEPS = [
    Step(8, 16, 128, 8, "tail", True, "hidden-128 chain backward: the penalty's gradient handed over as d_extra"),
    Step(2, 37, 64, 4, (37, 33), False, "ragged clips on the composed path, N = 74 barely above H"),
    Step(4, 80, 128, 8, "tail", None, "320 rows: both routes admit it"),
    Step(8, 1200, 128, 8, "tail", True, "9600 rows: refused by the Jacobi route"),
    Step(2, 160, 256, 8, "tail", False, "hidden 256: [2H, H] past the LDS kernel, the blocked sweep with erank_max_sweeps"),
]
BOTH_ROUTES = (4, 80, 128)
JACOBI_REFUSES = (8, 1200, 128)


def step_id(s):
    return f"B{s.B}-S{s.S}-H{s.H}x{s.heads}"


def gram_tol(n, H):
    """Bound on ||R^T R - X^T X||_F / ||X^T X||_F for an fp32 Householder fold.  Every entry of R is the end of a chain of
    k = max(n, H) fp32 updates (n tile rows per dot product, H reflectors per entry), each with relative error eps = 2^-24;
    rounding errors of that many operations accumulate like sqrt(k) eps in norm (the worst case k eps is never met by
    random rounding), and R^T R doubles it.  A factor 8 on top: 2 for the doubling, 4 of head room."""
    return 8.0 * 2.0 ** -24 * float(np.sqrt(max(n, H)))


def fold_input(n, H, seed, kind="plain"):
    """fp32 [n, H]: normal rows, column scales graded over two decades (R's columns then differ in size as token
    features do).  kind "zeros": an all-zero column and a block of zero rows."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, H)) * np.logspace(0, -2, H)[None, :]
    if kind == "zeros":
        x[:, H // 3] = 0.0
        x[n // 4:n // 2] = 0.0
    return x.astype(np.float32)
