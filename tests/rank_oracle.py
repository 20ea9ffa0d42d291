"""Float64 restatements for the streaming-QR tests, and a float32 numpy restatement of the append itself.

  make_input        -- the inputs of tests/rank_cases.py, float64 [N, H];
  svdvals64, erank64, check_against_fp64 -- singular values / effective rank of the valid rows in float64 and the
                       comparison at the project's tolerances (rank_cases.SIGMA_*, erank_tol);
  append_f32, stream_f32 -- what r3d_qr_append / r3d_qr_merge compute, in numpy float32: tiles of rows folded into an
                       upper-triangular R by one Householder reflector per column, lanes over contiguous row slices,
                       a pairwise merge tree.  (The summation order inside a dot product is numpy's, not the kernel's: this
                       pins the method's accuracy, not the kernel's bits.)"""
import numpy as np

from tests import rank_cases as RC


def make_input(kind, N, H, seed):
    g = np.random.default_rng(seed)
    if kind == "gauss":
        return g.standard_normal((N, H))
    if kind == "relu":
        return np.maximum(g.standard_normal((N, H)) + 0.5, 0.0)
    if kind == "col":                                   # one dominant direction, a tail at 1e-4 of it
        a, b = g.standard_normal((N, 1)), g.standard_normal((1, H)) / np.sqrt(H)
        return a @ b + 1e-4 * g.standard_normal((N, H))       # sigma_1 ~ sqrt(N), the tail ~ 1e-4 sqrt(N)
    k = min(N, H)
    if kind == "sep":
        sv = np.linspace(0.2, 2.0, k)[::-1]
    elif kind == "clu":
        base = np.logspace(0, -4, k // 4)
        sv = np.sort((base[:, None] * (1.0 + 1e-3 * np.arange(4))[None, :]).reshape(-1))[::-1] * 50.0
        if sv.size < k:
            sv = np.concatenate([sv, np.repeat(sv[-1:] * 0.5, k - sv.size)])
    else:
        raise ValueError(kind)
    q1 = np.linalg.qr(g.standard_normal((N, k)))[0]
    q2 = np.linalg.qr(g.standard_normal((H, k)))[0]
    return (q1 * sv[None, :]) @ q2.T


def svdvals64(x):
    return np.linalg.svd(np.asarray(x, dtype=np.float64), compute_uv=False)


def erank_of_sigma(s):
    s = np.asarray(s, dtype=np.float64)
    p = s / s.sum()
    p = p[p > 0]
    return float(np.exp(-(p * np.log(p)).sum()))


def erank64(x):
    return erank_of_sigma(svdvals64(x))


def check_against_fp64(R, x_valid, what=""):
    """R: an [H, H] triangle (any float dtype) accumulated over the rows x_valid [n, H].  Its singular values, taken in
    float64, against float64 svdvals of x_valid.  Returns (worst sigma error / sigma_max, float64 effective rank)."""
    H = R.shape[0]
    got = svdvals64(R)
    ref = svdvals64(x_valid.astype(np.float32))        # the rows as the device saw them
    k = min(x_valid.shape[0], H)
    smax = ref[0]
    want = np.zeros(H)
    want[:k] = ref[:k]
    err = np.abs(got[:k] - want[:k])
    lim = RC.SIGMA_ATOL_REL * smax + RC.SIGMA_RTOL * want[:k]
    assert (err <= lim).all(), f"{what}: sigma off by {err.max() / smax:.3e} of sigma_max"
    if H > k:
        assert got[k:].max() <= RC.SURPLUS_REL * smax, f"{what}: surplus sigma {got[k:].max() / smax:.3e} of sigma_max"
    assert not np.tril(np.asarray(R), -1).any(), f"{what}: the strictly lower triangle of R is not zero"
    return float(err.max() / smax), erank_of_sigma(ref)


# ---------------------------------------------------------------------------------------------------------------------
# the append in float32
# ---------------------------------------------------------------------------------------------------------------------
def append_f32(R, X, tile):
    """Folds the rows of X (float32 [n, H]) into R (float32 [H, H], upper triangular, in place), `tile` rows at a time."""
    f = np.float32
    H = R.shape[0]
    for t0 in range(0, X.shape[0], tile):
        x = np.array(X[t0:t0 + tile], dtype=f)
        for j in range(H):
            xj = x[:, j].copy()
            s = f(np.dot(xj, xj))
            if s == 0:
                continue                                # an all-zero tile column: no step
            alpha = R[j, j]
            nrm = f(np.sqrt(f(alpha * alpha + s)))
            beta = -nrm if alpha >= 0 else nrm
            fac = f(1.0) / f(alpha - beta)
            tau = f(beta - alpha) / beta
            R[j, j] = beta
            if j + 1 < H:
                w = R[j, j + 1:] + (xj @ x[:, j + 1:]).astype(f) * fac
                R[j, j + 1:] = R[j, j + 1:] - tau * w
                x[:, j + 1:] -= np.outer(xj, (tau * w * fac).astype(f)).astype(f)
    return R


def stream_f32(X, chunk, lanes, tile):
    """StreamingRank in float32 numpy: update() per `chunk` rows (None: all at once), each call's rows cut into `lanes`
    contiguous slices of ceil(n / lanes), then the pairwise merge tree.  Returns the merged R [H, H]."""
    X = np.asarray(X, dtype=np.float32)
    N, H = X.shape
    Rs = [np.zeros((H, H), dtype=np.float32) for _ in range(lanes)]
    chunk = N if chunk is None else chunk
    for c0 in range(0, N, chunk):
        xc = X[c0:c0 + chunk]
        per = -(-xc.shape[0] // lanes)
        for g in range(lanes):
            append_f32(Rs[g], xc[g * per:(g + 1) * per], tile)
    stride = 1
    while stride < lanes:
        for g in range(0, lanes, 2 * stride):
            if g + stride < lanes:
                append_f32(Rs[g], Rs[g + stride], tile)
        stride *= 2
    return Rs[0]
