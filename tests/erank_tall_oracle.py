"""The tall rank route (r3d_amd.erank.ErankTall) restated in numpy, in float64 (the reference) and in float32 (how far
LAPACK's own QR and SVD land from it in the working precision: the yardstick of the tolerances in erank_tall_cases.py).

    fold     per lane g: Householder QR of the rows [g ceil(n / lanes), ...) -> R_g [H, H] upper triangular (lanes with
             fewer than H rows: zero-padded; lanes without rows: zero);
    merge    the tree of r3d_qr_merge: lane g + stride folded into lane g by a QR of the two stacked triangles;
    route    SVD of the merged R = U S V^T; erank = exp(-sum p log p), p = sigma / sum sigma;
             d erank / dX = X M,  M = V diag(g / sigma) V^T,  g_k = -erank (log p_k + entropy) / sum sigma,
             with r3d_erank_bwd_coef2's guard: sigma_k <= 1e-6 sigma_max gives 0."""
import numpy as np


def fold_lane(rows, H, dtype):
    R = np.zeros((H, H), dtype)
    if rows.shape[0]:
        r = np.linalg.qr(rows.astype(dtype), mode="r")
        R[:r.shape[0]] = r
    return R


def fold(X, lanes, dtype=np.float64):
    """X [n, H] -> R [lanes, H, H], lane g from the rows [g ceil(n / lanes), ...)."""
    n, H = X.shape
    per = -(-n // lanes) if n else 0
    return np.stack([fold_lane(X[min(g * per, n):min(g * per + per, n)], H, dtype) for g in range(lanes)])


def merge(R):
    """The merge tree over R [lanes, H, H]; returns the total (lane 0)."""
    R = R.copy()
    lanes, H = R.shape[0], R.shape[1]
    stride = 1
    while stride < lanes:
        for g in range(0, lanes, 2 * stride):
            if g + stride < lanes:
                R[g] = np.linalg.qr(np.vstack([R[g], R[g + stride]]), mode="r")
        stride *= 2
    return R[0]


def erank_of_sigma(s):
    total = s.sum()
    p = s[s > 0] / total
    ent = -(p * np.log(p)).sum()
    return np.exp(ent), ent, total


def route(X, lanes=1, dtype=np.float64):
    """(erank, dX [n, H], sigma [H]) of the tall route in `dtype`."""
    X = X.astype(dtype)
    R = merge(fold(X, lanes, dtype))
    _, s, vt = np.linalg.svd(R)
    er, ent, total = erank_of_sigma(s)
    coef = np.zeros_like(s)
    ok = s > 1e-6 * s.max()
    coef[ok] = -er * (np.log(s[ok] / total) + ent) / total / s[ok]
    M = (vt.T * coef[None, :]) @ vt
    return float(er), X @ M, s


def grad_err(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
