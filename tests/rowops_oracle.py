"""Plain restatements of the row-wise kernels (csrc/rowops.hip), each taking a dtype: at float64 they are the reference of
tests/test_rowops_gpu.py, at float32 they measure e32 = max|f32 - f64| on the same operands (tests/rowops_cases.py).
Operands are float32 tensors on the CPU and are cast on entry.  Every sum over rows is a plain left-to-right loop in the
working dtype, so at float32 it carries the rounding of the longest serial chain a kernel may use (torch.sum would
accumulate pairwise, or in double)."""
import torch

EPS = 1e-5                      # nn.LayerNorm's default, kLnEps of the kernels


def rowsum(x, dtype):
    """sum over dim 0, one row after the other, accumulated in dtype"""
    x = x.to(dtype)
    acc = torch.zeros(x.shape[1:], dtype=dtype)
    for r in range(x.shape[0]):
        acc = acc + x[r]
    return acc


def ln_fwd(x, gamma, beta, dtype, *, nsplit=0, bias=None, relu=False, pair=False):
    """x [rows, H], or [nsplit, rows, H] slabs (+ bias) summed into `pre` first.  Returns pre, xhat, v (gamma xhat + beta,
    before the ReLU), y, mean, rstd and pair (the mean of rows 2u, 2u + 1; None unless pair).  Differentiable in its
    operands."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    pre = x
    if nsplit:
        assert x.dim() == 3 and x.shape[0] == nsplit
        pre = x[0]
        for p in range(1, nsplit):
            pre = pre + x[p]
        if bias is not None:
            pre = pre + bias.to(dtype)
    rows, H = pre.shape
    mean = pre.sum(1) / H
    dlt = pre - mean[:, None]
    rstd = 1.0 / torch.sqrt((dlt * dlt).sum(1) / H + EPS)
    xhat = dlt * rstd[:, None]
    v = xhat * gamma + beta
    y = v.clamp_min(0) if relu else v
    return dict(pre=pre, xhat=xhat, v=v, y=y, mean=mean, rstd=rstd, pair=(y.view(rows // 2, 2, H).sum(1) * 0.5) if pair else None)


def _finish_bwd(gx, add1, add2, mask, drop_scale, dtype):
    dx = gx
    if add1 is not None:
        dx = dx + add1.to(dtype)
    if add2 is not None:
        dx = dx + add2.to(dtype)
    dx2 = dx * (drop_scale * mask.to(dtype)) if mask is not None else dx
    return dx, dx2


def ln_bwd(dy, x, gamma, beta, dtype, *, dy2=None, pair_in=False, relu=False, add1=None, add2=None, mask=None, drop_scale=1.0):
    """The reference: autograd through ln_fwd.  The incoming gradient dy + dy2 is that of y, or under pair_in that of the
    pair mean ([rows / 2, H]).  dx = dL/dx + add1 + add2; dx2 = dx drop_scale mask (dx where there is no mask)."""
    xr = x.to(dtype).clone().requires_grad_(True)
    gr, br = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    f = ln_fwd(xr, gr, br, dtype, relu=relu, pair=pair_in)
    d = dy.to(dtype) if dy2 is None else dy.to(dtype) + dy2.to(dtype)
    (f["pair"] if pair_in else f["y"]).backward(d)
    dx, dx2 = _finish_bwd(xr.grad, add1, add2, mask, drop_scale, dtype)
    return dict(dx=dx, dx2=dx2, dgamma=gr.grad, dbeta=br.grad)


def ln_bwd_closed(dy, x, gamma, beta, dtype, *, dy2=None, pair_in=False, relu=False, add1=None, add2=None, mask=None, drop_scale=1.0):
    """The same in closed form, as the kernel states it: d = dy + dy2 (both halved and row-paired under pair_in), zeroed
    where the ReLU is off; g = d gamma; dx = rstd (g - mean_c g - xhat mean_c(g xhat)); dgamma = sum_r d xhat,
    dbeta = sum_r d."""
    with torch.no_grad():
        f = ln_fwd(x, gamma, beta, dtype)
        d = dy.to(dtype) if dy2 is None else dy.to(dtype) + dy2.to(dtype)
        if pair_in:
            d = 0.5 * d.repeat_interleave(2, dim=0)
        if relu:
            d = torch.where(f["v"] > 0, d, torch.zeros_like(d))
        H = x.shape[1]
        g = d * gamma.to(dtype)
        s1, s2 = g.sum(1, keepdim=True) / H, (g * f["xhat"]).sum(1, keepdim=True) / H
        gx = f["rstd"][:, None] * (g - s1 - f["xhat"] * s2)
        dx, dx2 = _finish_bwd(gx, add1, add2, mask, drop_scale, dtype)
        return dict(dx=dx, dx2=dx2, dgamma=rowsum(d * f["xhat"], dtype), dbeta=rowsum(d, dtype))


def colsum(x, dtype, out0=None):
    """out[c] (+)= sum_r x[r, c]; out0: what the accumulate form adds onto"""
    s = rowsum(x, dtype)
    return s if out0 is None else s + out0.to(dtype)


def rowmod_sum(x1, x2, mod, dtype, out0=None):
    """out[r, c] (+)= sum over rows with row % mod == r of x1[row, c] (+ x2[row, c]).  A residue class with no row is an
    exact 0."""
    x = x1.to(dtype) if x2 is None else x1.to(dtype) + x2.to(dtype)
    rows, cols = x.shape
    turns = -(-rows // mod)
    padded = torch.zeros(turns * mod, cols, dtype=dtype)
    padded[:rows] = x
    s = rowsum(padded.view(turns, mod, cols), dtype)
    return s if out0 is None else s + out0.to(dtype)


def add_rowbcast(x, add, mod, rows, dtype):
    """out[r, :] = x[r, :] + add[r % mod, :]; x None: the broadcast alone"""
    b = add.to(dtype)[torch.arange(rows) % mod]
    return b if x is None else b + x.to(dtype)


def finalize(ws, dtype):
    """ws [blocks, 2, H] partial (dgamma, dbeta) pairs -> (dgamma [H], dbeta [H])"""
    s = rowsum(ws, dtype)
    return s[0], s[1]
