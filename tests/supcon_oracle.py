"""Float64 restatement of the supervised contrastive loss, written from its formula (not from the reference's text).

Rows z_0 .. z_{N-1}, labels y_r, the first A rows anchors, T = temperature, T_b = base_temperature:

    s_ij   = z_i . z_j / T
    C(i)   = {j != i : row j not ignored}          lse_i = log sum_{j in C(i)} exp s_ij
    Pos(i) = {j in C(i) : y_j = y_i},  P_i = |Pos(i)|
    l_i    = -(T / T_b) ((1 / P_i) sum_{Pos(i)} s_ij - lse_i)  if P_i > 0 else 0
    loss   = sum over non-ignored anchors of l_i / max(1, number of non-ignored anchors)

normalize: z_r = x_r / max(|x_r|, 1e-12).  Everything is torch float64 and differentiable, so autograd gives the
gradient the kernel's backward is compared with."""
import torch


def contrast_rows(features):
    """[bsz, n_views, D] -> [n_views * bsz, D], view by view."""
    return torch.cat(torch.unbind(features, dim=1), dim=0)


def supcon(x, y, *, A=None, temperature=0.07, base_temperature=0.07, ignore_index=None, normalize=False):
    """x [N, D] (any float dtype; computed in float64), y [N] integer labels.  Returns (loss, lse [A], P [A]); lse is -inf and
    P is 0 where C(i) is empty."""
    x = x.double()
    N = x.shape[0]
    A = N if A is None else A
    z = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) if normalize else x
    kept = torch.ones(N, dtype=torch.bool) if ignore_index is None else (y != ignore_index)
    s = (z[:A] @ z.t()) / temperature
    in_c = kept[None, :].expand(A, N) & ~torch.eye(N, dtype=torch.bool)[:A]
    pos = in_c & (y[:A, None] == y[None, :])
    P = pos.sum(1)
    lse = torch.logsumexp(s.masked_fill(~in_c, float("-inf")), dim=1)
    live = kept[:A] & (P > 0)
    pos_sum = (s * pos).sum(1)
    per_row = torch.zeros(A, dtype=torch.float64)
    if bool(live.any()):
        idx = live.nonzero().flatten()
        per_row = per_row.index_put((idx,), -(temperature / base_temperature) * (pos_sum[idx] / P[idx] - lse[idx]))
    loss = per_row.sum() / max(1, int(kept[:A].sum()))
    return loss, lse.detach(), P


def supcon_with_grad(x, y, **kw):
    """(loss, d loss / d x, lse, P) in float64."""
    xr = x.detach().double().requires_grad_(True)
    loss, lse, P = supcon(xr, y, **kw)
    if loss.requires_grad:
        loss.backward()
    g = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    return loss.detach(), g, lse, P
