"""The reference's ``loss/spc.py``: ``SupConLoss`` (Supervised Contrastive Learning, arXiv 2004.11362; SimCLR when neither
labels nor mask are given), computed by the streaming kernel of csrc/supcon.hip.  No N x N tensor is formed: the forward
keeps one log-sum-exp, one positive mean and one count per row, the backward recomputes the scores tile by tile.

Contrast rows z_0 .. z_{N-1} are the views of ``features [bsz, n_views, D]`` concatenated view by view; the first A rows
are anchors (A = N for ``contrast_mode='all'``, bsz for ``'one'``); with T = temperature and s_ij = z_i . z_j / T

    C(i) = {j != i : row j not ignored}     lse_i = log sum_{C(i)} exp s_ij     Pos(i) = {j in C(i) : y_j = y_i}
    loss = mean over the non-ignored anchors of  -(T / base_temperature) (mean_{Pos(i)} s_ij - lse_i)   (0 if Pos(i) is empty)

which is the reference's value wherever the reference is finite.  Two differences, both where the reference returns nan:
its stabilising maximum includes the diagonal |z_i|^2 / T, which underflows every other exp on unnormalised rows (0.3 *
randn(130, 128) is enough); the maximum here runs over C(i) only and the result stays finite.  And a row with no admissible
contrast (bsz * n_views == 1, or every other row ignored) contributes 0 here and nan there.

There is no torch fallback: features must be float32 on the GPU, D <= 256; ``SupConLoss(..., wide=True)`` opts into the
kernel's wide route, which walks rows of up to 2048 columns in chunks of 256 (the same launches and bits up to 256).
"""
import torch
import torch.nn as nn

from .. import ops

MAX_WIDTH = 256      # the kernel's feature width limit (r3d_supcon_supported) without wide=True
MAX_WIDTH_WIDE = 2048       # with it (r3d_supcon_wide_supported): the widest hidden size any engine admits, the RGB feature width


class _SupConFn(torch.autograd.Function):
    """Saves the input and the row statistics only."""

    @staticmethod
    def forward(ctx, z, labels, bsz, A, temperature, base_temperature, ignore_index, normalize, wide):
        kw = dict(temperature=temperature, base_temperature=base_temperature, ignore_index=ignore_index, normalize=normalize,
                  wide=wide)
        ws = torch.empty(ops.supcon_ws_floats(z.shape[0], z.shape[1], normalize, wide), dtype=torch.float32, device=z.device)
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        ops.supcon_fwd(z, labels, bsz, A, ws, loss, **kw)
        ctx.save_for_backward(z, ws)
        ctx.labels, ctx.bsz, ctx.A, ctx.kw = labels, bsz, A, kw
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        z, ws = ctx.saved_tensors
        dz = torch.empty(z.shape, dtype=torch.float32, device=z.device)
        ops.supcon_bwd(z, ctx.labels, ctx.bsz, ctx.A, ws, dz, d_loss=g.to(torch.float32).contiguous(), **ctx.kw)
        return dz, None, None, None, None, None, None, None, None


class SupConLoss(nn.Module):
    """``SupConLoss(temperature, contrast_mode, base_temperature)`` with the reference's signature and ValueErrors.
    Keyword-only additions, both defaulting to the reference's behaviour: ``ignore_index`` (a row whose label equals it is
    neither anchor nor contrast: the result equals the loss of the kept rows alone) and ``normalize`` (rows are divided by
    max(|x|, 1e-12) inside the kernel, as ``F.normalize`` would, without a normalised copy).  A third, ``wide`` (default
    False: D <= 256), admits D <= 2048 through the kernel's wide route."""

    def __init__(self, temperature=0.07, contrast_mode='all', base_temperature=0.07, *, ignore_index=None, normalize=False,
                 wide=False):
        super().__init__()
        self.temperature = temperature
        self.contrast_mode = contrast_mode
        self.base_temperature = base_temperature
        self.ignore_index = ignore_index
        self.normalize = normalize
        self.wide = wide

    def forward(self, features, labels=None, mask=None):
        """features [bsz, n_views, ...] (further dimensions are flattened), labels [bsz] or None.  Returns the scalar loss."""
        if features.dim() < 3:
            raise ValueError('`features` needs to be [bsz, n_views, ...],'
                             'at least 3 dimensions are required')
        if features.dim() > 3:
            features = features.reshape(features.shape[0], features.shape[1], -1)
        bsz, n_views, D = features.shape
        if labels is not None and mask is not None:
            raise ValueError('Cannot define both `labels` and `mask`')
        if mask is not None:
            raise NotImplementedError("`mask`: an explicit contrastive mask is not supported by the streaming kernel (no "
                                      "training loop of the reference passes one); pass `labels`")
        if labels is not None:
            labels = labels.contiguous().view(-1)
            if labels.shape[0] != bsz:
                raise ValueError('Num of labels does not match num of features')
        if self.contrast_mode == 'one':
            A = bsz
        elif self.contrast_mode == 'all':
            A = bsz * n_views
        else:
            raise ValueError('Unknown mode: {}'.format(self.contrast_mode))
        if not ops.supcon_supported(D, wide=bool(self.wide)):
            if self.wide:
                raise ValueError(f"feature width {D}: the supervised contrastive kernel's wide route takes 1 <= D <= {MAX_WIDTH_WIDE}")
            raise ValueError(f"feature width {D}: the supervised contrastive kernel takes 1 <= D <= {MAX_WIDTH} "
                             f"(SupConLoss(..., wide=True) admits D <= {MAX_WIDTH_WIDE})")
        if not (features.is_cuda and features.dtype == torch.float32):
            raise TypeError("SupConLoss runs on the GPU in float32 only (there is no torch fallback)")
        if labels is not None:
            labels = labels.to(device=features.device, dtype=torch.int64)
        if n_views == 1:
            z = features[:, 0]                                  # a view: no copy
            if z.stride(1) != 1:
                z = z.contiguous()
        else:
            z = torch.cat(torch.unbind(features, dim=1), dim=0)
        return _SupConFn.apply(z, labels, bsz, A, float(self.temperature), float(self.base_temperature), self.ignore_index,
                               bool(self.normalize), bool(self.wide))
