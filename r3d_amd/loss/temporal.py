"""The reference's temporal auxiliary objectives -- ``utils.py``: ``temporal_contrastive_loss`` (:229), ``temporal_cluster_loss``
(:271), ``focal_loss`` (:493), ``cal_performance_focal`` (:394) -- and the run detection that feeds the first two
(``train/train_unsupervised.py``: ``get_cluster_intervals``, :34), computed by csrc/temporal.hip.

A run of clip b starts at t = 0 and wherever ``labels[b, t] != labels[b, t - 1]`` (padding is a label like any other): the
partition ``get_cluster_intervals`` returns.  ``label_runs`` finds it in one launch without a host synchronisation; each loss
takes a ``Runs``, a ``[B, T]`` integer label tensor, or the reference's list of lists of ``(start, end)``.

    temporal_cluster_loss      intra = sum_{b,r} mse(x_r, m_r) / total,  inter = sum_{b: R_b > 1} sum_{i<j} 1 / (1e-5 + |m_i - m_j|)
                               / (M (n_last - 1)); n_last is the run count of the LAST clip with more than one run (the
                               reference divides by its leftover loop variable), inter = 0 when no clip has two runs.
    temporal_contrastive_loss  per clip z = F.normalize(x), p = softmax(z z^T / temperature) over all columns; frame t of the
                               run (st, en) has the positive set {c : st <= c <= en, c != t - st} -- the reference's
                               fill_diagonal_ on its [n, T] mask removes the row's index inside its run, not t itself.  The
                               log-sum-exp carries a maximum, so the value stays finite where the reference's bare exp
                               overflows (temperature 0.01 in float32); it equals the reference wherever that is finite.
    focal_loss                 mean over all N rows of alpha (1 - p_gold)^gamma CE + penalty_weight [argmax == pad, unmasked];
                               a row is masked when gold is pad or the excluded class.  An unmasked label outside [0, C) is
                               treated as masked too (the reference raises an index error there).  gamma >= 1.

All of it is float32 on the GPU with no torch fallback; every call only enqueues (``cal_performance_focal`` and
``get_cluster_intervals`` read their result back in one transfer), allocates its outputs and workspace through torch, uses
no atomics, and can be captured in a graph.  The autograd functions save the input and the row / run statistics only.

Not here: ``generate_prompt`` (the LLM prompt builder), and a ``train_unsupervised`` loop -- its models
(``futr_unsupervised*.py`` other than the depth-query model) are not built.
"""
import numpy as np
import torch

from .. import ops

MAX_WIDTH = 256      # widest row of the cluster (C) and contrastive (D) kernels (r3d_temporal_width_supported)


class Runs:
    """The runs of equal labels of B clips of T frames, on the device, all int32: ``first`` / ``last`` [B, T] (the first and
    last frame of each frame's run), ``starts`` [B, T] (``starts[b, r]``: first frame of run r; T past the last run) and
    ``count`` [B].  One buffer ``buf`` = (first, last, starts, count) backs the four views."""

    def __init__(self, buf, B, T):
        n = B * T
        self.buf, self.B, self.T = buf, B, T
        self.first, self.last, self.starts = buf[:n].view(B, T), buf[n:2 * n].view(B, T), buf[2 * n:3 * n].view(B, T)
        self.count = buf[3 * n:]

    @property
    def device(self):
        return self.buf.device

    def intervals(self):
        """The reference's list (per clip) of lists of (start, end); one device-to-host transfer."""
        return _intervals_from_host(self.buf.cpu().numpy(), self.B, self.T)


def _intervals_from_host(h, B, T):
    n = B * T
    last, starts, count = h[n:2 * n].reshape(B, T), h[2 * n:3 * n].reshape(B, T), h[3 * n:]
    return [[(int(s), int(last[b, s])) for s in starts[b, :count[b]]] for b in range(B)]


def label_runs(labels):
    """labels [B, T], any integer dtype, on the GPU -> Runs.  One launch, no synchronisation."""
    if labels.dim() != 2 or labels.shape[0] < 1 or labels.shape[1] < 1:
        raise ValueError(f"label_runs takes labels [B, T] with B, T >= 1, got {tuple(labels.shape)}")
    if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise ValueError(f"label_runs takes integer labels, got {labels.dtype}")
    if not labels.is_cuda:
        raise TypeError("label_runs runs on the GPU only (there is no torch fallback)")
    B, T = labels.shape
    buf = torch.empty(3 * B * T + B, dtype=torch.int32, device=labels.device)
    r = Runs(buf, B, T)
    ops.label_runs(labels.to(torch.int64).contiguous(), r.first, r.last, r.starts, r.count)
    return r


def runs_from_intervals(cluster_intervals, T, device):
    """The reference's list of lists of (start, end) -> Runs, with one upload.  ValueError unless every clip's intervals
    partition 0 .. T - 1 in order."""
    B = len(cluster_intervals)
    if B < 1 or T < 1:
        raise ValueError(f"runs_from_intervals takes B >= 1 clips of T >= 1 frames, got B {B}, T {T}")
    h = np.empty(3 * B * T + B, dtype=np.int32)
    n = B * T
    first, last, starts = h[:n].reshape(B, T), h[n:2 * n].reshape(B, T), h[2 * n:3 * n].reshape(B, T)
    starts[:] = T
    for b, clip in enumerate(cluster_intervals):
        nxt = 0
        for r, (s, e) in enumerate(clip):
            s, e = int(s), int(e)
            if s != nxt or e < s or e >= T:
                raise ValueError(f"clip {b}: interval {r} = ({s}, {e}) does not continue a partition of 0..{T - 1} at {nxt}")
            first[b, s:e + 1], last[b, s:e + 1], starts[b, r] = s, e, s
            nxt = e + 1
        if nxt != T:
            raise ValueError(f"clip {b}: the intervals end at {nxt - 1}, not at T - 1 = {T - 1}")
        h[3 * n + b] = len(clip)
    return Runs(torch.from_numpy(h).to(device), B, T)


def get_cluster_intervals(gt):
    """``train_unsupervised.get_cluster_intervals``: gt [B, T] -> list of lists of (start, end), from the device runs with one
    transfer (the reference synchronises once per frame)."""
    return label_runs(gt).intervals()


def _as_runs(runs, B, T, device):
    if isinstance(runs, Runs):
        if (runs.B, runs.T) != (B, T):
            raise ValueError(f"the runs describe [{runs.B}, {runs.T}] frames, the predictions [{B}, {T}]")
        return runs
    if torch.is_tensor(runs):
        if tuple(runs.shape) != (B, T):
            raise ValueError(f"labels {tuple(runs.shape)} do not match the predictions' [B, T] = [{B}, {T}]")
        return label_runs(runs.to(device))
    if len(runs) != B:
        raise ValueError(f"{len(runs)} interval lists for {B} clips")
    return runs_from_intervals(runs, T, device)


def _rows(x, what):
    """predictions [B, T, W] -> (rows [B * T, W] without a copy where the layout allows it, B, T); ValueError past a limit"""
    if x.dim() != 3:
        raise ValueError(f"{what} takes predictions [B, T, C], got {tuple(x.shape)}")
    B, T, W = x.shape
    if B < 1 or T < 1:
        raise ValueError(f"{what}: B = {B}, T = {T}; B >= 1 and T >= 1 are required")
    if not 1 <= W <= MAX_WIDTH:
        raise ValueError(f"{what}: row width {W}; the kernel takes 1 <= width <= {MAX_WIDTH}")
    return B, T, W


def _flat(x):
    B, T, W = x.shape
    if not (x.stride(2) == 1 and (B * T == 1 or (x.stride(1) >= W and (B == 1 or x.stride(0) == T * x.stride(1))))):
        x = x.contiguous()                                      # (rows of one stride >= W are taken as they are)
    return torch.as_strided(x, (B * T, W), (x.stride(1), 1), x.storage_offset())


def _device_f32(x, what):
    if not (x.is_cuda and x.dtype == torch.float32):
        raise TypeError(f"{what} runs on the GPU in float32 only (there is no torch fallback)")


class _ClusterFn(torch.autograd.Function):
    """Saves the input and the run statistics (means, scales) only."""

    @staticmethod
    def forward(ctx, x, runs):
        B, T, C = x.shape
        rows = _flat(x)
        ws = torch.empty(ops.tcluster_ws_floats(B, T, C), dtype=torch.float32, device=x.device)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        ops.tcluster_fwd(rows, B, T, runs.starts, runs.last, runs.count, ws, loss)
        ctx.save_for_backward(rows, ws)
        ctx.runs, ctx.shape = runs, (B, T, C)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        rows, ws = ctx.saved_tensors
        B, T, C = ctx.shape
        dx = torch.empty(B * T, C, dtype=torch.float32, device=rows.device)
        r = ctx.runs
        ops.tcluster_bwd(rows, B, T, r.starts, r.last, r.count, ws, dx, d_loss=g.to(torch.float32).contiguous())
        return dx.view(B, T, C), None


class _ContrastFn(torch.autograd.Function):
    """Saves the input and the row statistics only."""

    @staticmethod
    def forward(ctx, x, runs, temperature):
        B, T, D = x.shape
        rows = _flat(x)
        ws = torch.empty(ops.tcontrast_ws_floats(B, T), dtype=torch.float32, device=x.device)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        ops.tcontrast_fwd(rows, B, T, runs.first, runs.last, ws, loss, temperature=temperature)
        ctx.save_for_backward(rows, ws)
        ctx.runs, ctx.shape, ctx.temperature = runs, (B, T, D), temperature
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        rows, ws = ctx.saved_tensors
        B, T, D = ctx.shape
        dx = torch.empty(B * T, D, dtype=torch.float32, device=rows.device)
        r = ctx.runs
        ops.tcontrast_bwd(rows, B, T, r.first, r.last, ws, dx, temperature=ctx.temperature,
                          d_loss=g.to(torch.float32).contiguous())
        return dx.view(B, T, D), None, None


class _FocalFn(torch.autograd.Function):
    """Saves the input only: the backward is the same row-wise launch with the gradient switched on."""

    @staticmethod
    def forward(ctx, pred, gold, kw):
        N = pred.shape[0]
        dev = pred.device
        ws = torch.empty(N, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        flags = torch.empty(N, dtype=torch.bool, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        ops.focal_rows(pred, gold, ws=ws, loss_out=loss, flags=flags, counts=counts, **kw)
        ctx.save_for_backward(pred, gold)
        ctx.kw = kw
        ctx.mark_non_differentiable(flags, counts)
        return loss.view(()), flags, counts

    @staticmethod
    def backward(ctx, g, _gf, _gc):
        pred, gold = ctx.saved_tensors
        d = torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
        ops.focal_rows(pred, gold, d_pred=d, d_loss=g.to(torch.float32).contiguous(), **ctx.kw)
        return d, None, None


def temporal_cluster_loss(predictions, cluster_intervals):
    """``utils.temporal_cluster_loss(predictions [B, T, C], cluster_intervals)``; the second argument may also be a ``Runs`` or
    a [B, T] label tensor.  Returns the scalar loss (differentiable with respect to predictions)."""
    B, T, _ = _rows(predictions, "temporal_cluster_loss")
    if not isinstance(cluster_intervals, Runs) and torch.is_tensor(cluster_intervals) and tuple(cluster_intervals.shape) != (B, T):
        raise ValueError(f"labels {tuple(cluster_intervals.shape)} do not match the predictions' [B, T] = [{B}, {T}]")
    _device_f32(predictions, "temporal_cluster_loss")
    return _ClusterFn.apply(predictions, _as_runs(cluster_intervals, B, T, predictions.device))


def temporal_contrastive_loss(predictions, cluster_intervals, temperature=0.07):
    """``utils.temporal_contrastive_loss(predictions [B, T, D], cluster_intervals, temperature)``; the second argument may also
    be a ``Runs`` or a [B, T] label tensor.  Returns the scalar loss (differentiable with respect to predictions)."""
    B, T, _ = _rows(predictions, "temporal_contrastive_loss")
    if not float(temperature) > 0.0:
        raise ValueError(f"temporal_contrastive_loss: temperature {temperature}; temperature > 0 is required")
    if not isinstance(cluster_intervals, Runs) and torch.is_tensor(cluster_intervals) and tuple(cluster_intervals.shape) != (B, T):
        raise ValueError(f"labels {tuple(cluster_intervals.shape)} do not match the predictions' [B, T] = [{B}, {T}]")
    _device_f32(predictions, "temporal_contrastive_loss")
    return _ContrastFn.apply(predictions, _as_runs(cluster_intervals, B, T, predictions.device), float(temperature))


def _focal(pred, gold, trg_pad_idx, exclude_class_idx, alpha, gamma, penalty_weight):
    if pred.dim() != 2 or pred.shape[0] < 1 or pred.shape[1] < 1:
        raise ValueError(f"focal_loss takes pred [N, C] with N, C >= 1, got {tuple(pred.shape)}")
    if gold.dim() != 1 or gold.shape[0] != pred.shape[0]:
        raise ValueError(f"focal_loss: gold {tuple(gold.shape)} does not match pred's {pred.shape[0]} rows")
    if not float(gamma) >= 1.0:
        raise ValueError(f"focal_loss: gamma {gamma}; gamma >= 1 is required (the gradient of (1 - p)^gamma is unbounded below it)")
    _device_f32(pred, "focal_loss")
    if pred.stride(1) != 1:
        pred = pred.contiguous()
    kw = dict(pad_idx=int(trg_pad_idx), exclude_idx=None if exclude_class_idx is None else int(exclude_class_idx),
              alpha=float(alpha), gamma=float(gamma), penalty_weight=float(penalty_weight))
    return _FocalFn.apply(pred, gold.to(device=pred.device, dtype=torch.int64).contiguous(), kw)


def focal_loss(pred, gold, trg_pad_idx, exclude_class_idx=None, alpha=1.0, gamma=2.0, penalty_weight=0.0):
    """``utils.focal_loss``: pred [N, C] logits, gold [N].  Returns (loss, l3_correct): the scalar loss (differentiable with
    respect to pred) and the bool flags ``argmax == gold`` on unmasked rows, False elsewhere.  No synchronisation."""
    loss, flags, _ = _focal(pred, gold, trg_pad_idx, exclude_class_idx, alpha, gamma, penalty_weight)
    return loss, flags


def cal_performance_focal(pred, gold, trg_pad_idx, exclude_class_idx=None, smoothing=False, reference=None, target_ref=None):
    """``utils.cal_performance_focal`` (smoothing, reference and target_ref are unused there too).  Returns (loss, n_correct,
    n_word, l3_correct); the two counters are read back in one transfer."""
    loss, flags, counts = _focal(pred, gold, trg_pad_idx, exclude_class_idx, 1.0, 2.0, 0.0)
    n_correct, n_word = counts.tolist()
    return loss, n_correct, n_word, flags
