"""Effective rank of a representation over a whole data set (the paper's own number: RGB, depth and fused tokens over an
evaluation split), by a streaming QR.

``effective_rank`` (erank.py) decomposes ONE matrix that must fit the Jacobi kernels: at most 9596 rows, in practice one
step's [B*S, H] fused tokens, whose rank is capped by the rows of the batch.  Here an upper-triangular R [H, H] with
R^T R = sum X^T X is kept on the device and every batch's rows are folded into it by Householder reflectors
(qr_stream.hip) -- the square is never formed, so a collapsed representation (one dominant direction, a tail at 1e-4 of
it) keeps its tail, which an fp32 Gram accumulation loses.  At the end R, which has the singular values of the whole
[rows, H] matrix, goes to the Jacobi that already exists.

    acc = StreamingRank(H, device)            # lanes independent accumulators, one workgroup each
    acc.update(x, labels, pad_idx)            # enqueue only; x [n, H] or [B, S, H]
    acc.finalize()                            # dict(erank=float, sigma=Tensor[H], rows=int): the one device->host read

``measure_rank(model, loader, device)`` runs the validation forward of a fuser model over a loader and returns one such
dict for the RGB embedding, the depth embedding and the fused tokens; ``train(..., args.erank_report)`` feeds the same
accumulators from validate()'s own forwards (FusionEngine.rank_stream)."""
import torch

from . import ops

BUFFERS = {"rgb": "rgb", "depth": "dep", "fused": "fused"}      # public name -> attribute of the engine's workspace
BUFFERS3 = {"rgb": "rgb", "depth": "dep", "gaze": "gaze", "fused": "fused"}     # the three-modality model's


def _is_m3(core):
    return hasattr(core, "gaze_projection")


def buffers_of(model):
    """public name -> workspace attribute for this model: BUFFERS, or BUFFERS3 for the three-modality model"""
    return BUFFERS3 if _is_m3(_fuser_core(model)) else BUFFERS


class StreamingRank:
    """Streaming QR accumulator of [*, H] rows; see the module docstring.  1 <= H <= 2048, 1 <= lanes <= 64."""

    def __init__(self, H, device, lanes=8):
        if not (isinstance(H, int) and H >= 1 and ops.qr_append_supported(H)):
            raise ValueError(f"StreamingRank: width {H} outside 1..2048 (r3d_qr_append_supported)")
        if not 1 <= lanes <= 64:
            raise ValueError(f"StreamingRank: {lanes} lanes outside 1..64")
        self.H, self.lanes, self.device = H, lanes, torch.device(device)
        self.R = torch.zeros(lanes, H, H, dtype=torch.float32, device=self.device)
        self.rows = torch.zeros(lanes, dtype=torch.int64, device=self.device)
        self._scratch = None

    def reset(self):
        self.R.zero_()
        self.rows.zero_()

    def update(self, x, labels=None, pad_idx=None):
        """Folds the rows of x ([n, H] or [B, S, H], float32, unit column stride) in.  labels ([n] or [B, S], int64) with
        pad_idx: rows whose label equals pad_idx are left out.  Enqueues one launch on the current stream, no host sync
        (usable inside a captured graph).  Contiguous inputs -- the engine's workspaces and labels are -- and [n, H]
        row slices (row stride >= H) are read in place with no allocation; a non-contiguous [B, S, H] x or non-contiguous
        labels are first copied by reshape(), which allocates."""
        if x.dim() == 3:
            x = x.reshape(-1, x.shape[-1])
        if x.dim() != 2 or x.shape[1] != self.H:
            raise ValueError(f"StreamingRank.update: expected [n, {self.H}] or [B, S, {self.H}], got {tuple(x.shape)}")
        if labels is not None:
            if pad_idx is None:
                raise ValueError("StreamingRank.update: labels need pad_idx")
            labels = labels.reshape(-1)
            if labels.numel() != x.shape[0]:
                raise ValueError(f"StreamingRank.update: {labels.numel()} labels for {x.shape[0]} rows")
        ops.qr_append(x, self.R, rows=self.rows, row_label=labels, pad_idx=0 if pad_idx is None else pad_idx)

    def finalize(self):
        """Merges the lanes into a scratch copy (the accumulators stay as they are: accumulation can go on), runs the
        Jacobi on the merged R and reads the result back: dict(erank, sigma [H] descending on the host, rows).  An
        accumulator that has seen no valid row reports erank 0.0 and sigma 0."""
        H = self.H
        if self._scratch is None:
            self._scratch = (torch.empty_like(self.R), torch.empty_like(self.rows))
        R, rows = self._scratch
        R.copy_(self.R)
        rows.copy_(self.rows)
        ops.qr_merge(R, rows)
        if ops.erank_fits(H, H):
            sigma = torch.empty(1, H, dtype=torch.float32, device=self.device)
            stats = torch.empty(1, 4, dtype=torch.float32, device=self.device)
            ops.erank_jacobi(R[0], sigma, stats)
            sigma, stats = sigma[0], stats[0]
        else:
            sigma, stats, _ = ops.erank_blocked(R[0])
        out = torch.cat([stats[:1].double(), rows[:1].double(), sigma.double()]).cpu()      # the single device->host read
        n = int(out[1])
        sig = torch.sort(out[2:].float(), descending=True)[0]
        if n == 0:                                       # nothing folded in: R is zero, the Jacobi's answer means nothing
            return dict(erank=0.0, sigma=torch.zeros(H), rows=0)
        return dict(erank=float(out[0]), sigma=sig, rows=n)


def _fuser_core(model):
    from .model.futr_safuser_tokenfusion import FUTR
    m = model
    while hasattr(m, "module") and not isinstance(m, FUTR):
        m = m.module
    if not isinstance(m, FUTR):
        raise ValueError(f"{type(m).__module__}.{type(m).__name__} has no fused token matrix: the data-set rank is measured "
                         f"on the RGB / depth embeddings and fused tokens of the SA-Fuser models (token fusion, BN-blend, "
                         f"activation-magnitude, plain); StreamingRank itself takes any [n, H] tensor")
    return m


def attach(model, which=None, lanes=8):
    """Accumulators (name -> StreamingRank) fed by every forward of the model's engine until detach().  Raises ValueError
    for a model without a fused token matrix, before anything is allocated.  which: default rgb, depth, fused (and gaze
    for the three-modality model)."""
    bufs = buffers_of(model)
    if which is None:
        which = tuple(bufs)
    for name in which:
        if name not in bufs:
            raise ValueError(f"measure_rank: unknown representation {name!r} (one of {sorted(bufs)})")
    eng = _fuser_core(model).engine()
    accs = {name: StreamingRank(eng.H, eng.device, lanes) for name in which}
    eng.rank_stream = [(bufs[name], acc) for name, acc in accs.items()]
    return accs


def detach(model):
    _fuser_core(model).engine().rank_stream = None


def measure_rank(model, loader, device, which=None):
    """Effective rank of the RGB embedding, the depth embedding and the fused tokens over every frame of `loader`
    (anything validate() accepts), padded frames (past_label == pad_idx) left out: {name: dict(erank, sigma, rows)}.
    The validation forward of each batch feeds the accumulators; one device->host read per name at the end.
    `device` is there for validate()'s calling convention: as in validate(), the batches go to the engine's own device."""
    from .train_proposed_depth import _to_dev
    core = _fuser_core(model)
    eng = core.engine()
    model.eval()
    accs = attach(core, which)
    try:
        with torch.no_grad():
            for data in loader:
                if data is None:
                    continue
                batch = _to_dev(data, eng.device, gaze=_is_m3(core))
                kw = dict(gaze=batch[5]) if len(batch) == 6 else {}
                eng.forward(batch[0], batch[1], batch[2], "val", training=False, need_grad=False, **kw)
    finally:
        detach(core)
    return {name: acc.finalize() for name, acc in accs.items()}


def report_line(results):
    """The line train() prints after validate() with --erank_report (the three-modality model: four names)."""
    if "gaze" in results:
        return "Effective rank over %d frames: rgb %.3f, depth %.3f, gaze %.3f, fused %.3f" % (
            results["fused"]["rows"], results["rgb"]["erank"], results["depth"]["erank"], results["gaze"]["erank"],
            results["fused"]["erank"])
    return "Effective rank over %d frames: rgb %.3f, depth %.3f, fused %.3f" % (
        results["fused"]["rows"], results["rgb"]["erank"], results["depth"]["erank"], results["fused"]["erank"])
