"""Device-resident clip store: the whole training set in HBM, batches collated on the device by ONE kernel launch
(r3d_clip_collate, csrc/clipcache.hip).  Drop-in for the DataLoader of main_darai.py: `train()` / `validate()` take a
DeviceClipLoader unchanged.

Why it works (data/basedataset_darai_depth.py:84-206): an item (video, seq_idx, obs_perc) is deterministic -- rows
0:observed_len:sample_rate of the feature file, the same rows of the depth file after its start_frame:end_frame+1 trim,
and fixed label / transcript arrays -- and only the shuffle order changes between epochs.  So the frames are uploaded
once, as fp32 (lossless against the reference's torch.tensor(..., dtype=float32)), and a batch is a row gather plus
padding on the device: no host copy, no PCIe transfer per step.

    store = ClipStore.from_specs(clips, labels, pad_idx, "cuda")    # per-clip .npy specs (NpyClipReader's), deduplicated
    store = ClipStore.from_dataset(dataset, pad_idx, "cuda")        # any map-style dataset of the reference's items
    loader = DeviceClipLoader(store, batch_size, shuffle=True)      # yields [features, depth, past_label, dur, target]

Both constructors first build a host-only ClipPlan (pool rows, CSR tables, per-item lengths, bytes), check it against
free device memory, then allocate and upload."""
import ctypes as C
import os

import numpy as np
import torch
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler

from . import _lib
from .utils import NpyClipReader

MARGIN_BYTES = 1 << 30           # left free beside the store (the step's own buffers, the allocator's slack)
CHUNK_BYTES = 64 << 20           # pinned staging per upload chunk (two of them alternate)
_KEYS = ("features", "depth_features", "past_label", "trans_future_dur", "trans_future_target")


def _csr(lengths):
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(np.asarray(lengths, np.int64), out=off[1:])
    return off


class ClipPlan:
    """Host-only description of a store (no GPU needed).

    Pools: `rgb_src` / `dep_src` are lists of segments (source, rows) whose rows, concatenated, are the pool's rows in
    order; source is a `.npy` path (rows: file row indices) or an in-memory array (rows None: all of it).
    Tables (numpy int64 unless noted), CSR over the n items: off_f / ids_f and off_d / ids_d (pool rows of each item's
    feature / depth frames), off_l / lab (past_label), off_q / q_dur (fp32) / q_tgt (trans_future_dur / _target).
    len_f, len_d, len_l, len_q: per-item lengths, from which each batch's padded sizes are taken on the host."""

    def __init__(self, rgb_src, dep_src, feat_shape, frame_shape, ids_f, len_f, ids_d, len_d, labels, pad_idx):
        self.rgb_src, self.dep_src = rgb_src, dep_src
        self.feat_shape, self.frame_shape = tuple(int(x) for x in feat_shape), tuple(int(x) for x in frame_shape)
        self.D, self.P = int(np.prod(self.feat_shape)), int(np.prod(self.frame_shape))
        self.pad_idx = int(pad_idx)
        self.len_f, self.len_d = np.asarray(len_f, np.int64), np.asarray(len_d, np.int64)
        self.off_f, self.off_d = _csr(self.len_f), _csr(self.len_d)
        self.ids_f, self.ids_d = np.asarray(ids_f, np.int64), np.asarray(ids_d, np.int64)
        lab, dur, tgt = [], [], []
        for i, (pl, d, t) in enumerate(labels):
            pl = np.asarray(pl).reshape(-1).astype(np.int64)
            d = np.asarray(d).reshape(-1).astype(np.float32)
            t = np.asarray(t).reshape(-1).astype(np.int64)
            if d.shape != t.shape:
                raise ValueError(f"item {i}: trans_future_dur has {d.size} entries and trans_future_target {t.size}; "
                                 "the store keeps one length for both (the reference pads both to n_query)")
            lab.append(pl), dur.append(d), tgt.append(t)
        self.len_l = np.array([x.size for x in lab], np.int64)
        self.len_q = np.array([x.size for x in tgt], np.int64)
        self.off_l, self.off_q = _csr(self.len_l), _csr(self.len_q)
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)      # noqa: E731
        self.lab, self.q_dur, self.q_tgt = cat(lab, np.int64), cat(dur, np.float32), cat(tgt, np.int64)
        self.F_rgb = int(sum(len(r) if r is not None else len(s) for s, r in rgb_src))
        self.F_dep = int(sum(len(r) if r is not None else len(s) for s, r in dep_src))
        n = len(self.len_f)
        if not (len(self.len_d) == len(self.len_l) == n):
            raise ValueError("clips and labels differ in number")

    def __len__(self):
        return len(self.len_f)

    @property
    def nbytes(self):
        """Device bytes of the store: both pools (fp32) and every table."""
        tables = (self.off_f, self.ids_f, self.off_d, self.ids_d, self.off_l, self.lab, self.off_q, self.q_dur, self.q_tgt)
        return 4 * (self.F_rgb * self.D + self.F_dep * self.P) + sum(max(t.size, 1) * t.itemsize for t in tables)

    def sizes(self, idx):
        """Padded extents (S_f, S_d, S_l, S_q) of a batch of item ids: the per-tensor maxima pad_sequence pads to."""
        idx = np.asarray(idx, np.int64)
        if idx.size == 0:
            return 0, 0, 0, 0
        return tuple(int(a[idx].max()) for a in (self.len_f, self.len_d, self.len_l, self.len_q))

    def check_capacity(self, device, budget=None):
        """ValueError unless the store fits.  budget (bytes) overrides the free device memory minus MARGIN_BYTES; with a
        budget nothing touches the device."""
        if budget is None:
            free, _ = torch.cuda.mem_get_info(torch.device(device))
            avail, what = free - MARGIN_BYTES, f"free device memory {free} bytes minus a margin of {MARGIN_BYTES}"
        else:
            avail, what = int(budget), "the budget"
        if self.nbytes > avail:
            raise ValueError(f"clip store needs {self.nbytes} bytes but {what} leaves {max(avail, 0)} bytes")


def plan_specs(clips, labels, pad_idx):
    """ClipPlan of NpyClipReader clip specs (feature_file, depth_file, start, stop, step[, depth_offset[, depth_end]]).
    Frames are deduplicated by (file, row): items that share a prefix (DARai's 0.2 / 0.3 / 0.5 observations of one
    sequence) share pool rows, and only rows some item samples are stored.  Files are only opened for their shapes."""
    clips, labels = list(clips), list(labels)
    if len(clips) != len(labels):
        raise ValueError(f"{len(clips)} clips but {len(labels)} label triples")
    shapes = {}

    def shape(path):
        key = os.path.realpath(path)
        if key not in shapes:
            shapes[key] = tuple(np.load(path, mmap_mode="r").shape)
        return key, shapes[key]

    def pool(rows_per_item):
        """rows_per_item: [(file key, range)] -> (segments, ids per item)."""
        files = {}
        for key, r in rows_per_item:
            files.setdefault(key, []).append(np.asarray(r, np.int64))
        base, segs, uniq = 0, [], {}
        for key, rs in files.items():
            u = np.unique(np.concatenate(rs))
            uniq[key] = (base, u)
            if u.size:
                segs.append((key, u))
            base += u.size
        ids = [uniq[k][0] + np.searchsorted(uniq[k][1], np.asarray(r, np.int64)) for k, r in rows_per_item]
        return segs, ids

    rows_f, rows_d, feat_shape, frame_shape = [], [], None, None
    for c in clips:
        kf, sf = shape(c[0])
        kd, sd = shape(c[1])
        if feat_shape is None:
            feat_shape, frame_shape = sf[1:], sd[1:]
        if sf[1:] != feat_shape or sd[1:] != frame_shape:
            raise ValueError(f"clip {c[:2]}: frame shapes {sf[1:]} / {sd[1:]} differ from {feat_shape} / {frame_shape}")
        rows_f.append((kf, NpyClipReader._rows(sf[0], c[2], c[3], c[4])))
        rows_d.append((kd, NpyClipReader._rows(sd[0], c[2], c[3], c[4], *(c[5:7]))))
    seg_f, ids_f = pool(rows_f)
    seg_d, ids_d = pool(rows_d)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)       # noqa: E731
    return ClipPlan(seg_f, seg_d, feat_shape or (0,), frame_shape or (0,), cat(ids_f), [len(r) for _, r in rows_f],
                    cat(ids_d), [len(r) for _, r in rows_d], labels, pad_idx)


def plan_dataset(dataset, pad_idx):
    """ClipPlan of a map-style dataset whose items are the reference's item dict (basedataset_darai_depth.py:174-180) or the
    five tensors in my_collate order.  Each item is read once and its frames are kept as the dataset returned them until
    the upload; they are NOT deduplicated (the dataset hides which file rows an item came from)."""
    rgb, dep, len_f, len_d, labels = [], [], [], [], []
    feat_shape = frame_shape = None
    for i in range(len(dataset)):
        it = dataset[i]
        if isinstance(it, dict):
            it = [it[k] for k in _KEYS]
        f, d, pl, dur, tgt = [x.numpy() if torch.is_tensor(x) else np.asarray(x) for x in it]
        if feat_shape is None:
            feat_shape, frame_shape = f.shape[1:], d.shape[1:]
        if f.shape[1:] != feat_shape or d.shape[1:] != frame_shape:
            raise ValueError(f"item {i}: frame shapes {f.shape[1:]} / {d.shape[1:]} differ from {feat_shape} / {frame_shape}")
        if len(f):
            rgb.append((f, None))
        if len(d):
            dep.append((d, None))
        len_f.append(len(f)), len_d.append(len(d)), labels.append((pl, dur, tgt))
    return ClipPlan(rgb, dep, feat_shape or (0,), frame_shape or (0,), np.arange(sum(len_f), dtype=np.int64), len_f,
                    np.arange(sum(len_d), dtype=np.int64), len_d, labels, pad_idx)


def _upload(pool, segments, chunk_bytes=CHUNK_BYTES):
    """Fills pool [F, row] (device fp32) from the segments through two alternating pinned chunks: host memory holds at most
    2 * chunk_bytes of frames, whatever the pool's size.  .npy sources are memory-mapped one file at a time."""
    F, row = pool.shape
    if F == 0:
        return
    per = max(1, chunk_bytes // (4 * row))
    stream = torch.cuda.current_stream(pool.device)
    bufs = [torch.empty((min(per, F), row), dtype=torch.float32, pin_memory=True) for _ in range(2)]
    done = [None, None]
    k, n, dst = 0, 0, 0

    def flush():
        nonlocal k, n, dst
        with torch.cuda.stream(stream):
            pool[dst:dst + n].copy_(bufs[k][:n], non_blocking=True)
        done[k] = stream.record_event()
        dst, n, k = dst + n, 0, 1 - k
        if done[k] is not None:
            done[k].synchronize()                   # the other buffer's copy has left it: refill

    for src, rows in segments:
        arr = np.load(src, mmap_mode="r") if isinstance(src, str) else src
        total = len(rows) if rows is not None else len(arr)
        pos = 0
        while pos < total:
            take = min(total - pos, bufs[k].shape[0] - n)
            part = arr[rows[pos:pos + take]] if rows is not None else arr[pos:pos + take]
            bufs[k].numpy()[n:n + take] = np.asarray(part).reshape(take, row)
            n, pos = n + take, pos + take
            if n == bufs[k].shape[0]:
                flush()
        del arr
    if n:
        flush()
    stream.synchronize()


class ClipStore:
    """The frame pools and per-item tables of a ClipPlan on one device; collate() gathers a padded batch in one launch."""

    def __init__(self, plan, device, budget=None):
        plan.check_capacity(device, budget)
        dev = torch.device(device)
        if dev.index is None:
            dev = torch.device(dev.type, torch.cuda.current_device())
        self.plan, self.device = plan, dev
        self.rgb_pool = torch.empty((plan.F_rgb, plan.D), dtype=torch.float32, device=dev)
        self.depth_pool = torch.empty((plan.F_dep, plan.P), dtype=torch.float32, device=dev)
        _upload(self.rgb_pool, plan.rgb_src)
        _upload(self.depth_pool, plan.dep_src)

        def table(a):                                   # (never empty: a NULL pointer is what the ABI rejects)
            t = torch.from_numpy(np.ascontiguousarray(a)) if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype)
            return t.to(dev)
        self.t = {k: table(getattr(plan, k)) for k in
                  ("off_f", "ids_f", "off_d", "ids_d", "off_l", "lab", "off_q", "q_dur", "q_tgt")}
        plan.rgb_src = plan.dep_src = None              # (from_dataset: the host frames are released)
        self._lib = _lib.load()

    @classmethod
    def from_specs(cls, clips, labels, pad_idx, device, budget=None):
        """clips[i]: NpyClipReader's spec (feature_file, depth_file, start, stop, step[, depth_offset[, depth_end]]);
        labels[i] = (past_label, trans_future_dur, trans_future_target).  Frames deduplicated by (file, row)."""
        return cls(plan_specs(clips, labels, pad_idx), device, budget)

    @classmethod
    def from_dataset(cls, dataset, pad_idx, device, budget=None):
        """Any map-style dataset of the reference's items (dict or my_collate-ordered 5-sequence); read once, frames not
        deduplicated."""
        return cls(plan_dataset(dataset, pad_idx), device, budget)

    def __len__(self):
        return len(self.plan)

    @property
    def nbytes(self):
        return self.plan.nbytes

    def sizes(self, idx):
        return self.plan.sizes(idx)

    def empty_batch(self, B, sizes):
        """Uninitialised outputs of a batch of B items with padded extents `sizes` (on the current stream)."""
        S_f, S_d, S_l, S_q = sizes
        f32, i64, dev = torch.float32, torch.int64, self.device
        return [torch.empty((B, S_f) + self.plan.feat_shape, dtype=f32, device=dev),
                torch.empty((B, S_d) + self.plan.frame_shape, dtype=f32, device=dev),
                torch.empty((B, S_l), dtype=i64, device=dev), torch.empty((B, S_q), dtype=f32, device=dev),
                torch.empty((B, S_q), dtype=i64, device=dev)]

    def launch(self, items, sizes, out, stream=None):
        """Enqueue the collate of `items` (int64 device tensor of item ids) into `out` (empty_batch's five tensors) on
        `stream` (default: the current one).  Enqueue only: capturable into a hipGraph."""
        p, t = self.plan, self.t
        assert items.device == self.device and items.dtype == torch.int64 and items.is_contiguous()
        S_f, S_d, S_l, S_q = sizes
        j = _lib.ClipCollateJob(
            rgb_pool=self.rgb_pool.data_ptr(), F_rgb=p.F_rgb, D=p.D, depth_pool=self.depth_pool.data_ptr(), F_dep=p.F_dep,
            P=p.P, n_items=len(p), items=items.data_ptr(), B=items.numel(), S_f=S_f, S_d=S_d, S_l=S_l, S_q=S_q,
            pad_idx=p.pad_idx, **{k: v.data_ptr() for k, v in t.items()},
            **{k: o.data_ptr() for k, o in zip(("features", "depth", "past_label", "trans_future_dur", "trans_future_target"),
                                                out)})
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        _lib.check(self._lib.r3d_clip_collate(C.byref(j), C.c_void_p(s.cuda_stream)), "r3d_clip_collate")
        return out

    def collate(self, idx):
        """The padded batch [features, depth, past_label, trans_future_dur, trans_future_target] of the item ids `idx`
        (host sequence), allocated and enqueued on the current stream.  The padded extents come from the host's lengths:
        nothing is read back from the device."""
        idx = np.asarray(idx, np.int64).reshape(-1)
        sizes = self.sizes(idx)
        out = self.empty_batch(len(idx), sizes)
        if idx.size:
            items = torch.from_numpy(idx).pin_memory().to(self.device, non_blocking=True)
        else:
            items = torch.empty(0, dtype=torch.int64, device=self.device)
        return self.launch(items, sizes, out)


class DeviceClipLoader:
    """torch.utils.data.DataLoader over a ClipStore: the same batch order (BatchSampler over `sampler`, or over
    RandomSampler(generator=...) / SequentialSampler), each batch collated on the device by one launch, and the collate
    of batch t+1 enqueued on a side stream while the consumer runs step t.  Outputs come from the caching allocator on
    the side stream and are record_stream'ed onto the consumer's stream: a yielded batch is never overwritten.

    `store` may be a host-only ClipPlan for the batch order alone (index_batches(), len())."""

    def __init__(self, store, batch_size, shuffle=False, sampler=None, generator=None, drop_last=False):
        if sampler is not None and shuffle:
            raise ValueError("sampler option is mutually exclusive with shuffle")
        self.store = store
        if sampler is None:
            n = range(len(store))
            sampler = RandomSampler(n, generator=generator) if shuffle else SequentialSampler(n)
        self.sampler = sampler
        self.batch_sampler = BatchSampler(sampler, batch_size, drop_last)
        self._side = None

    def set_epoch(self, epoch):
        if hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def __len__(self):
        return len(self.batch_sampler)

    def index_batches(self):
        return iter(self.batch_sampler)

    def __iter__(self):
        store = self.store
        dev = store.device
        if self._side is None:
            self._side = torch.cuda.Stream(dev)
        side = self._side

        def stage(idx):
            with torch.cuda.stream(side):
                out = store.collate(idx)
                ev = torch.cuda.Event()
                ev.record(side)
            return out, ev

        it = self.index_batches()
        idx = next(it, None)
        nxt = stage(idx) if idx is not None else None
        while nxt is not None:
            out, ev = nxt
            consumer = torch.cuda.current_stream(dev)
            consumer.wait_event(ev)
            for t in out:
                t.record_stream(consumer)
            idx = next(it, None)                        # enqueue the following collate before handing this batch out
            nxt = stage(idx) if idx is not None else None
            yield out
