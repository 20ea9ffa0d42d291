"""Device-resident clip store: the whole training set in HBM, batches collated on the device by ONE kernel launch
(csrc/clipcache.hip).  Drop-in for the DataLoader of every training loop: `train()` / `validate()` take a DeviceClipLoader
unchanged.

Why it works (data/basedataset_darai_depth.py:84-206): an item (video, seq_idx, obs_perc) is deterministic -- rows
0:observed_len:sample_rate of the feature file, the same rows of the depth file after its start_frame:end_frame+1 trim,
and fixed label / transcript arrays -- and only the shuffle order changes between epochs.  So the frames are uploaded
once, as fp32 (lossless against the reference's torch.tensor(..., dtype=float32)), and a batch is a row gather plus
padding on the device: no host copy, no PCIe transfer per step.

A batch is described by a LAYOUT: an ordered list of tracks, one per tensor of the batch.  A `frames` track is fp32 rows
gathered from a pool of its own; a `words` track is one int64 or fp32 word per position.  Every track names the length group
it belongs to: the tracks of a group share their per-item length and so their padded extent.

    LAYOUT_DEPTH                [features, depth_features, past_label, trans_future_dur, trans_future_target]    (the default:
                                basedataset_darai_depth.my_collate; train_proposed_depth with the two-modality models)
    layout_query(query_pad_idx) [features, past_label, trans_future_dur, trans_future_target, query_label]       (basedataset_darai /
                                _proposed_breakfast / _proposed_50salads: train_unsupervised, train_tcn)
    LAYOUT_GAZE                 LAYOUT_DEPTH + [gaze [S_g, gaze_dim]]                    (train_proposed_depth, three modalities)

    store = ClipStore.from_specs(clips, labels, pad_idx, "cuda", layout=...)  # per-clip .npy specs (NpyClipReader's), deduplicated
    store = ClipStore.from_dataset(dataset, pad_idx, "cuda", layout=...)      # any map-style dataset of the reference's items
    loader = DeviceClipLoader(store, batch_size, shuffle=True)                # yields the layout's tensors, in its order

Both constructors first build a host-only ClipPlan (pool rows, CSR tables, per-item lengths, bytes), check it against
free device memory, then allocate and upload.  Any layout collates through r3d_clip_collate_tracks; LAYOUT_DEPTH launches
the entry named by DEPTH_LAYOUT_ENTRY (both give the same bits)."""
import collections
import ctypes as C
import os

import numpy as np
import torch
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler

from . import _lib
from .utils import NpyClipReader

MARGIN_BYTES = 1 << 30           # left free beside the store (the step's own buffers, the allocator's slack)
CHUNK_BYTES = 64 << 20           # pinned staging per upload chunk (two of them alternate)
# What LAYOUT_DEPTH launches.  tools/clip_tracks_speed.py times both entries (profiles/clip_tracks_speed.json): the tracks entry
# is faster at (8, 16), level at (8, 1142) and 0.7 % slower at (16, 256), beyond the rounds' spread -- so the default stayed.
DEPTH_LAYOUT_ENTRY = "r3d_clip_collate"


class Track(collections.namedtuple("Track", "name kind dtype pad group")):
    """One tensor of a batch.  name: the key of the reference's item dict; kind: "frames" (fp32 rows [S, *frame shape] gathered
    from a pool) or "words" ([S] words); dtype: torch.float32, or torch.int64 for words; pad: the value written past an item's
    length (None: the store's pad_idx; cast to float for fp32 tracks); group: the tracks of one group share their length."""
    __slots__ = ()


class Layout(tuple):
    """An ordered tuple of Tracks with a name (used in error messages).  A frames track is alone in its group (its pool ids
    are the group's table); word tracks may share one (trans_future_dur and trans_future_target are padded together)."""

    def __new__(cls, name, tracks):
        self = super().__new__(cls, tracks)
        self.name = str(name)
        if len(self) > _lib.CLIP_MAX_TRACKS:
            raise ValueError(f"layout {name}: {len(self)} tracks, the collate launch takes {_lib.CLIP_MAX_TRACKS}")
        if len({t.name for t in self}) != len(self):
            raise ValueError(f"layout {name}: track names repeat")
        for t in self:
            if (t.kind, t.dtype) not in (("frames", torch.float32), ("words", torch.float32), ("words", torch.int64)):
                raise ValueError(f"layout {name}: track {t.name} is {t.kind} of {t.dtype}; frames are float32, words float32 or int64")
            if t.kind == "frames" and sum(u.group == t.group for u in self) != 1:
                raise ValueError(f"layout {name}: the frames track {t.name} shares its length group {t.group!r}")
        self.groups = tuple(dict.fromkeys(t.group for t in self))          # in order of first appearance: sizes()'s order
        self.frames = tuple(t for t in self if t.kind == "frames")
        self.words = tuple(t for t in self if t.kind == "words")
        return self


_F32, _I64 = torch.float32, torch.int64
LAYOUT_DEPTH = Layout("depth", [Track("features", "frames", _F32, 0, "f"), Track("depth_features", "frames", _F32, 0, "d"),
                                Track("past_label", "words", _I64, None, "l"), Track("trans_future_dur", "words", _F32, None, "q"),
                                Track("trans_future_target", "words", _I64, None, "q")])
LAYOUT_GAZE = Layout("gaze", tuple(LAYOUT_DEPTH) + (Track("gaze", "frames", _F32, 0, "g"),))


def layout_query(query_pad_idx):
    """[features, past_label, trans_future_dur, trans_future_target, query_label]: the per-frame L3 label is padded with
    query_pad_idx and keeps a length of its own (the 50salads items carry an empty one)."""
    q = int(query_pad_idx)
    return Layout(f"query(pad {q})", [LAYOUT_DEPTH[0], LAYOUT_DEPTH[2], LAYOUT_DEPTH[3], LAYOUT_DEPTH[4],
                                      Track("query_label", "words", _I64, q, "x")])


_TABLE = {"past_label": "lab", "trans_future_dur": "q_dur", "trans_future_target": "q_tgt"}     # device-table names (ClipStore.t)
_NP = {torch.float32: np.float32, torch.int64: np.int64}


def _csr(lengths):
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(np.asarray(lengths, np.int64), out=off[1:])
    return off


class ClipPlan:
    """Host-only description of a store (no GPU needed), for one layout.

    Per frames track (dicts keyed by the track's name): `src` a list of segments (source, rows) whose rows, concatenated,
    are the pool's rows in order -- source is a `.npy` path (rows: file row indices) or an in-memory array (rows None: all
    of it); `shape` the frame shape, `width` its floats, `F` the pool's rows, `ids` (int64) the pool rows of every item's
    frames, item after item.  Per word track: `words[name]` the items' words, concatenated (int64 or fp32).
    Per length group: `lens[group]` the per-item lengths, from which each batch's padded sizes are taken on the host, and
    `offs[group]` their CSR.
    With LAYOUT_DEPTH (and wherever a layout has the track) the tables also go by their short names: rgb_src / dep_src,
    feat_shape / frame_shape, D / P, F_rgb / F_dep, off_f / ids_f, off_d / ids_d, off_l / lab, off_q / q_dur / q_tgt, len_f,
    len_d, len_l, len_q."""

    def __init__(self, layout, pad_idx, frames, words):
        """frames: {track name: (segments, frame shape, ids, per-item lengths)}; words: per item, the arrays of the layout's
        word tracks in their order."""
        self.layout, self.pad_idx = layout, int(pad_idx)
        self.src, self.shape, self.width, self.F, self.ids, self.words, self.lens = {}, {}, {}, {}, {}, {}, {}
        words = list(words)
        n = len(words)
        for t in layout.frames:
            seg, shape, ids, lens = frames[t.name]
            if len(lens) != n:
                raise ValueError(f"layout {layout.name}: {len(lens)} clips of {t.name} but {n} label tuples: clips and labels "
                                 "differ in number")
            self.src[t.name], self.shape[t.name] = seg, tuple(int(x) for x in shape)
            self.width[t.name] = int(np.prod(self.shape[t.name]))
            self.F[t.name] = int(sum(len(r) if r is not None else len(s) for s, r in seg))
            self.ids[t.name], self.lens[t.group] = np.asarray(ids, np.int64), np.asarray(lens, np.int64)
        cols = {t.name: [] for t in layout.words}
        glen = {t.group: [] for t in layout.words}
        for i, w in enumerate(words):
            if len(w) != len(layout.words):
                raise ValueError(f"layout {layout.name}, item {i}: {len(w)} label arrays, the layout's word tracks are "
                                 f"{[t.name for t in layout.words]}")
            seen = {}
            for t, a in zip(layout.words, w):
                a = (a.numpy() if torch.is_tensor(a) else np.asarray(a)).reshape(-1).astype(_NP[t.dtype])
                first = seen.setdefault(t.group, t.name)
                if first != t.name and a.size != cols[first][-1].size:
                    raise ValueError(f"layout {layout.name}, item {i}: {first} has {cols[first][-1].size} entries and {t.name} "
                                     f"{a.size}; the store keeps one length for both (the reference pads both to n_query)")
                cols[t.name].append(a)
            for g, first in seen.items():
                glen[g].append(cols[first][-1].size)
        for t in layout.words:
            self.words[t.name] = np.concatenate(cols[t.name]) if cols[t.name] else np.zeros(0, _NP[t.dtype])
            self.lens[t.group] = np.asarray(glen[t.group], np.int64)
        self.offs = {g: _csr(v) for g, v in self.lens.items()}
        self._n = n

    def __len__(self):
        return self._n

    # ---- the short names of the tables (those of LAYOUT_DEPTH; a layout without the track raises KeyError)
    rgb_src = property(lambda s: s.src["features"], lambda s, v: s.src.__setitem__("features", v))
    dep_src = property(lambda s: s.src["depth_features"], lambda s, v: s.src.__setitem__("depth_features", v))
    feat_shape, frame_shape = property(lambda s: s.shape["features"]), property(lambda s: s.shape["depth_features"])
    D, P = property(lambda s: s.width["features"]), property(lambda s: s.width["depth_features"])
    F_rgb, F_dep = property(lambda s: s.F["features"]), property(lambda s: s.F["depth_features"])
    ids_f, ids_d = property(lambda s: s.ids["features"]), property(lambda s: s.ids["depth_features"])
    lab, q_dur = property(lambda s: s.words["past_label"]), property(lambda s: s.words["trans_future_dur"])
    q_tgt = property(lambda s: s.words["trans_future_target"])
    len_f, len_d = property(lambda s: s.lens["f"]), property(lambda s: s.lens["d"])
    len_l, len_q = property(lambda s: s.lens["l"]), property(lambda s: s.lens["q"])
    off_f, off_d = property(lambda s: s.offs["f"]), property(lambda s: s.offs["d"])
    off_l, off_q = property(lambda s: s.offs["l"]), property(lambda s: s.offs["q"])

    def tables(self):
        """{device-table name: host array}: off_<group> per length group, ids_<group> per frames track, and each word track's
        table (lab, q_dur, q_tgt; any other by the track's name)."""
        t = {}
        for tr in self.layout:
            t[f"off_{tr.group}"] = self.offs[tr.group]
            if tr.kind == "frames":
                t[f"ids_{tr.group}"] = self.ids[tr.name]
            else:
                t[_TABLE.get(tr.name, tr.name)] = self.words[tr.name]
        return t

    @property
    def nbytes(self):
        """Device bytes of the store: every pool (fp32) and every table."""
        return (4 * sum(self.F[t.name] * self.width[t.name] for t in self.layout.frames) +
                sum(max(a.size, 1) * a.itemsize for a in self.tables().values()))

    def sizes(self, idx):
        """Padded extents of a batch of item ids, one per length group in the layout's order -- (S_f, S_d, S_l, S_q) for
        LAYOUT_DEPTH: the per-tensor maxima pad_sequence pads to."""
        idx = np.asarray(idx, np.int64)
        if idx.size == 0:
            return (0,) * len(self.layout.groups)
        return tuple(int(self.lens[g][idx].max()) for g in self.layout.groups)

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


_SPEC_FRAMES = ("features", "depth_features", "gaze")


def plan_specs(clips, labels, pad_idx, layout=LAYOUT_DEPTH):
    """ClipPlan of NpyClipReader clip specs (feature_file, depth_file, start, stop, step[, depth_offset[, depth_end]]) and, per
    clip, the tuple of its word arrays in the layout's order ((past_label, trans_future_dur, trans_future_target) for
    LAYOUT_DEPTH; a fourth, query_label, for layout_query).  A layout with a gaze track takes the clip's gaze `.npy`
    [rows, gaze_dim] as the spec's LAST element; its rows are the clip's own file[start:stop:step].  A layout without a depth
    track ignores the spec's depth_file (None will do).
    Frames are deduplicated by (file, row): items that share a prefix (DARai's 0.2 / 0.3 / 0.5 observations of one
    sequence) share pool rows, and only rows some item samples are stored.  Files are only opened for their shapes."""
    clips, labels = list(clips), list(labels)
    if len(clips) != len(labels):
        raise ValueError(f"layout {layout.name}: {len(clips)} clips but {len(labels)} label tuples")
    names = [t.name for t in layout.frames]
    if any(n not in _SPEC_FRAMES for n in names):
        raise ValueError(f"layout {layout.name}: clip specs carry {_SPEC_FRAMES}, not {names}; use from_dataset")
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

    rows, fshape = {n: [] for n in names}, {}
    for i, c in enumerate(clips):
        c = tuple(c)
        files = {}
        if "gaze" in names:
            if len(c) < 6 or not isinstance(c[-1], (str, os.PathLike)):
                raise ValueError(f"layout {layout.name}, clip {i}: the spec's last element must be the gaze .npy file, got {c!r}")
            files["gaze"], c = c[-1], c[:-1]
        if not 5 <= len(c) <= 7:
            raise ValueError(f"layout {layout.name}, clip {i}: a spec is (feature_file, depth_file, start, stop, step[, "
                             f"depth_offset[, depth_end]]) with the gaze file, if the layout has one, after it; got {len(c)} "
                             "such elements")
        files["features"], files["depth_features"] = c[0], c[1]
        for n in names:
            key, sh = shape(files[n])
            if fshape.setdefault(n, sh[1:]) != sh[1:]:
                raise ValueError(f"layout {layout.name}, clip {i}: {n} frames of shape {sh[1:]} in {files[n]}, {fshape[n]} in "
                                 "the clips before it")
            rows[n].append((key, NpyClipReader._rows(sh[0], c[2], c[3], c[4], *(c[5:7] if n == "depth_features" else ()))))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)       # noqa: E731
    frames = {}
    for n in names:
        seg, ids = pool(rows[n])
        frames[n] = (seg, fshape.get(n, (0,)), cat(ids), [len(r) for _, r in rows[n]])
    return ClipPlan(layout, pad_idx, frames, labels)


def plan_dataset(dataset, pad_idx, layout=LAYOUT_DEPTH):
    """ClipPlan of a map-style dataset whose items are the reference's item dict (basedataset_darai_depth.py:174-180; the keys
    are the layout's track names) or the tensors in the layout's (my_collate's) order.  Each item is read once and its frames
    are kept as the dataset returned them until the upload; they are NOT deduplicated (the dataset hides which file rows an
    item came from)."""
    keys = [t.name for t in layout]
    segs, lens, fshape, words = {t.name: [] for t in layout.frames}, {t.name: [] for t in layout.frames}, {}, []
    for i in range(len(dataset)):
        it = dataset[i]
        if isinstance(it, dict):
            if any(k not in it for k in keys):
                raise ValueError(f"layout {layout.name}, item {i}: the item's keys {sorted(it)} lack "
                                 f"{[k for k in keys if k not in it]}")
            it = [it[k] for k in keys]
        if len(it) != len(keys):
            raise ValueError(f"layout {layout.name}, item {i}: {len(it)} elements, the layout has {len(keys)}: {keys}")
        it = [x.numpy() if torch.is_tensor(x) else np.asarray(x) for x in it]
        for t, x in zip(layout, it):
            if t.kind != "frames":
                continue
            if x.ndim < 2 or fshape.setdefault(t.name, x.shape[1:]) != x.shape[1:]:
                raise ValueError(f"layout {layout.name}, item {i}: {t.name} of shape {x.shape}, frames of shape "
                                 f"{fshape.get(t.name, '[S, ...]')} in the items before it")
            if len(x):
                segs[t.name].append((x, None))
            lens[t.name].append(len(x))
        words.append([x for t, x in zip(layout, it) if t.kind == "words"])
    frames = {n: (segs[n], fshape.get(n, (0,)), np.arange(sum(lens[n]), dtype=np.int64), lens[n]) for n in segs}
    return ClipPlan(layout, pad_idx, frames, words)


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
        self.layout = plan.layout
        self.pools = {}                                 # track name -> [F, width] fp32
        for t in plan.layout.frames:
            self.pools[t.name] = torch.empty((plan.F[t.name], plan.width[t.name]), dtype=torch.float32, device=dev)
            _upload(self.pools[t.name], plan.src[t.name])
            plan.src[t.name] = None                     # (from_dataset: the host frames are released)

        def table(a):                                   # (never empty: a NULL pointer is what the ABI rejects)
            t = torch.from_numpy(np.ascontiguousarray(a)) if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype)
            return t.to(dev)
        self.t = {k: table(a) for k, a in plan.tables().items()}
        self._lib = _lib.load()
        # the tracks job, filled once: a launch sets items, B, and each track's S and out
        self._job = j = _lib.ClipTracksJob(n_items=len(plan), n_tracks=len(plan.layout))
        for k, t in zip(j.tracks, plan.layout):
            k.off, k.pad = self.t[f"off_{t.group}"].data_ptr(), plan.pad_idx if t.pad is None else int(t.pad)
            if t.kind == "frames":
                k.kind, k.src, k.ids = _lib.CLIP_FRAMES_F32, self.pools[t.name].data_ptr(), self.t[f"ids_{t.group}"].data_ptr()
                k.rows, k.width = plan.F[t.name], plan.width[t.name]
            else:
                k.kind = _lib.CLIP_WORDS_I64 if t.dtype == torch.int64 else _lib.CLIP_WORDS_F32
                k.src, k.rows, k.width = self.t[_TABLE.get(t.name, t.name)].data_ptr(), plan.words[t.name].size, 1

    rgb_pool = property(lambda s: s.pools["features"])
    depth_pool = property(lambda s: s.pools["depth_features"])

    @classmethod
    def from_specs(cls, clips, labels, pad_idx, device, budget=None, layout=LAYOUT_DEPTH):
        """clips[i]: NpyClipReader's spec (feature_file, depth_file, start, stop, step[, depth_offset[, depth_end]]), with the
        clip's gaze file as its last element for a layout with a gaze track; labels[i]: the clip's word arrays in the
        layout's order -- (past_label, trans_future_dur, trans_future_target), and query_label for layout_query.  Frames
        deduplicated by (file, row)."""
        return cls(plan_specs(clips, labels, pad_idx, layout), device, budget)

    @classmethod
    def from_dataset(cls, dataset, pad_idx, device, budget=None, layout=LAYOUT_DEPTH):
        """Any map-style dataset of the reference's items (the dict with the layout's keys, or a sequence in the layout's
        order); read once, frames not deduplicated."""
        return cls(plan_dataset(dataset, pad_idx, layout), device, budget)

    def __len__(self):
        return len(self.plan)

    @property
    def nbytes(self):
        return self.plan.nbytes

    def sizes(self, idx):
        return self.plan.sizes(idx)

    def empty_batch(self, B, sizes):
        """Uninitialised outputs of a batch of B items with padded extents `sizes` (on the current stream)."""
        S = dict(zip(self.layout.groups, sizes, strict=True))
        return [torch.empty((B, S[t.group]) + (self.plan.shape[t.name] if t.kind == "frames" else ()), dtype=t.dtype,
                            device=self.device) for t in self.layout]

    def launch(self, items, sizes, out, stream=None, entry=None):
        """Enqueue the collate of `items` (int64 device tensor of item ids) into `out` (empty_batch's tensors) on `stream`
        (default: the current one).  Enqueue only: capturable into a hipGraph.  entry: "r3d_clip_collate_tracks", or for
        LAYOUT_DEPTH "r3d_clip_collate" (None: DEPTH_LAYOUT_ENTRY for LAYOUT_DEPTH, the tracks entry otherwise)."""
        p, t = self.plan, self.t
        assert items.device == self.device and items.dtype == torch.int64 and items.is_contiguous()
        assert len(out) == len(self.layout)
        if entry is None:
            entry = DEPTH_LAYOUT_ENTRY if self.layout is LAYOUT_DEPTH else "r3d_clip_collate_tracks"
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if entry == "r3d_clip_collate":
            if self.layout is not LAYOUT_DEPTH:
                raise ValueError(f"layout {self.layout.name}: r3d_clip_collate writes LAYOUT_DEPTH's five tensors only")
            S_f, S_d, S_l, S_q = sizes
            j = _lib.ClipCollateJob(
                rgb_pool=self.rgb_pool.data_ptr(), F_rgb=p.F_rgb, D=p.D, depth_pool=self.depth_pool.data_ptr(), F_dep=p.F_dep,
                P=p.P, n_items=len(p), items=items.data_ptr(), B=items.numel(), S_f=S_f, S_d=S_d, S_l=S_l, S_q=S_q,
                pad_idx=p.pad_idx, **{k: v.data_ptr() for k, v in t.items()},
                **{k: o.data_ptr() for k, o in zip(("features", "depth", "past_label", "trans_future_dur",
                                                    "trans_future_target"), out)})
        elif entry == "r3d_clip_collate_tracks":
            S = dict(zip(self.layout.groups, sizes, strict=True))
            j = self._job
            j.items, j.B = items.data_ptr(), items.numel()
            for k, tr, o in zip(j.tracks, self.layout, out):
                k.S, k.out = S[tr.group], o.data_ptr()
        else:
            raise ValueError(f"no collate entry {entry!r}")
        _lib.check(getattr(self._lib, entry)(C.byref(j), C.c_void_p(s.cuda_stream)), entry)
        return out

    def collate(self, idx):
        """The padded batch of the item ids `idx` (host sequence): the layout's tensors in its order ([features, depth,
        past_label, trans_future_dur, trans_future_target] for LAYOUT_DEPTH), allocated and enqueued on the current stream.
        The padded extents come from the host's lengths: nothing is read back from the device."""
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
