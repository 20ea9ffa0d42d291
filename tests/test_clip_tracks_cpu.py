"""The clip store's layouts (r3d_amd/clipcache.py) without a GPU: a numpy restatement of the tracked collate over the host
plan against the reference's collate (pad_sequence per track) for LAYOUT_DEPTH, layout_query and LAYOUT_GAZE over the seven
ragged clips of test_clip_cache_cpu._write; deduplication of gaze rows; nbytes, sizes, the batch order; and the refusals, each
before anything touches a device."""
import numpy as np
import pytest
import torch
from torch.utils.data import BatchSampler, RandomSampler

from r3d_amd.clipcache import (LAYOUT_DEPTH, LAYOUT_GAZE, ClipStore, DeviceClipLoader, Layout, Track, layout_query, plan_dataset,
                               plan_specs)
from r3d_amd.utils import NpyClipReader
from tests.test_clip_cache_cpu import PAD, _reference_item, _specs, _write

QPAD = 47                                   # query_pad_idx != pad_idx
GAZE_ROWS = {"v0": 16, "v1": 2, "short": 30}
BATCHES = ([0, 1, 2, 3, 4, 5, 6], [3, 3, 1], [5], [2, 5, 0, 4], [6, 4], [6], [])


def make_case(tmp_path, kind, D=16, hw=(6, 8), gaze_dim=2):
    """(layout, clips, labels, items) of the seven clips of _specs for kind "depth" | "query" | "gaze".  items: the reference's
    items as lists in the layout's order (what its dataset returns), from the files.
    gaze: one `.npy` per video; v0's ends before its features do (clip 2 gets fewer gaze rows than feature rows), v1's has 2
    rows (clip 5 has frames but no gaze row), short's outlasts its depth file (clips 3 and 6: more gaze rows than depth frames).
    query: a per-frame label as long as the features, except clip 2's (3 entries longer) and clip 5's (empty)."""
    paths = _write(tmp_path, D=D, hw=hw)
    clips, labels = _specs(paths)
    base = [_reference_item(c, lab) for c, lab in zip(clips, labels)]
    rng = np.random.default_rng(21)
    if kind == "depth":
        return LAYOUT_DEPTH, clips, labels, base
    if kind == "query":
        ql = [rng.integers(0, QPAD, len(it[0]) + (3 if i == 2 else 0)) if i != 5 else np.zeros(0, np.int64)
              for i, it in enumerate(base)]
        labels = [lab + (q,) for lab, q in zip(labels, ql)]
        items = [[it[0], it[2], it[3], it[4], torch.tensor(q, dtype=torch.long)] for it, q in zip(base, ql)]
        return layout_query(QPAD), clips, labels, items
    assert kind == "gaze"
    gfile = {}
    for name, rows in GAZE_ROWS.items():
        gfile[paths[name][0]] = str(tmp_path / f"{name}_gaze.npy")
        np.save(gfile[paths[name][0]], rng.standard_normal((rows, gaze_dim)).astype(np.float32))
    clips = [c + (gfile[c[0]],) for c in clips]
    items = [it + [torch.tensor(np.load(c[-1])[c[2]:c[3]][::c[4]], dtype=torch.float32)] for it, c in zip(base, clips)]
    return LAYOUT_GAZE, clips, labels, items


def long_gaze_items(items):
    """The gaze items with clip 2's gaze track 3 rows LONGER than its features (a dataset may return that; a clip spec, which
    samples both files by one slice, cannot)."""
    g = torch.Generator().manual_seed(5)
    items = [list(it) for it in items]
    items[2][5] = torch.randn(items[2][0].shape[0] + 3, items[2][5].shape[1], generator=g)
    return items


def reference_collate(layout, items):
    """the reference's my_collate for the layout: pad_sequence per track"""
    pad = torch.nn.utils.rnn.pad_sequence
    if not items:
        return None
    return [pad([it[k] for it in items], batch_first=True, padding_value=PAD if t.pad is None else t.pad)
            for k, t in enumerate(layout)]


def equal(got, want, n):
    assert len(got) == len(want) == n
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), k


def _host_collate(plan, idx):
    """What r3d_clip_collate_tracks computes, restated in numpy over the host plan."""
    lay, B = plan.layout, len(idx)
    S = dict(zip(lay.groups, plan.sizes(idx)))
    out = []
    for t in lay:
        pad = PAD if t.pad is None else t.pad
        off = plan.offs[t.group]
        if t.kind == "frames":
            rows = [(np.load(s)[r] if isinstance(s, str) else s).reshape(-1, plan.width[t.name]) for s, r in plan.src[t.name]]
            pool = np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, plan.width[t.name]), np.float32)
            o = np.full((B, S[t.group], plan.width[t.name]), pad, np.float32)
            for b, i in enumerate(idx):
                r = plan.ids[t.name][off[i]:off[i + 1]]
                o[b, :len(r)] = pool[r]
            o = o.reshape((B, S[t.group]) + plan.shape[t.name])
        else:
            o = np.full((B, S[t.group]), pad, plan.words[t.name].dtype)
            for b, i in enumerate(idx):
                o[b, :off[i + 1] - off[i]] = plan.words[t.name][off[i]:off[i + 1]]
        out.append(torch.from_numpy(o))
    return out


@pytest.mark.parametrize("kind", ["depth", "query", "gaze"])
def test_host_collate_equals_reference_collate(tmp_path, kind):
    layout, clips, labels, items = make_case(tmp_path, kind)
    dicts = [dict(zip([t.name for t in layout], it)) for it in items]
    plans = [(plan_specs(clips, labels, PAD, layout), items), (plan_dataset(items, PAD, layout), items),
             (plan_dataset(dicts, PAD, layout), items)]
    if kind == "gaze":
        longer = long_gaze_items(items)
        assert len(longer[2][5]) > len(longer[2][0])
        plans.append((plan_dataset(longer, PAD, layout), longer))
    for plan, its in plans:
        assert plan.layout is layout and len(plan) == 7
        for idx in BATCHES[:-1]:
            equal(_host_collate(plan, idx), reference_collate(layout, [its[i] for i in idx]), len(layout))
        empty = _host_collate(plan, [])
        assert [tuple(e.shape[:2]) for e in empty] == [(0, 0)] * len(layout)
    if kind == "gaze":                          # the lengths the case promises
        p = plans[0][0]
        assert p.lens["g"][5] == 0 < p.lens["f"][5] and p.lens["g"][2] < p.lens["f"][2]
        assert p.lens["g"][3] > p.lens["d"][3] and p.lens["g"][6] > p.lens["d"][6] == 0
    if kind == "depth":                         # the default layout is what plan_specs / plan_dataset build without one
        q = plan_specs(clips, labels, PAD)
        assert q.layout is LAYOUT_DEPTH and q.sizes([0, 3]) == plans[0][0].sizes([0, 3]) and q.nbytes == plans[0][0].nbytes


def test_gaze_rows_are_deduplicated(tmp_path):
    layout, clips, labels, _ = make_case(tmp_path, "gaze", gaze_dim=3)
    plan = plan_specs(clips + clips[:2], labels + labels[:2], PAD, layout)     # repeated items add no rows
    want = set()
    for c in clips:
        want |= {(c[-1], r) for r in NpyClipReader._rows(np.load(c[-1], mmap_mode="r").shape[0], c[2], c[3], c[4])}
    assert plan.F["gaze"] == len(want) < int(plan.lens["g"].sum())             # clips 0, 1, 2 share v0's first rows
    assert plan.shape["gaze"] == (3,) and plan.width["gaze"] == 3
    pool = [(s, int(r)) for s, rows in plan.src["gaze"] for r in rows]         # pool row -> (file, file row)
    for i, c in enumerate(clips):
        got = [pool[p] for p in plan.ids["gaze"][plan.offs["g"][i]:plan.offs["g"][i + 1]]]
        assert [r for _, r in got] == list(NpyClipReader._rows(np.load(c[-1], mmap_mode="r").shape[0], c[2], c[3], c[4]))
        assert all(s.endswith(c[-1].split("/")[-1]) for s, _ in got)


@pytest.mark.parametrize("kind", ["depth", "query", "gaze"])
def test_nbytes_sizes_and_batch_order(tmp_path, kind):
    layout, clips, labels, _ = make_case(tmp_path, kind)
    plan = plan_specs(clips, labels, PAD, layout)
    n = len(clips)
    # nbytes: every pool (fp32) and every table, one CSR per length group (an empty table still takes one element)
    pools = sum(4 * plan.F[t.name] * plan.width[t.name] for t in layout.frames)
    csr = 8 * (n + 1) * len(layout.groups)
    ids = sum(8 * max(int(plan.lens[t.group].sum()), 1) for t in layout.frames)
    words = sum((8 if t.dtype == torch.int64 else 4) * max(int(plan.lens[t.group].sum()), 1) for t in layout.words)
    assert plan.nbytes == pools + csr + ids + words
    assert set(plan.tables()) >= {f"off_{g}" for g in layout.groups} and len(plan.tables()) == len(layout.groups) + len(layout)
    # sizes: the per-group maxima, in the layout's group order
    assert len(layout.groups) == {"depth": 4, "query": 4, "gaze": 5}[kind]
    for idx in BATCHES:
        want = tuple(max([int(plan.lens[g][i]) for i in idx], default=0) for g in layout.groups)
        assert plan.sizes(idx) == want
    if kind != "query":
        assert plan.sizes([0, 3])[:4] == plan_specs([c if kind == "depth" else c[:-1] for c in clips], labels, PAD).sizes([0, 3])
    # the batch order is the DataLoader's, whatever the layout
    for B, drop in ((3, False), (3, True)):
        got = list(DeviceClipLoader(plan, B, shuffle=True, generator=torch.Generator().manual_seed(7), drop_last=drop).index_batches())
        assert got == list(BatchSampler(RandomSampler(range(n), generator=torch.Generator().manual_seed(7)), B, drop))
        assert list(DeviceClipLoader(plan, B, drop_last=drop).index_batches()) == list(BatchSampler(range(n), B, drop))


def test_refusals_raise_without_a_device(tmp_path, monkeypatch):
    cases = {}
    for kind in ("depth", "query", "gaze"):
        (tmp_path / kind).mkdir()
        cases[kind] = make_case(tmp_path / kind, kind)

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    for kind, (layout, clips, labels, items) in cases.items():
        names = [t.name for t in layout]
        # a wrong element count / wrong keys
        bad = [list(it) for it in items]
        bad[3] = bad[3][:-1]
        with pytest.raises(ValueError, match=rf"layout {layout.name[:5]}.*item 3"):
            ClipStore.from_dataset(bad, PAD, "cuda", layout=layout)
        bad[3] = items[3] + [items[3][0]]
        with pytest.raises(ValueError, match=rf"layout {layout.name[:5]}.*item 3"):
            ClipStore.from_dataset(bad, PAD, "cuda", layout=layout)
        dicts = [dict(zip(names, it)) for it in items]
        dicts[2] = {("nope" if k == names[-1] else k): v for k, v in dicts[2].items()}
        with pytest.raises(ValueError, match=rf"layout {layout.name[:5]}.*item 2.*{names[-1]}"):
            ClipStore.from_dataset(dicts, PAD, "cuda", layout=layout)
        # a frame shape that differs between items
        for k, t in enumerate(layout):
            if t.kind != "frames":
                continue
            bad = [list(it) for it in items]
            bad[5][k] = torch.zeros((2,) + tuple(items[5][k].shape[1:]) + (2,))
            with pytest.raises(ValueError, match=rf"layout {layout.name[:5]}.*item 5.*{t.name}"):
                ClipStore.from_dataset(bad, PAD, "cuda", layout=layout)
        # a length mismatch inside a shared-length group (trans_future_dur / trans_future_target)
        k = names.index("trans_future_dur")
        bad = [list(it) for it in items]
        bad[4][k] = torch.cat([bad[4][k], bad[4][k][:1]])
        with pytest.raises(ValueError, match=rf"layout {layout.name[:5]}.*item 4.*trans_future_dur.*trans_future_target"):
            ClipStore.from_dataset(bad, PAD, "cuda", layout=layout)
        w = [t.name for t in layout.words].index("trans_future_dur")
        lab = [tuple(x) for x in labels]
        lab[1] = lab[1][:w] + (np.append(lab[1][w], 1.0),) + lab[1][w + 1:]
        with pytest.raises(ValueError, match=rf"layout {layout.name[:5]}.*item 1.*trans_future_dur"):
            ClipStore.from_specs(clips, lab, PAD, "cuda", layout=layout)
        # from_specs: a label tuple of the wrong length, clips and labels of different number
        lab = [tuple(x) for x in labels]
        lab[6] = lab[6][:-1]
        with pytest.raises(ValueError, match=rf"layout {layout.name[:5]}.*item 6"):
            ClipStore.from_specs(clips, lab, PAD, "cuda", layout=layout)
        with pytest.raises(ValueError, match=rf"layout {layout.name[:5]}"):
            ClipStore.from_specs(clips, labels[:-1], PAD, "cuda", layout=layout)
    # from_specs: frame files of different shapes; a gaze layout without the gaze file in the spec
    layout, clips, labels, _ = cases["gaze"]
    np.save(tmp_path / "g5.npy", np.zeros((9, 5), np.float32))
    bad = list(clips)
    bad[4] = bad[4][:-1] + (str(tmp_path / "g5.npy"),)
    with pytest.raises(ValueError, match=r"layout gaze, clip 4.*gaze"):
        ClipStore.from_specs(bad, labels, PAD, "cuda", layout=layout)
    with pytest.raises(ValueError, match=r"layout gaze, clip 0.*gaze"):
        ClipStore.from_specs([c[:-1] for c in clips], labels, PAD, "cuda", layout=layout)
    # a layout the launch cannot describe
    f32 = torch.float32
    with pytest.raises(ValueError, match="9 tracks"):
        Layout("nine", [Track(f"t{i}", "words", f32, 0, "g") for i in range(9)])
    with pytest.raises(ValueError, match="shares its length group"):
        Layout("shared", [Track("a", "frames", f32, 0, "g"), Track("b", "words", f32, 0, "g")])
    with pytest.raises(ValueError, match="frames are float32"):
        Layout("ints", [Track("a", "frames", torch.int64, 0, "g")])
