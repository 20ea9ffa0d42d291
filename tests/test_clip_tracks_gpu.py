"""The clip store's layouts on the GPU: r3d_clip_collate_tracks against the reference's collate (bitwise) for the query and
gaze layouts; the packed path's edges through the ABI (row widths on both sides of the wide-row threshold, a track that crosses
a 4096-element workgroup, a misaligned pool, repeated and out-of-range ids); the tracks entry against r3d_clip_collate on the
depth layout; the ABI's refusals; graph replay; and the L3, TCN and three-modality loops trained from a DeviceClipLoader
against the same batches handed over as a plain list."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from r3d_amd import _lib  # noqa: E402
from r3d_amd.clipcache import LAYOUT_DEPTH, LAYOUT_GAZE, ClipStore, DeviceClipLoader, layout_query  # noqa: E402
from tests.test_clip_cache_cpu import PAD, _reference_collate, _reference_item, _specs, _write  # noqa: E402
from tests.test_clip_tracks_cpu import BATCHES, equal, long_gaze_items, make_case, reference_collate  # noqa: E402

EINVAL = -1


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------
# layouts against the reference's collate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,D,gaze_dim", [("query", 16, 0), ("query", 37, 0)] +
                         [("gaze", D, g) for D in (16, 37) for g in (1, 2, 3, 8)])
def test_layout_equals_reference_collate(tmp_path, kind, D, gaze_dim):
    layout, clips, labels, items = make_case(tmp_path, kind, D=D, hw=(7, 9), gaze_dim=gaze_dim)
    stores = [(ClipStore.from_specs(clips, labels, PAD, "cuda", layout=layout), items),
              (ClipStore.from_dataset(items, PAD, "cuda", layout=layout), items)]
    if kind == "gaze":
        longer = long_gaze_items(items)                          # one gaze track longer than its clip's frames
        stores.append((ClipStore.from_dataset(longer, PAD, "cuda", layout=layout), longer))
    for store, its in stores:
        for idx in BATCHES:
            got = store.collate(idx)
            torch.cuda.synchronize()
            if idx:
                equal(got, reference_collate(layout, [its[i] for i in idx]), len(layout))
            else:                                                # B = 0
                assert [tuple(g.shape[:2]) for g in got] == [(0, 0)] * len(layout)
        loader = DeviceClipLoader(store, 3)
        for got, idx in zip(loader, loader.index_batches()):
            torch.cuda.synchronize()
            equal(got, reference_collate(layout, [its[i] for i in idx]), len(layout))


# ---------------------------------------------------------------------------------------------------------------------
# the packed path's edges, through the ABI
# ---------------------------------------------------------------------------------------------------------------------
_EDGE = {}


def _edge_tables():
    """Three items of 700, 350 and 0 rows over a pool of 500 rows (ids repeat; some are out of range), shared by every width."""
    if not _EDGE:
        rng = np.random.default_rng(17)
        lens = np.array([700, 350, 0], np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ids = rng.integers(0, 500, int(lens.sum())).astype(np.int64)
        ids[[5, 699, 700, 1049]] = [-1, 500, 1 << 40, -(1 << 35)]          # pool ids out of range: padding rows
        _EDGE.update(lens=lens, off=off, ids=ids, pool=rng.standard_normal(500 * 257 + 1).astype(np.float32))
    return _EDGE


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("width", [1, 2, 3, 8, 63, 64, 65, 255, 256, 257])
def test_one_frame_track_through_the_abi(width, misaligned):
    lib, e = _lib.load(), _edge_tables()
    B, S, F, pad = 3, 700, 500, -3
    buf = torch.from_numpy(e["pool"]).cuda()
    pool = buf[1:1 + F * width] if misaligned else buf[:F * width]       # (a pool base one float off a 16-byte boundary)
    assert (pool.data_ptr() % 16 != 0) == misaligned
    off, ids = torch.from_numpy(e["off"]).cuda(), torch.from_numpy(e["ids"]).cuda()
    host_pool = pool.cpu().view(F, width)
    for item_ids in ([1, 1, 0], [0, 3, -1], [2, 0, 1 << 33]):              # repeated items; item ids out of range; an empty item
        items = torch.tensor(item_ids, dtype=torch.int64, device="cuda")
        out = torch.full((B, S, width), 123.0, device="cuda")
        j = _lib.ClipTracksJob(items=items.data_ptr(), B=B, n_items=3, n_tracks=1)
        k = j.tracks[0]
        k.kind, k.src, k.rows, k.width, k.off, k.ids = _lib.CLIP_FRAMES_F32, pool.data_ptr(), F, width, off.data_ptr(), ids.data_ptr()
        k.S, k.pad, k.out = S, pad, out.data_ptr()
        assert lib.r3d_clip_collate_tracks(C.byref(j), _stream()) == 0
        torch.cuda.synchronize()
        want = torch.full((B, S, width), float(pad))
        for b, it in enumerate(item_ids):
            if 0 <= it < 3:
                r = e["ids"][e["off"][it]:e["off"][it + 1]]
                ok = (r >= 0) & (r < F)
                rows = torch.full((len(r), width), float(pad))
                rows[torch.from_numpy(ok)] = host_pool[torch.from_numpy(r[ok])]
                want[b, :len(r)] = rows
        assert out.dtype == want.dtype and out.shape == want.shape and torch.equal(out.cpu(), want), (width, item_ids)
    assert B * S * 2 > 4096 and _lib.CLIP_WIDE_ROW == 256                 # width 2 crosses a workgroup; 255 / 256 the threshold


def test_word_tracks_through_the_abi():
    """An int64 and an fp32 word track that share one CSR, 4500 elements each (more than a workgroup's 4096), padded with a
    negative value; a table whose length is shorter than the CSR claims reads nothing past it."""
    lib = _lib.load()
    rng = np.random.default_rng(4)
    lens = np.array([1500, 0, 777], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wi, wf = rng.integers(-9, 9, int(lens.sum())), rng.standard_normal(int(lens.sum())).astype(np.float32)
    d_off, d_wi, d_wf = (torch.from_numpy(x).cuda() for x in (off, wi, wf))
    B, S, pad = 3, 1500, -2
    item_ids = [0, 2, 5]
    items = torch.tensor(item_ids, dtype=torch.int64, device="cuda")
    for rows in (int(lens.sum()), 2000):
        oi, of = torch.full((B, S), 55, dtype=torch.int64, device="cuda"), torch.full((B, S), 55.0, device="cuda")
        j = _lib.ClipTracksJob(items=items.data_ptr(), B=B, n_items=3, n_tracks=2)
        for k, kind, src, out in ((j.tracks[0], _lib.CLIP_WORDS_I64, d_wi, oi), (j.tracks[1], _lib.CLIP_WORDS_F32, d_wf, of)):
            k.kind, k.src, k.rows, k.width, k.off, k.S, k.pad, k.out = kind, src.data_ptr(), rows, 1, d_off.data_ptr(), S, pad, out.data_ptr()
        assert lib.r3d_clip_collate_tracks(C.byref(j), _stream()) == 0
        torch.cuda.synchronize()
        for got, w in ((oi, wi), (of, wf)):
            want = torch.full((B, S), pad, dtype=got.dtype)
            for b, it in enumerate(item_ids[:2]):
                seg = torch.from_numpy(w[off[it]:min(off[it + 1], rows)]).to(got.dtype)
                want[b, :len(seg)] = seg
            assert torch.equal(got.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# the tracks entry against r3d_clip_collate on the depth layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,hw", [(2048, (224, 224)), (2048, (120, 160)), (37, (7, 9)), (37, (67, 71)), (2048, (7, 9)),
                                  (37, (224, 224))])
def test_tracks_entry_equals_the_five_tensor_entry(tmp_path, D, hw):
    clips, labels = _specs(_write(tmp_path, D=D, hw=hw))
    store = ClipStore.from_specs(clips, labels, PAD, "cuda")
    assert store.layout is LAYOUT_DEPTH
    for idx in BATCHES:
        sizes = store.sizes(idx)
        items = torch.tensor(idx, dtype=torch.int64, device="cuda")
        outs = []
        for fill, entry in ((-7, "r3d_clip_collate"), (-9, "r3d_clip_collate_tracks")):
            out = store.empty_batch(len(idx), sizes)
            for t in out:
                t.fill_(fill)
            outs.append(store.launch(items, sizes, out, entry=entry))
        torch.cuda.synchronize()
        for a, b in zip(*outs):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
        if idx:
            equal(outs[1], _reference_collate([_reference_item(clips[i], labels[i]) for i in idx]), 5)
    with pytest.raises(ValueError, match="no collate entry"):
        store.launch(items, sizes, out, entry="r3d_nope")


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_tracks_abi_rejects_bad_arguments(tmp_path):
    lib = _lib.load()
    layout, clips, labels, items_ref = make_case(tmp_path, "gaze")
    store = ClipStore.from_specs(clips, labels, PAD, "cuda", layout=layout)
    idx = [0, 3]
    sizes = store.sizes(idx)
    items = torch.tensor(idx, dtype=torch.int64, device="cuda")
    out = store.empty_batch(2, sizes)
    store.launch(items, sizes, out)
    torch.cuda.synchronize()
    equal(out, reference_collate(layout, [items_ref[i] for i in idx]), 6)
    for t in out:
        t.fill_(-7)
    before = [t.clone() for t in out]

    def job(track=None, **kw):
        """the store's job with fields of the job, or of one track, replaced"""
        j = _lib.ClipTracksJob.from_buffer_copy(store._job)
        for k, v in kw.items():
            setattr(j.tracks[track] if track is not None else j, k, v)
        return lib.r3d_clip_collate_tracks(C.byref(j), _stream())
    assert lib.r3d_clip_collate_tracks(None, None) == EINVAL
    assert job(n_tracks=_lib.CLIP_MAX_TRACKS + 1) == EINVAL and job(n_tracks=-1) == EINVAL
    assert job(B=-1) == EINVAL and job(n_items=-1) == EINVAL and job(items=None) == EINVAL
    for t, tr in enumerate(layout):
        assert job(t, kind=3) == EINVAL and job(t, kind=-1) == EINVAL                      # an unknown kind
        assert job(t, width=0) == EINVAL and job(t, width=-4) == EINVAL                    # width <= 0 on a non-empty track
        assert job(t, S=-2) == EINVAL and job(t, rows=-1) == EINVAL
        assert job(t, src=None) == EINVAL and job(t, off=None) == EINVAL and job(t, out=None) == EINVAL
        if tr.kind == "frames":
            assert job(t, ids=None) == EINVAL
        else:
            assert job(t, width=2) == EINVAL                                                # words are one wide
    torch.cuda.synchronize()
    for a, b in zip(out, before):
        assert torch.equal(a, b)                                                            # nothing was enqueued
    # what is legal: no tracks, no items, an empty track with NULL pointers and no width
    assert job(n_tracks=0) == 0 and job(B=0, items=None) == 0
    torch.cuda.synchronize()
    for a, b in zip(out, before):
        assert torch.equal(a, b)
    j = _lib.ClipTracksJob.from_buffer_copy(store._job)
    j.tracks[5].S, j.tracks[5].out, j.tracks[5].src, j.tracks[5].ids, j.tracks[5].width = 0, None, None, None, 0
    assert lib.r3d_clip_collate_tracks(C.byref(j), _stream()) == 0
    torch.cuda.synchronize()
    equal(out[:5], reference_collate(layout, [items_ref[i] for i in idx])[:5], 5)
    assert torch.equal(out[5], before[5])


# ---------------------------------------------------------------------------------------------------------------------
# graph replay
# ---------------------------------------------------------------------------------------------------------------------
def test_gaze_layout_captured_in_a_graph_replays_the_eager_result(tmp_path):
    layout, clips, labels, items_ref = make_case(tmp_path, "gaze", D=64, hw=(30, 40), gaze_dim=2)
    store = ClipStore.from_specs(clips, labels, PAD, "cuda", layout=layout)
    idx = [2, 0, 3, 4, 1]
    sizes = store.sizes(idx)
    items = torch.tensor(idx, dtype=torch.int64, device="cuda")
    out = store.empty_batch(len(idx), sizes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        store.launch(items, sizes, out)                          # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        store.launch(items, sizes, out)
    for order in (idx, idx[::-1]):                               # same item set, same padded sizes
        items.copy_(torch.tensor(order, dtype=torch.int64))
        for t in out:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        eager = store.collate(order)
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
        equal(out, reference_collate(layout, [items_ref[i] for i in order]), 6)


# ---------------------------------------------------------------------------------------------------------------------
# the loops, trained from the store
# ---------------------------------------------------------------------------------------------------------------------
def _store_of(bs, layout, pad_idx, tmp_path, tag):
    """ClipStore.from_specs of the batches written as per-clip `.npy` files, with frames before and after each clip."""
    clips, labels = [], []
    for i, b in enumerate(bs):
        for c in range(b[0].shape[0]):
            S, pre, post = b[0].shape[1], 3 + c, 2
            files = {}
            for k, t in enumerate(layout):
                if t.kind == "frames":
                    x = b[k][c].numpy()
                    files[t.name] = str(tmp_path / f"{tag}{i}c{c}_{t.name}.npy")
                    np.save(files[t.name], np.concatenate([np.full((pre,) + x.shape[1:], 7.0, np.float32), x,
                                                           np.full((post,) + x.shape[1:], 9.0, np.float32)]))
            clips.append((files["features"], files.get("depth_features"), pre, pre + S, 1) +
                         ((files["gaze"],) if "gaze" in files else ()))
            labels.append(tuple(b[k][c].numpy() for k, t in enumerate(layout) if t.kind == "words"))
    return ClipStore.from_specs(clips, labels, pad_idx, "cuda", layout=layout)


def _loaders(train, val, layout, pad_idx, tmp_path):
    loader = DeviceClipLoader(_store_of(train, layout, pad_idx, tmp_path, "t"), train[0][0].shape[0])
    vloader = DeviceClipLoader(_store_of(val, layout, pad_idx, tmp_path, "v"), val[0][0].shape[0])
    assert len(loader) == len(train) and len(vloader) == len(val)
    for ld, bs in ((loader, train), (vloader, val)):
        for got, b in zip(ld, bs):
            torch.cuda.synchronize()
            equal(got, list(b), len(layout))
    return loader, vloader


class _NoSched:
    def step(self):
        pass


def test_l3_loop_trains_identically_from_the_store(tmp_path):
    from r3d_amd import train_unsupervised as TU
    from r3d_amd.optim import FlatAdamW
    from tests import l3_cases as LC
    from tests.helpers import load_fixture
    from tests.test_l3_gpu import _loop_args, build_model
    fx = load_fixture("l3_train_loop")
    m, c = fx["meta"], LC.STEP_BY_TAG["l3_tiny"]
    train = [LC.batch(c, m["seed"]), LC.batch(c, m["seed"] + 1), LC.batch(dict(c, B=3), m["seed"] + 50)]     # (the last: skipped)
    val = [LC.batch(dict(c, S=c["S"] + 1), m["seed"] + 100)]
    loader, vloader = _loaders(train, val, layout_query(47), m["pad_idx"], tmp_path)
    finals = []
    for cached in (False, True):
        model = build_model(fx)
        opt = FlatAdamW(model.parameters(), m["lr"], weight_decay=m["wd"])
        TU.train(_loop_args(1), model, loader if cached else train, opt, _NoSched(), torch.nn.MSELoss(reduction="none"),
                 str(tmp_path), m["pad_idx"], torch.device("cuda"), vloader if cached else val, m["seed"])
        torch.cuda.synchronize()
        finals.append(model.engine().arena.params.clone())
    assert torch.equal(finals[0], finals[1])


def test_tcn_loop_trains_identically_from_the_store(tmp_path):
    from r3d_amd import train_tcn as TT
    from r3d_amd.optim import FlatAdamW
    from tests import tcn_cases as TC
    from tests.helpers import load_fixture
    from tests.test_tcn_gpu import _loop_batch, _model
    fx = load_fixture(TC.TRAIN_LOOP["tag"])
    m = fx["meta"]

    def batch(B, S, seed):                   # the 50salads 5-tuple: a per-frame query label rides along (the loop ignores it)
        b = _loop_batch(m, B, S, seed)
        return b[:4] + ((b[1] * 3 + 1) % 19,)
    train = [batch(m["B"], m["S"], m["seed"] + i) for i in range(3)]
    val = [batch(2, m["val_S"], m["seed"] + 100), batch(1, m["val_S"], m["seed"] + 101)]
    loader, vloader = _loaders(train, val, layout_query(19), m["pad_idx"], tmp_path)

    class Args:
        epochs = 1
    finals = []
    for cached in (False, True):
        model = _model(fx)
        opt = FlatAdamW(model.parameters(), m["lr"], weight_decay=m["wd"])
        TT.train(Args(), model, loader if cached else train, vloader if cached else val, opt, _NoSched(), None, str(tmp_path),
                 m["pad_idx"], torch.device("cuda"))
        torch.cuda.synchronize()
        finals.append(model.engine().arena.params.clone())
    assert torch.equal(finals[0], finals[1])


def test_three_modality_loop_trains_identically_from_the_store(tmp_path):
    from tests import m3_cases as MC
    from tests.test_m3_gpu import _train
    c = MC._step("loop", 8, 6, 64, 4, 17, 1, 256, 80)
    train = [MC.batch(c, seed=80), MC.batch(c, seed=82), MC.batch(c, seed=81, B=3)]          # (the last: skipped, 3 < 8)
    val = [MC.batch(c, seed=90, B=2, S=7)]
    loader, vloader = _loaders(train, val, LAYOUT_GAZE, MC.pad_idx(c), tmp_path)
    m_list, text_list = _train(c, tmp_path / "list", [], train, val)
    m_store, text_store = _train(c, tmp_path / "store", [], loader, vloader)
    assert text_list == text_store
    assert int(m_store.engine().step_t.item()) == 4                                           # two epochs of two steps
    assert torch.equal(m_list.engine().arena.params, m_store.engine().arena.params)
    for (n, p), (_, q) in zip(m_list.named_parameters(), m_store.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
