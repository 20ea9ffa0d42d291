"""The device-resident clip store on the GPU: r3d_clip_collate against the reference's collate (bitwise) over ragged,
trimmed, short, empty and step-3 clips, repeated items and several row lengths (16-byte and dword paths, rows of one and
of many 16-KiB chunks); the ABI's argument checks; capture into a hipGraph; DeviceClipLoader's look-ahead; and train()
fed by DeviceClipLoader against train() on the same batches as a plain list."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from r3d_amd import _lib  # noqa: E402
from r3d_amd.clipcache import ClipStore, DeviceClipLoader  # noqa: E402
from tests.test_clip_cache_cpu import PAD, _reference_collate, _reference_item, _specs, _write  # noqa: E402

BATCHES = ([0, 1, 2, 3, 4, 5, 6], [3, 3, 1], [5], [2, 5, 0, 4], [6, 4], [6])


def _equal(got, want):
    assert len(got) == len(want) == 5
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), k


@pytest.mark.parametrize("D,hw", [(2048, (224, 224)), (2048, (120, 160)), (37, (7, 9)), (37, (67, 71)), (2048, (7, 9)),
                                  (37, (224, 224))])
def test_collate_equals_reference_collate(tmp_path, D, hw):
    clips, labels = _specs(_write(tmp_path, D=D, hw=hw))
    for make in ("specs", "dataset"):
        if make == "specs":
            store = ClipStore.from_specs(clips, labels, PAD, "cuda")
        else:
            store = ClipStore.from_dataset([_reference_item(c, lab) for c, lab in zip(clips, labels)], PAD, "cuda")
        for idx in BATCHES:
            want = _reference_collate([_reference_item(clips[i], labels[i]) for i in idx])
            got = store.collate(idx)
            torch.cuda.synchronize()
            _equal(got, want)
        f, d, lab, dur, tgt = store.collate([6, 4])              # no depth rows in the batch: S_d = 0, no error
        torch.cuda.synchronize()
        assert d.shape == (2, 0, 1) + hw and f.shape[1] == 6
        assert store.collate([])[0].shape == (0, 0, D)           # B = 0


def test_collate_abi_rejects_bad_arguments(tmp_path):
    lib = _lib.load()
    clips, labels = _specs(_write(tmp_path))
    store = ClipStore.from_specs(clips, labels, PAD, "cuda")
    idx = [0, 3]
    sizes = store.sizes(idx)
    items = torch.tensor(idx, dtype=torch.int64, device="cuda")
    out = store.empty_batch(2, sizes)

    def job(**kw):
        p, t = store.plan, store.t
        j = _lib.ClipCollateJob(rgb_pool=store.rgb_pool.data_ptr(), F_rgb=p.F_rgb, D=p.D, depth_pool=store.depth_pool.data_ptr(),
                                F_dep=p.F_dep, P=p.P, n_items=len(p), items=items.data_ptr(), B=2, S_f=sizes[0], S_d=sizes[1],
                                S_l=sizes[2], S_q=sizes[3], pad_idx=PAD, features=out[0].data_ptr(), depth=out[1].data_ptr(),
                                past_label=out[2].data_ptr(), trans_future_dur=out[3].data_ptr(),
                                trans_future_target=out[4].data_ptr(), **{k: v.data_ptr() for k, v in t.items()})
        for k, v in kw.items():
            setattr(j, k, v)
        return lib.r3d_clip_collate(C.byref(j), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert job() == 0
    torch.cuda.synchronize()
    _equal(out, _reference_collate([_reference_item(clips[i], labels[i]) for i in idx]))
    assert job(B=-1) == -1                                       # R3D_EINVAL
    assert job(rgb_pool=None) == -1                              # a null pool with rows
    assert job(depth_pool=None) == -1
    assert job(S_d=-3) == -1 and job(D=-1) == -1 and job(n_items=-1) == -1
    assert job(items=None) == -1 and job(features=None) == -1 and job(lab=None) == -1
    assert lib.r3d_clip_collate(None, None) == -1
    assert job(B=0) == 0 and job(S_f=0, S_d=0, S_l=0, S_q=0) == 0   # zero extents: legal, nothing enqueued
    torch.cuda.synchronize()


def test_collate_captured_in_a_graph_replays_the_eager_result(tmp_path):
    clips, labels = _specs(_write(tmp_path, D=64, hw=(120, 160)))
    store = ClipStore.from_specs(clips, labels, PAD, "cuda")
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
        _equal(out, _reference_collate([_reference_item(clips[i], labels[i]) for i in order]))


def test_look_ahead_never_overwrites_a_held_batch(tmp_path):
    clips, labels = _specs(_write(tmp_path, D=2048, hw=(224, 224)))
    store = ClipStore.from_specs(clips * 3, labels * 3, PAD, "cuda")
    loader = DeviceClipLoader(store, 3)
    want = [_reference_collate([_reference_item((clips * 3)[i], (labels * 3)[i]) for i in b]) for b in loader.index_batches()]
    it = iter(loader)
    held = next(it)                                              # batch t
    b1 = next(it)                                                # t + 1 (t + 2 is being collated meanwhile)
    del b1                                                       # its blocks go back to the allocator
    b2 = next(it)
    torch.cuda.synchronize()
    _equal(held, want[0])
    _equal(b2, want[2])
    rest = list(it)
    torch.cuda.synchronize()
    for got, w in zip(rest, want[3:]):
        _equal(got, w)
    _equal(held, want[0])


def test_device_clip_loader_trains_identically(tmp_path):
    """train() with hipGraph steps fed by DeviceClipLoader over ClipStore.from_specs of the batches written as per-clip
    `.npy` files (with frames before and after each clip), and a DeviceClipLoader as val_loader, ends with the same
    parameters (bitwise) as train() on the batches handed over as a plain list."""
    from r3d_amd.train_proposed_depth import train
    from r3d_amd.optim import FlatAdamW
    from tests.helpers import load_fixture, fixture_batch
    from tests.test_engine_gpu import build_model
    fx = load_fixture("train_loop")
    m = fx["meta"]
    batches = [[t for t in fixture_batch(fx, seed=500 + i)] for i in range(3)]
    val = [[t[:1] for t in fixture_batch(fx, seed=300)]]

    def store_of(bs, tag):
        clips, labels = [], []
        for i, b in enumerate(bs):
            for c in range(b[0].shape[0]):
                S, pre, post = b[0].shape[1], 3 + c, 2
                arrs = []
                for t in b[:2]:
                    arrs.append(np.concatenate([np.full((pre,) + tuple(t.shape[2:]), 7.0, np.float32), t[c].numpy(),
                                                np.full((post,) + tuple(t.shape[2:]), 9.0, np.float32)]))
                fp, dp = tmp_path / f"{tag}{i}c{c}.npy", tmp_path / f"{tag}{i}c{c}_1.npy"
                np.save(fp, arrs[0])
                np.save(dp, arrs[1])
                clips.append((str(fp), str(dp), pre, pre + S, 1))
                labels.append((b[2][c].numpy(), b[3][c].numpy(), b[4][c].numpy()))
        return ClipStore.from_specs(clips, labels, m["pad_idx"], "cuda")
    loader = DeviceClipLoader(store_of(batches, "t"), batches[0][0].shape[0])
    vloader = DeviceClipLoader(store_of(val, "v"), 1)
    assert len(loader) == 3 and len(vloader) == 1
    for got, b in zip(loader, batches):
        torch.cuda.synchronize()
        _equal(got, b)
    finals = []
    for cached in (False, True):
        model = build_model(fx)
        args = argparse.Namespace(epochs=1, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=1,
                                  graph_steps=True)
        opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)

        class NoSched:
            def step(self):
                pass
        model.eval()
        train(args, model, loader if cached else batches, opt, NoSched(), None, str(tmp_path), m["pad_idx"],
              torch.device("cuda"), vloader if cached else val, seed=1)
        torch.cuda.synchronize()
        finals.append(model.engine().arena.params.clone())
    assert torch.equal(finals[0], finals[1])
