"""ClipStore's host-only plan (r3d_amd/clipcache.py), without a GPU: pool rows against NpyClipReader's row semantics,
deduplication by (file, row), a numpy collate over the plan against the reference's np.load -> slice -> torch.tensor ->
pad_sequence (basedataset_darai_depth.py:110-130,174-206), DeviceClipLoader's batch order against DataLoader's samplers,
and the capacity check."""
import numpy as np
import pytest
import torch
from torch.utils.data import BatchSampler, DistributedSampler, RandomSampler

from r3d_amd.clipcache import ClipStore, DeviceClipLoader, plan_dataset, plan_specs
from r3d_amd.utils import NpyClipReader

PAD = 11


def _write(tmp_path, D=16, hw=(6, 8)):
    """Two videos (features + a longer per-recording depth file) and a depth file shorter than its feature file."""
    rng = np.random.default_rng(3)
    paths = {}
    for name, T, Td in (("v0", 30, 60), ("v1", 22, 22), ("short", 30, 18)):
        f = rng.standard_normal((T, D)).astype(np.float32)
        d = rng.random((Td, 1) + hw).astype(np.float32)
        fp, dp = tmp_path / f"{name}.npy", tmp_path / f"{name}_1.npy"
        np.save(fp, f)
        np.save(dp, d)
        paths[name] = (str(fp), str(dp))
    return paths


def _specs(paths):
    v0, v1, sh = paths["v0"], paths["v1"], paths["short"]
    clips = [(*v0, 0, 6, 1, 25, 56),       # depth trim
             (*v0, 0, 12, 1, 25, 56),      # same sequence, longer observation: shares the first rows
             (*v0, 0, 20, 3, 25),          # step 3 on the same files
             (*sh, 10, 26, 2),             # depth file ends before the slice
             (*v1, 4, 4, 1),               # empty clip
             (*v1, 2, 17, 3),
             (*sh, 20, 26, 1)]             # features but no depth rows at all
    rng = np.random.default_rng(8)
    labels = []
    for i in range(len(clips)):
        n, q = (i * 5) % 9, 4 + i % 3
        labels.append((rng.integers(0, 10, n), rng.random(q).astype(np.float64), rng.integers(0, 10, q).astype(np.float64)))
    return clips, labels


def _reference_item(c, lab):
    f, d = np.load(c[0]), np.load(c[1])
    if len(c) > 5:
        d = d[c[5]:(c[6] if len(c) > 6 else None)]
    return [torch.tensor(f[c[2]:c[3]][::c[4]], dtype=torch.float32), torch.tensor(d[c[2]:c[3]][::c[4]], dtype=torch.float32),
            torch.tensor(lab[0], dtype=torch.long), torch.tensor(lab[1], dtype=torch.float32),
            torch.tensor(lab[2], dtype=torch.long)]


def _reference_collate(items):
    pad = torch.nn.utils.rnn.pad_sequence
    return [pad([it[k] for it in items], batch_first=True, padding_value=v) for k, v in enumerate((0, 0, PAD, PAD, PAD))]


def _host_pools(plan):
    pools = []
    for segs, shape in ((plan.rgb_src, plan.D), (plan.dep_src, plan.P)):
        rows = [(np.load(s)[r] if isinstance(s, str) else s).reshape(-1, shape) for s, r in segs]
        pools.append(np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, shape), np.float32))
    return pools


def _host_collate(plan, idx):
    """What r3d_clip_collate computes, restated in numpy over the host plan."""
    rgb, dep = _host_pools(plan)
    S_f, S_d, S_l, S_q = plan.sizes(idx)
    B = len(idx)
    out = [np.zeros((B, S_f, plan.D), np.float32), np.zeros((B, S_d, plan.P), np.float32), np.full((B, S_l), PAD, np.int64),
           np.full((B, S_q), PAD, np.float32), np.full((B, S_q), PAD, np.int64)]
    for b, i in enumerate(idx):
        for o, pool, off, ids in ((out[0], rgb, plan.off_f, plan.ids_f), (out[1], dep, plan.off_d, plan.ids_d)):
            r = ids[off[i]:off[i + 1]]
            o[b, :len(r)] = pool[r]
        lab = plan.lab[plan.off_l[i]:plan.off_l[i + 1]]
        out[2][b, :len(lab)] = lab
        q0, q1 = plan.off_q[i], plan.off_q[i + 1]
        out[3][b, :q1 - q0] = plan.q_dur[q0:q1]
        out[4][b, :q1 - q0] = plan.q_tgt[q0:q1]
    out[0] = out[0].reshape((B, S_f) + plan.feat_shape)
    out[1] = out[1].reshape((B, S_d) + plan.frame_shape)
    return [torch.from_numpy(x) for x in out]


def test_plan_rows_follow_npy_clip_reader(tmp_path):
    clips, labels = _specs(_write(tmp_path))
    plan = plan_specs(clips, labels, PAD)
    for seg_list, off, ids, col in ((plan.rgb_src, plan.off_f, plan.ids_f, 0), (plan.dep_src, plan.off_d, plan.ids_d, 1)):
        pool = [(s, int(r)) for s, rows in seg_list for r in rows]            # pool row -> (file, file row)
        for i, c in enumerate(clips):
            n = np.load(c[col], mmap_mode="r").shape[0]
            want = NpyClipReader._rows(n, c[2], c[3], c[4], *(c[5:7] if col else ()))
            got = [pool[p] for p in ids[off[i]:off[i + 1]]]
            assert [r for _, r in got] == list(want)
            assert all(np.load(s, mmap_mode="r").shape[0] == n and s.endswith(c[col].split("/")[-1]) for s, _ in got)
    assert plan.len_f[4] == 0 and plan.len_d[4] == 0                          # the empty clip
    assert plan.len_f[3] == 8 and plan.len_d[3] == 4                          # short depth file: fewer depth rows


def test_pool_rows_are_deduplicated(tmp_path):
    clips, labels = _specs(_write(tmp_path))
    plan = plan_specs(clips + clips[:2], labels + labels[:2], PAD)             # repeated items add no rows
    want_f, want_d = set(), set()
    for c in clips:
        nf, nd = (np.load(p, mmap_mode="r").shape[0] for p in c[:2])
        want_f |= {(c[0], r) for r in NpyClipReader._rows(nf, c[2], c[3], c[4])}
        want_d |= {(c[1], r) for r in NpyClipReader._rows(nd, c[2], c[3], c[4], *c[5:7])}
    assert plan.F_rgb == len(want_f) and plan.F_dep == len(want_d)
    assert plan.F_rgb < int(plan.len_f.sum()) and plan.F_dep < int(plan.len_d.sum())
    assert plan.nbytes >= 4 * (plan.F_rgb * plan.D + plan.F_dep * plan.P)


def test_host_collate_equals_reference_collate(tmp_path):
    clips, labels = _specs(_write(tmp_path))
    plan = plan_specs(clips, labels, PAD)
    for idx in ([0, 1, 2, 3, 4, 5, 6], [3, 3, 1], [4], [2, 5, 0, 4], [6, 4]):
        want = _reference_collate([_reference_item(clips[i], labels[i]) for i in idx])
        got = _host_collate(plan, idx)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)
    # from_dataset's plan over the reference items themselves (dicts and 5-lists) gives the same batches
    items = [_reference_item(c, lab) for c, lab in zip(clips, labels)]
    dicts = [dict(zip(("features", "depth_features", "past_label", "trans_future_dur", "trans_future_target"), it))
             for it in items]
    for ds in (dicts, items):
        dplan = plan_dataset(ds, PAD)
        assert dplan.F_rgb == int(dplan.len_f.sum())                          # (not deduplicated)
        for idx in ([0, 1, 2, 3, 4, 5], [5, 4]):
            want = _reference_collate([items[i] for i in idx])
            for g, w in zip(_host_collate(dplan, idx), want):
                assert g.dtype == w.dtype and torch.equal(g, w)


def test_batch_order_matches_dataloader_samplers(tmp_path):
    clips, labels = _specs(_write(tmp_path))
    plan = plan_specs((clips * 4)[:24], (labels * 4)[:24], PAD)
    n = len(plan)
    for B, drop in ((5, False), (5, True), (8, False)):
        got = list(DeviceClipLoader(plan, B, shuffle=True, generator=torch.Generator().manual_seed(7),
                                    drop_last=drop).index_batches())
        want = list(BatchSampler(RandomSampler(range(n), generator=torch.Generator().manual_seed(7)), B, drop))
        assert got == want
        ld = DeviceClipLoader(plan, B, drop_last=drop)
        assert len(ld) == (n // B if drop else -(-n // B)) == len(list(ld.index_batches()))
        assert list(ld.index_batches()) == list(BatchSampler(range(n), B, drop))
    for rank in (0, 1):
        ld = DeviceClipLoader(plan, 4, sampler=DistributedSampler(plan, num_replicas=2, rank=rank, seed=3))
        ref = DistributedSampler(range(n), num_replicas=2, rank=rank, seed=3)
        for epoch in (0, 1, 2):
            ld.set_epoch(epoch)
            ref.set_epoch(epoch)
            assert list(ld.index_batches()) == list(BatchSampler(ref, 4, False))
        assert len(ld) == 3
    with pytest.raises(ValueError):
        DeviceClipLoader(plan, 4, shuffle=True, sampler=range(n))


def test_budget_below_plan_raises_without_a_device(tmp_path, monkeypatch):
    clips, labels = _specs(_write(tmp_path))
    need = plan_specs(clips, labels, PAD).nbytes

    def no_device(*a, **k):
        raise AssertionError("the capacity check touched the device")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    with pytest.raises(ValueError) as e:
        ClipStore.from_specs(clips, labels, PAD, "cuda", budget=need - 1)
    assert str(need) in str(e.value) and str(need - 1) in str(e.value)
    items = [_reference_item(c, lab) for c, lab in zip(clips, labels)]
    need_ds = plan_dataset(items, PAD).nbytes
    with pytest.raises(ValueError) as e:
        ClipStore.from_dataset(items, PAD, "cuda", budget=need_ds // 2)
    assert str(need_ds) in str(e.value) and str(need_ds // 2) in str(e.value)
