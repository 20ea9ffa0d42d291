#!/usr/bin/env python3
"""Timings of the clip store's layouts (r3d_amd/clipcache.py).  One process, device events, medians of alternating rounds after
a warm-up; every round's extremes are kept.

(a) collate   the collate launch alone at (B, S) = (8, 16), (16, 256), (8, 1142) with D 2048, 224 x 224 depth and gaze_dim 2,
    for LAYOUT_DEPTH, layout_query and LAYOUT_GAZE.  The store holds enough clips (at least 400 MB of frames) that consecutive
    batches read frames the 256 MiB Infinity Cache does not hold; the launches of several shuffled batches are captured in one
    hipGraph (no host gaps) and the graph's replays are timed.  For LAYOUT_DEPTH the tracks entry (r3d_clip_collate_tracks)
    alternates with the five-tensor entry (r3d_clip_collate) of the same library, round by round.
    verdict: the tracks entry "is not slower" at a shape when its median exceeds the old entry's by no more than half the
    larger of the two entries' own round-to-round ranges (max - min).  clipcache.DEPTH_LAYOUT_ENTRY moves to the tracks entry
    only if that holds at all three shapes.
(b) epochs    train() of the L3, TCN and three-modality loops at (8, 16) fed by a DeviceClipLoader of the matching layout,
    against the same batches as pinned host tensors through InputPrefetcher (every batch crosses PCIe under the previous step).
    Each loader runs one epoch as a warm-up (allocations, planning, graph capture) and one timed epoch, its validation batch and
    checkpoint included.  Recorded, not a bar.
Prints one JSON line and writes it to --out.
    python tools/clip_tracks_speed.py [--rounds 7] [--epoch-steps 1600] [--skip-epochs] [--out profiles/clip_tracks_speed.json]"""
import argparse, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from r3d_amd import clipcache
from r3d_amd.clipcache import LAYOUT_DEPTH, LAYOUT_GAZE, ClipStore, DeviceClipLoader, layout_query

K, Q, D, HW, G = 17, 8, 2048, (224, 224), 2
PAD, QPAD = K + 1, 47
SHAPES = ((8, 16), (16, 256), (8, 1142))
LAUNCHES = {16: 64, 256: 8, 1142: 4}            # launches per timed graph: a window of a few milliseconds at every shape
MIN_POOL_BYTES = 400 << 20


class _Clips:
    """n items of one layout whose frame tracks all view ONE host array per track (the timing does not read the values; the
    store still uploads every item's rows, so the pools have n distinct clips' worth of rows)."""

    def __init__(self, layout, n, S, seed):
        rng = np.random.default_rng(seed)
        shapes = {"features": (S, D), "depth_features": (S, 1) + HW, "gaze": (S, G)}
        self.n, self.layout = n, layout
        self.frames = {t.name: rng.random(shapes[t.name], dtype=np.float32) for t in layout.frames}
        self.words = {"past_label": rng.integers(0, K - 1, S), "trans_future_dur": rng.random(Q).astype(np.float32),
                      "trans_future_target": rng.integers(0, K - 1, Q), "query_label": rng.integers(0, QPAD, S)}

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return [self.frames[t.name] if t.kind == "frames" else self.words[t.name] for t in self.layout]


def _window(replay, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps           # us


def collate_times(layout, B, S, dev, rounds):
    clip_bytes = 4 * S * sum({"features": D, "depth_features": HW[0] * HW[1], "gaze": G}[t.name] for t in layout.frames)
    n_batches = max(2, -(-MIN_POOL_BYTES // (B * clip_bytes)))
    store = ClipStore.from_dataset(_Clips(layout, B * n_batches, S, seed=S), PAD, dev, layout=layout)
    idx = list(DeviceClipLoader(store, B, shuffle=True, generator=torch.Generator().manual_seed(0)).index_batches())
    n = LAUNCHES[S]
    items = [torch.tensor(idx[i % len(idx)], dtype=torch.int64, device=dev) for i in range(n)]
    sizes = store.sizes(idx[0])
    out = store.empty_batch(B, sizes)
    entries = ["r3d_clip_collate_tracks"] + (["r3d_clip_collate"] if layout is LAYOUT_DEPTH else [])
    graphs, ref = {}, None
    for e in entries:
        for t in out:
            t.fill_(-1)
        store.launch(items[0], sizes, out, entry=e)
        torch.cuda.synchronize()
        if ref is None:
            ref = [t.clone() for t in out]
        same = all(torch.equal(a, b) for a, b in zip(out, ref))
        assert same, f"{e} differs from {entries[0]} at B {B}, S {S}"
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for it in items:
                store.launch(it, sizes, out, entry=e)
        graphs[e] = g
    reps = 5
    for _ in range(3):
        for g in graphs.values():
            _window(g.replay, reps)
    t = {e: [] for e in graphs}
    for _ in range(rounds):
        for e, g in graphs.items():
            t[e].append(_window(g.replay, reps) / n)
    moved = 2 * B * clip_bytes                         # the frames, read once and written once (tables and labels left out)
    res = dict(B=B, S=S, clips=len(store), store_MB=round(store.nbytes / 1e6, 1), launches_per_graph=n,
               read_write_MB=round(moved / 1e6, 2))
    for e, v in t.items():
        med = statistics.median(v)
        res[e] = dict(us=round(med, 3), us_min_max=[round(min(v), 3), round(max(v), 3)], TB_per_s=round(moved / med / 1e6, 3))
    if len(t) == 2:
        new, old = t["r3d_clip_collate_tracks"], t["r3d_clip_collate"]
        spread = max(max(new) - min(new), max(old) - min(old)) / 2
        res["tracks_over_old"] = round(statistics.median(new) / statistics.median(old), 4)
        res["tracks_not_slower"] = bool(statistics.median(new) - statistics.median(old) <= spread)
    del store, out, ref
    torch.cuda.empty_cache()
    return res


# ---- (b) epochs ---------------------------------------------------------------------------------------------------------
class _NoSched:
    def step(self):
        pass


def _loop(kind, dev):
    """(layout, make_batch(seed) -> host tensors in the layout's order, run(train_loader, val_loader, out_dir))"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from r3d_amd.optim import FlatAdamW
    B, S = 8, 16
    if kind == "l3":
        import l3_step_speed as L
        from r3d_amd import train_unsupervised as TU
        from r3d_amd.model.futr_unsupervised_temp3 import FUTR
        torch.manual_seed(1)
        model = FUTR(K, L.H, PAD, dev, L._model_args(), n_query=Q, n_head=L.HEADS, num_encoder_layers=2, num_decoder_layers=1,
                     query_num=L.C).to(dev)
        opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)
        args = argparse.Namespace(epochs=1, seg=True, anticipate=True, task="long", input_type="i3d_transcript", graph_steps=True)

        def run(tl, vl, d):
            TU.train(args, model, tl, opt, _NoSched(), torch.nn.MSELoss(reduction="none"), d, PAD, dev, vl, 1)
        return layout_query(QPAD), (lambda seed: [t.cpu() for t in L.make_batch(B, S, "cpu", seed)]), run
    if kind == "tcn":
        import l3_step_speed as L
        from r3d_amd import train_tcn as TT
        from r3d_amd.model.tcn import MustafaNet1DTCN
        torch.manual_seed(1)
        model = MustafaNet1DTCN(num_classes=K, anticipated_frames=Q).to(dev).train()
        opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)
        args = argparse.Namespace(epochs=1, graph_steps=True)

        def run(tl, vl, d):
            TT.train(args, model, tl, vl, opt, _NoSched(), None, d, PAD, dev)
        return layout_query(19), (lambda seed: [t.cpu() for t in L.make_batch(B, S, "cpu", seed)]), run
    import m3_step_speed as M
    from r3d_amd.opts import parser
    from r3d_amd.train_proposed_depth import train
    model = M.build("m3", 128, dev)
    opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)
    o = parser.parse_args([])
    args = argparse.Namespace(epochs=1, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=8,
                              graph_steps=True, erank_report=o.erank_report, erank_weight=o.erank_weight, erank_route=o.erank_route,
                              erank_every=0, restore_train_mode=False, supcon_weight=0.0, pixel_shard=False)

    def run(tl, vl, d):
        train(args, model, tl, opt, _NoSched(), None, d, PAD, dev, vl, seed=1)
    return LAYOUT_GAZE, (lambda seed: [t.cpu() for t in M.make_inputs(B, S, "cpu", seed)]), run


def epoch_times(kind, dev, steps):
    from r3d_amd.utils import InputPrefetcher
    layout, make, run = _loop(kind, dev)
    nb = 16
    host = [make(s) for s in range(nb)]
    B = host[0][0].shape[0]
    items = [[t[c].numpy() for t in b] for b in host for c in range(B)]
    store = ClipStore.from_dataset(items, PAD, dev, layout=layout)
    per = max(1, steps // nb)
    order = [j for _ in range(per) for j in range(len(items))]
    long_at = tuple(i for i, t in enumerate(layout) if t.dtype == torch.int64)
    pinned = [[t.pin_memory() for t in b] for b in host]
    loaders = {"device_clip_loader": (DeviceClipLoader(store, B, sampler=order), DeviceClipLoader(store, B, sampler=list(range(B)))),
               "input_prefetcher_pinned_host": (InputPrefetcher(pinned * per, dev, long_at=long_at), [pinned[0]])}
    res = dict(B=B, S=int(host[0][0].shape[1]), steps=per * nb, layout=layout.name, store_MB=round(store.nbytes / 1e6, 1))
    with tempfile.TemporaryDirectory() as d:
        for name, (tl, vl) in loaders.items():
            run(tl, vl, d)                                      # warm-up epoch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(tl, vl, d)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[name] = dict(us_per_step=round(dt / (per * nb) * 1e6, 1), clips_per_s=round(B * per * nb / dt))
    res["device_over_host_clips_per_s"] = round(res["device_clip_loader"]["clips_per_s"] /
                                                res["input_prefetcher_pinned_host"]["clips_per_s"], 3)
    del store
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--epoch-steps", type=int, default=1600)
    ap.add_argument("--skip-epochs", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(D=D, depth_hw=list(HW), gaze_dim=G, rounds=a.rounds, depth_layout_entry=clipcache.DEPTH_LAYOUT_ENTRY, collate={})
    for name, layout in (("depth", LAYOUT_DEPTH), ("query", layout_query(QPAD)), ("gaze", LAYOUT_GAZE)):
        res["collate"][name] = []
        for B, S in SHAPES:
            r = collate_times(layout, B, S, dev, a.rounds)
            res["collate"][name].append(r)
            print(name, json.dumps(r), flush=True)
    res["tracks_entry_not_slower_at_all_shapes"] = all(r["tracks_not_slower"] for r in res["collate"]["depth"])
    if not a.skip_epochs:
        res["epochs"] = {}
        for kind in ("l3", "tcn", "m3"):
            import contextlib, io
            with contextlib.redirect_stdout(io.StringIO()):
                r = epoch_times(kind, dev, a.epoch_steps)
            res["epochs"][kind] = r
            print(kind, json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
