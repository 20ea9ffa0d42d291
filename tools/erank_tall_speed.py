#!/usr/bin/env python3
"""Times of the tall rank route (r3d_amd.erank.ErankTall, csrc/qr_fold_wy.hip) on one MI355X, one process, device events,
alternating rounds, medians over the rounds.

(a) the fold: R.zero_() + r3d_qr_fold_wy ("wy") against R.zero_() + r3d_qr_append ("column") at the same lanes (ErankTall's
    default for the blocked fold), at (n, H) in {(9600, 128), (18272, 128), (4096, 256), (4096, 512)}; the column fold at
    its own default lanes and the merge tree are timed next to them.  erank.fold_pays is written from "fold_pays".
(b) the penalty alone, forward + backward through pre-allocated buffers: ErankTall (default fold) against the Jacobi route
    (the blocked kernel + ErankBackward, what the engine enqueues) at (320, 128), (2048, 128), (9136, 128).
(c) train()'s graphed training step (token fusion, hidden 128, 8 heads, dropout on) at (B, S) = (8, 1142) without the
    penalty, with it on the Jacobi route and on the tall route; at (8, 1200) and (16, 1142) without it and on the tall route.
Prints one JSON line and writes it to --out.
    python tools/erank_tall_speed.py [--rounds 7] [--launches 10] [--steps 30] [--parts abc] [--out profiles/erank_tall_speed.json]"""
import argparse, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

K, Q, HEADS, H0 = 17, 8, 8, 128
PAD = K + 1
HYPER = (5e-3, (0.9, 0.999), 1e-8)
LAM = 0.05


def alternate(variants, rounds, launches, warmup=3):
    """variants: {name: fn}.  Per round and variant one event pair around `launches` calls; returns {name: median ms per call}."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / launches)
    return {k: statistics.median(v) for k, v in ts.items()}


def part_fold(rounds, launches, dev):
    from r3d_amd import ops
    res = []
    for n, H in ((9600, 128), (18272, 128), (4096, 256), (4096, 512)):
        x = torch.randn(n, H, generator=torch.Generator().manual_seed(n + H)).to(dev)
        lanes = min(64, -(-n // ops.qr_fold_wy_tile_rows(H)))
        lanes_c = min(64, -(-n // ops.qr_append_tile_rows(H)))
        R = torch.zeros(lanes, H, H, device=dev)
        Rc = torch.zeros(lanes_c, H, H, device=dev)

        def wy():
            R.zero_()
            ops.qr_fold_wy(x, R)

        def column():
            R.zero_()
            ops.qr_append(x, R)

        def column_own():
            Rc.zero_()
            ops.qr_append(x, Rc)

        def merge():
            ops.qr_merge(R)
        t = alternate({"wy": wy, "column": column, "column_own": column_own, "merge": merge}, rounds, launches)
        res.append(dict(n=n, H=H, lanes=lanes, wy_tile_rows=ops.qr_fold_wy_tile_rows(H), wy_ms=round(t["wy"], 4),
                        column_ms=round(t["column"], 4), column_own_lanes=lanes_c, column_own_lanes_ms=round(t["column_own"], 4),
                        merge_ms=round(t["merge"], 4), wy_rows_per_s=round(n / t["wy"] * 1e3),
                        fold_pays="wy" if t["wy"] < t["column"] else "column"))
    return res


def part_penalty(rounds, launches, dev):
    from r3d_amd import ops
    from r3d_amd.erank import ErankBackward, ErankTall
    res = []
    for N, H in ((320, 128), (2048, 128), (9136, 128)):
        x = torch.randn(N, H, generator=torch.Generator().manual_seed(N)).to(dev)
        gout = torch.ones(1, device=dev)
        ws = ops.GemmWorkspace(dev)
        tall = ErankTall(N, H, dev)
        blk = ops.ErankBlockedBufs(N, H, dev, max_sweeps=16)
        bwd = ErankBackward(N, H, False, dev, ld=blk.Rp)
        dx = torch.empty_like(x)

        def f_tall():
            tall.forward(x)
            tall.backward(x, gout, dx, False, ws)

        def f_jacobi():
            ops.erank_blocked_into(x, blk)
            bwd.run(x, blk.af_t, blk.sigma, blk.stats, gout, dx, False, ws)
        t = alternate({"tall": f_tall, "jacobi": f_jacobi}, rounds, launches)
        torch.cuda.synchronize()
        res.append(dict(N=N, H=H, tall_fold=tall.fold, tall_lanes=tall.lanes, tall_ms=round(t["tall"], 4),
                        jacobi_ms=round(t["jacobi"], 4), erank_tall=round(float(tall.stats[0, 0]), 4),
                        erank_jacobi=round(float(blk.stats[0]), 4)))
    return res


def make_inputs(B, S, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    feats = (torch.rand(B, S, 2048, device=dev, generator=g) * 2 - 1) * math.sqrt(3.0)
    depth = torch.rand(B, S, 1, 224, 224, device=dev, generator=g)
    lab = torch.randint(0, K - 1, (B, S), device=dev, generator=g)
    lab[1::2, S - max(S // 8, 1):] = PAD
    tgt = torch.randint(0, K - 1, (B, Q), device=dev, generator=g)
    dur = torch.rand(B, Q, device=dev, generator=g) + 0.05
    dur = dur / dur.sum(1, keepdim=True)
    return [feats, depth, lab, dur, tgt]


def part_step(rounds, steps, dev):
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    from r3d_amd.train_proposed_depth import _GraphedSteps
    args = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    res = []
    for B, S, routes in ((8, 1142, ("none", "jacobi", "tall")), (8, 1200, ("none", "tall")), (16, 1142, ("none", "tall"))):
        batch = make_inputs(B, S, dev, seed=B + S)
        runs = {}
        for route in routes:
            torch.manual_seed(1)
            model = FUTR(K, H0, PAD, dev, args, n_query=Q, n_head=HEADS, num_encoder_layers=2, num_decoder_layers=1).to(dev).train()
            eng = model.engine()
            eng.defer_tail = True
            eng.erank_weight = 0.0 if route == "none" else LAM
            eng.erank_route = "jacobi" if route == "none" else route
            gs = _GraphedSteps(eng, torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev),
                               None, PAD)
            runs[route] = (lambda gs=gs: gs.step(batch, 1e-3, HYPER, True))
        t = alternate(runs, rounds, steps, warmup=5)
        res.append(dict(B=B, S=S, H=H0, **{f"{k}_ms_per_step": round(v, 4) for k, v in t.items()}))
        del runs, batch
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"rounds": a.rounds, "launches": a.launches, "steps": a.steps,
           "timing": "per variant one device-event pair around `launches` calls (`steps` graph replays) per round, variants "
                     "alternating inside every round, median over the rounds, one process"}
    if "a" in a.parts:
        res["fold"] = part_fold(a.rounds, a.launches, dev)
    if "b" in a.parts:
        res["penalty"] = part_penalty(a.rounds, a.launches, dev)
    if "c" in a.parts:
        res["step"] = part_step(a.rounds, a.steps, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
