#!/usr/bin/env python3
"""ms per call of the temporal auxiliary losses (csrc/temporal.hip): run detection, and the forward and forward + backward of
the cluster, contrastive and focal losses, at (B, T, C) = (8, 16, 48), (8, 512, 48), (8, 1142, 48), (8, 1142, 128) with run
lengths drawn from 5 .. 60 frames, and (8, 200, 48) with every frame its own run -- as the median of --launches event pairs
after a warm-up.  The focal loss runs on the same B T rows of C logits.

The yardstick is the loop form of the same losses in float32 torch ops on the same GPU (tests/temporal_oracle.py: loop_*): one
small torch call per run or pair of runs, and run detection by a host loop that reads one label per frame -- what a user of
the reference runs today.  Its calls take up to seconds, so each of its medians is over as many calls as fit into --ref-seconds
(at least 3, at most --launches; the number is recorded).
Prints one JSON line and writes it to --out.
    python tools/temporal_loss_speed.py [--launches 100] [--ref-seconds 6] [--out profiles/temporal_loss_speed.json]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tests import temporal_oracle as TO

SHAPES = ((8, 16, 48, "5-60"), (8, 512, 48, "5-60"), (8, 1142, 48, "5-60"), (8, 1142, 128, "5-60"), (8, 200, 48, "singletons"))
TAU = 0.07


def make_labels(B, T, kind, g):
    lab = torch.empty(B, T, dtype=torch.int64)
    for b in range(B):
        t, v = 0, 0
        while t < T:
            n = 1 if kind == "singletons" else int(torch.randint(5, 61, (1,), generator=g))
            lab[b, t:t + n] = v % 47
            t, v = t + n, v + 1 + int(torch.randint(0, 3, (1,), generator=g))
    return lab


def median_ms(fn, launches, warm=10, seconds=None):
    """median of event-pair times; with `seconds` as many calls as fit (at least 3, at most launches).  Returns (ms, calls)."""
    t_start = time.time()
    for i in range(warm):
        fn()
        if seconds is not None and time.time() - t_start > seconds / 2:
            break
    torch.cuda.synchronize()
    ts, t_start = [], time.time()
    for i in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1))
        if seconds is not None and len(ts) >= 3 and time.time() - t_start > seconds:
            break
    return round(statistics.median(ts), 4), len(ts)


def host_ms(fn, reps):
    """wall-clock median of a call that synchronises by itself"""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(ts), 4)


def shape(B, T, C, kind, launches, ref_seconds, dev):
    from r3d_amd import ops
    from r3d_amd.loss import temporal as TL
    g = torch.Generator().manual_seed(B * T + C)
    lab = make_labels(B, T, kind, g).to(dev)
    x = torch.randn(B * T, C, generator=g).to(dev)
    gold = lab.reshape(-1) % C
    out = dict(B=B, T=T, C=C, runs=kind)
    # run detection
    out["label_runs_ms"], _ = median_ms(lambda: TL.label_runs(lab), launches)
    out["host_loop_intervals_ms"] = host_ms(lambda: TO.loop_intervals(lab), 3)
    r = TL.label_runs(lab)
    iv = r.intervals()
    assert iv == TO.intervals(lab)
    out["runs_per_clip"] = round(sum(len(c) for c in iv) / B, 1)
    loss, dx = torch.empty(1, device=dev), torch.empty(B * T, C, device=dev)
    x3 = x.view(B, T, C)
    xt = x3.clone().requires_grad_(True)

    def pair(tag, fwd, bwd, ref):
        def fwd_bwd():
            fwd()
            bwd()

        def ref_fwd_bwd():
            xt.grad = None
            ref(xt).backward()
        out[f"{tag}_hip_fwd_ms"], _ = median_ms(fwd, launches)
        out[f"{tag}_hip_fwd_bwd_ms"], _ = median_ms(fwd_bwd, launches)
        out[f"{tag}_loop_fwd_ms"], out[f"{tag}_loop_fwd_calls"] = median_ms(lambda: ref(xt.detach()), launches, warm=2,
                                                                             seconds=ref_seconds)
        out[f"{tag}_loop_fwd_bwd_ms"], out[f"{tag}_loop_fwd_bwd_calls"] = median_ms(ref_fwd_bwd, launches, warm=2,
                                                                                     seconds=ref_seconds)
        out[f"{tag}_loop_over_hip_fwd"] = round(out[f"{tag}_loop_fwd_ms"] / out[f"{tag}_hip_fwd_ms"], 2)
        out[f"{tag}_loop_over_hip_fwd_bwd"] = round(out[f"{tag}_loop_fwd_bwd_ms"] / out[f"{tag}_hip_fwd_bwd_ms"], 2)
        fwd_bwd()
        ref_fwd_bwd()
        torch.cuda.synchronize()
        out[f"{tag}_loss_hip"], out[f"{tag}_loss_loop"] = round(float(loss), 6), round(float(ref(xt.detach())), 6)
        out[f"{tag}_grad_max_abs_diff_over_max_abs"] = float((dx.view(B, T, C) - xt.grad).abs().max() / xt.grad.abs().max())

    ws_c = torch.empty(ops.tcluster_ws_floats(B, T, C), device=dev)
    pair("cluster", lambda: ops.tcluster_fwd(x, B, T, r.starts, r.last, r.count, ws_c, loss),
         lambda: ops.tcluster_bwd(x, B, T, r.starts, r.last, r.count, ws_c, dx), lambda t: TO.loop_cluster(t, iv))
    ws_n = torch.empty(ops.tcontrast_ws_floats(B, T), device=dev)
    pair("contrast", lambda: ops.tcontrast_fwd(x, B, T, r.first, r.last, ws_n, loss, temperature=TAU),
         lambda: ops.tcontrast_bwd(x, B, T, r.first, r.last, ws_n, dx, temperature=TAU),
         lambda t: TO.loop_contrastive(t, iv, TAU))
    ws_f, flags, counts = torch.empty(B * T, device=dev), torch.empty(B * T, dtype=torch.bool, device=dev), \
        torch.empty(2, dtype=torch.int64, device=dev)
    pad = C - 1
    pair("focal", lambda: ops.focal_rows(x, gold, pad, ws=ws_f, loss_out=loss, flags=flags, counts=counts),
         lambda: ops.focal_rows(x, gold, pad, d_pred=dx), lambda t: TO.loop_focal(t.reshape(B * T, C), gold, pad)[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--ref-seconds", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_loss_speed.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(tool="temporal_loss_speed", launches=a.launches, ref_seconds=a.ref_seconds, temperature=TAU,
               device=torch.cuda.get_device_name(0), shapes=[])
    for B, T, C, kind in SHAPES:
        res["shapes"].append(shape(B, T, C, kind, a.launches, a.ref_seconds, dev))
        print(json.dumps(res["shapes"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
