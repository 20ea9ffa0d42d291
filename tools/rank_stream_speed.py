#!/usr/bin/env python3
"""Times of the streaming effective-rank measurement (r3d_qr_append / r3d_qr_merge, r3d_amd/rankstream.py) on one MI355X.

(a) r3d_qr_append alone: n = 4096 gaussian rows folded into warm accumulators at H in {128, 512, 1024} with 1 and 8 lanes;
    after a warm-up the median of --launches launches, each between its own pair of events; rows/s = n / median.
(b) [9596, 128], the largest matrix both ways admit: the streaming path end to end (update() in chunks of 512 rows with
    8 lanes, the merge, the Jacobi on R and the read-back: StreamingRank.finalize()) against effective_rank(x) on the same
    matrix and GPU; wall clock around a synchronised call, median of --launches runs each, and both results next to the
    float64 value.
(c) a validation pass of the headline model (token fusion, hidden 128, 8 heads): validate() over 200 one-clip batches with
    S = 16, with --erank_report's accumulators attached (reset, three update() launches per forward, three finalize())
    against the plain pass; median of --passes passes each, alternating.
Prints one JSON line and writes it to --out.
    python tools/rank_stream_speed.py [--launches 50] [--passes 7] [--out profiles/rank_stream_speed.json]"""
import argparse, contextlib, io, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

K, Q, HEADS, H0 = 17, 8, 8, 128
PAD = K + 1


def median_event_ms(fn, n, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def median_wall_ms(fn, n, warmup=3):
    out = None
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def append_rates(n_launch, dev):
    from r3d_amd import ops
    from r3d_amd.rankstream import StreamingRank
    res = []
    n = 4096
    for H in (128, 512, 1024):
        x = torch.randn(n, H, generator=torch.Generator().manual_seed(H)).to(dev)
        for lanes in (1, 8):
            acc = StreamingRank(H, dev, lanes=lanes)
            ms = median_event_ms(lambda: acc.update(x), n_launch)
            assert torch.isfinite(acc.R).all()
            T = ops.qr_append_tile_rows(H)
            tiles = -(-(-(-n // lanes)) // T)                       # tiles per lane
            res.append(dict(H=H, lanes=lanes, n=n, tile_rows=T, append_ms=round(ms, 4), rows_per_s=round(n / ms * 1e3),
                            us_per_column_step=round(ms * 1e3 / (tiles * H), 3)))
    return res


def end_to_end(n_launch, dev):
    from r3d_amd.erank import effective_rank
    from r3d_amd.rankstream import StreamingRank
    N, H = 9596, 128
    x = torch.randn(N, H, generator=torch.Generator().manual_seed(1)).to(dev)
    sv = torch.linalg.svdvals(x.double().cpu())
    p = sv / sv.sum()
    ref = float(torch.exp(-(p * p.log()).sum()))
    acc = StreamingRank(H, dev, lanes=8)

    def stream():
        acc.reset()
        for c0 in range(0, N, 512):
            acc.update(x[c0:c0 + 512])
        return acc.finalize()["erank"]

    def append_only():
        acc.reset()
        for c0 in range(0, N, 512):
            acc.update(x[c0:c0 + 512])
    with torch.no_grad():
        ms_s, er_s = median_wall_ms(stream, n_launch)
        ms_a, _ = median_wall_ms(append_only, n_launch)
        ms_j, er_j = median_wall_ms(lambda: float(effective_rank(x)), n_launch)
    return dict(N=N, H=H, chunk=512, lanes=8, streaming_ms=round(ms_s, 3), streaming_appends_only_ms=round(ms_a, 3),
                effective_rank_ms=round(ms_j, 3), erank_fp64=round(ref, 5), erank_streaming=round(er_s, 5),
                erank_effective_rank=round(er_j, 5))


def validation_pass(passes, dev):
    from oracle import synth
    from r3d_amd import rankstream
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    from r3d_amd.train_proposed_depth import validate
    args = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    torch.manual_seed(1)
    model = FUTR(K, H0, PAD, dev, args, n_query=Q, n_head=HEADS, num_encoder_layers=2, num_decoder_layers=1).to(dev).eval()
    eng = model.engine()
    distinct = [[torch.from_numpy(t).to(dev) for t in synth.make_batch(1, 16, K, PAD, 40 + s)] for s in range(8)]
    loader = [distinct[i % 8] for i in range(200)]
    accs = rankstream.attach(model)
    rankstream.detach(model)
    out = {}

    def run(flag):
        with contextlib.redirect_stdout(io.StringIO()):
            if flag:
                for a in accs.values():
                    a.reset()
                eng.rank_stream = [(rankstream.BUFFERS[n], a) for n, a in accs.items()]
            try:
                validate(model, loader, None, PAD, dev)
            finally:
                eng.rank_stream = None
            if flag:
                out["line"] = rankstream.report_line({n: a.finalize() for n, a in accs.items()})
    ts = {False: [], True: []}
    for flag in (False, True):
        run(flag)                                                     # warm-up: workspaces, planner
    for _ in range(passes):
        for flag in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(flag)
            torch.cuda.synchronize()
            ts[flag].append((time.perf_counter() - t0) * 1e3)
    off, on = statistics.median(ts[False]), statistics.median(ts[True])
    return dict(batches=200, B=1, S=16, H=H0, passes=passes, validate_ms=round(off, 2), validate_with_report_ms=round(on, 2),
                added_ms_per_batch=round((on - off) / 200, 4), line=out["line"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"launches": a.launches,
           "timing": "(a) median of per-launch event pairs after a warm-up; (b), (c) median wall clock around synchronised calls"}
    res["append"] = append_rates(a.launches, dev)
    res["end_to_end_9596x128"] = end_to_end(a.launches, dev)
    res["validation_pass"] = validation_pass(a.passes, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
