#!/usr/bin/env python3
"""Times of the split-key cross-attention core (r3d_mha_splitk_fwd / _bwd, csrc/attention_splitk.hip) against the tiled core
at Lq 8 (r3d_mha_tiled_*) and, where it runs, the S x S core (r3d_mha_core_*): B 8, 8 heads, Lq 8, dropout mask and key labels
given, operands laid out as the fusion engine has them, at (Lk, head width) = (1142, 16), (1142, 128), (2000, 16).  Forward,
and forward + backward, each replayed from a captured graph; device events around --reps replays, one process, the median
(min, max) of --rounds alternating rounds after a warm-up; no profiler anywhere.
    --alt-lib 64=path,256=path   also time a build of csrc/attention_splitk.hip ALONE (a shared library of that one object,
                                 compiled with -DR3D_SPLITK_CHUNK=n): how the chunk function was chosen.
Then (b) the token-fusion model's graphed training step (dropout on, 17 classes, 224 x 224 depth frames) at the newly admitted
(B, S, hidden) = (8, 1142, 1024) and (8, 2000, 128) with --long_clips, and at (8, 933, 1024) with the flag on and off in
alternating rounds (the same launches: the flag costs nothing where the core fits).  Prints one JSON line, writes it to --out.
    python tools/cross_splitk_speed.py [--rounds 7] [--reps 20] [--step-reps 4] [--skip-steps] [--out profiles/cross_splitk_speed.json]"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

B, HEADS, LQ = 8, 8, 8
PAIR_SHAPES = ((1142, 16), (1142, 128), (2000, 16))            # (Lk, head width)
STEP_NEW = ((8, 1142, 1024), (8, 2000, 128))
STEP_OLD = (8, 933, 1024)
HYPER = (5e-3, (0.9, 0.999), 1e-8)
K, D, HW = 17, 2048, (224, 224)
PAD = K + 1


def _events(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(reps):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def measure(configs, rounds, reps):
    """configs: {name: fn(i)}.  A warm-up pass, then `rounds` passes over all of them in turn; [median, min, max] ms per call."""
    for fn in configs.values():
        _events(fn, max(reps // 4, 3))
    got = {n: [] for n in configs}
    for _ in range(rounds):
        for n, fn in configs.items():
            got[n].append(_events(fn, reps))
    return {n: [round(statistics.median(v), 5), round(min(v), 5), round(max(v), 5)] for n, v in got.items()}


def _graphed(run, keep):
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    fn = lambda i: graph.replay()      # noqa: E731
    fn.keep = keep                     # the graph holds raw addresses: its buffers must outlive it
    return fn


class AltSplitk:
    """The two launches of a library that holds csrc/attention_splitk.hip alone (another R3D_SPLITK_CHUNK), bound from the
    header's prototypes as r3d_amd/_lib.py binds the product's."""

    def __init__(self, path):
        from r3d_amd import _abi, _lib
        self.lib = ctypes.CDLL(path)
        for name, ret, params in _lib._FUNCTIONS:
            if name.startswith("r3d_mha_splitk_"):
                fn = getattr(self.lib, name)
                fn.argtypes = [_abi.ctype_of(t) for t, _ in params]
                fn.restype = _abi.ctype_of(ret)


def pair_configs(Lk, dh, alts, dev):
    from r3d_amd import ops
    H = HEADS * dh
    g = torch.Generator().manual_seed(Lk + dh)
    q, kv, d_o = (torch.randn(r, c, generator=g).to(dev) for r, c in ((B * LQ, H), (B * Lk, 2 * H), (B * LQ, H)))
    keep = (torch.rand(B, HEADS, LQ, Lk, generator=g) > 0.1).to(torch.uint8).to(dev)
    lab = torch.zeros(B, Lk, dtype=torch.int64)
    lab[1::2, Lk - Lk // 4:] = PAD                                      # every other clip: a padded last quarter
    lab = lab.to(dev)
    k, v = kv[:, :H], kv[:, H:]
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)      # noqa: E731
    o, lse, delta, dq, dkv = e(B * LQ, H), e(B, HEADS, LQ), e(B, HEADS, LQ), e(B * LQ, H), e(B * Lk, 2 * H)
    dk, dv = dkv[:, :H], dkv[:, H:]
    kw = dict(key_labels=lab, pad_idx=PAD, drop_mask=keep, drop_scale=1 / 0.9)
    ws = e(max(ops.mha_splitk_ws_floats(B, HEADS, LQ, Lk, dh, t) for t in (False, True)))
    keepalive = (q, kv, d_o, keep, lab, o, lse, delta, dq, dkv, ws)
    args = (B, HEADS, LQ, Lk, dh)

    def splitk(bwd):
        ops.mha_splitk_fwd(q, k, v, o, lse, ws, *args, **kw)
        if bwd:
            ops.mha_splitk_bwd(q, k, v, o, lse, d_o, delta, dq, dk, dv, ws, *args, **kw)

    def tiled(bwd):
        ops.mha_tiled_fwd(q, k, v, o, lse, *args, **kw)
        if bwd:
            ops.mha_tiled_bwd(q, k, v, o, lse, d_o, delta, dq, dk, dv, *args, **kw)
    cfg = {}
    for name, fn in (("splitk", splitk), ("tiled", tiled)):
        cfg[f"{name}_fwd"] = _graphed(lambda fn=fn: fn(False), keepalive)
        cfg[f"{name}_fwd_bwd"] = _graphed(lambda fn=fn: fn(True), keepalive)
    if ops.mha_core_supported(LQ, Lk, dh, True):
        probs = e(B, HEADS, LQ, Lk)

        def core(bwd):
            ops.mha_core_fwd(q, k, v, probs, o, *args, **kw)
            if bwd:
                ops.mha_core_bwd(q, k, v, probs, d_o, dq, dk, dv, *args, drop_mask=keep, drop_scale=1 / 0.9)
        cfg["core_fwd"] = _graphed(lambda: core(False), keepalive + (probs,))
        cfg["core_fwd_bwd"] = _graphed(lambda: core(True), keepalive + (probs,))
    for chunk, alt in alts.items():
        n = -(-Lk // chunk)
        assert alt.lib.r3d_mha_splitk_chunk(Lk, dh) == chunk
        wsa = e(B * HEADS * n * LQ * (dh + 2))
        p, ld, st = ops._p, ops._ld, ops._stream

        def alt_pair(bwd, alt=alt, wsa=wsa):
            head = (p(q), ld(q), p(k), ld(k), p(v), ld(v), None, p(lab), PAD, p(keep), 1 / 0.9)
            rc = alt.lib.r3d_mha_splitk_fwd(*head, p(o), ld(o), p(lse), p(wsa), *args, st())
            if bwd and rc == 0:
                rc = alt.lib.r3d_mha_splitk_bwd(*head, p(o), ld(o), p(lse), p(d_o), ld(d_o), p(delta), p(dq), ld(dq), p(dk), ld(dk),
                                                p(dv), ld(dv), p(wsa), *args, st())
            assert rc == 0, rc
        cfg[f"splitk_chunk{chunk}_fwd"] = _graphed(lambda f=alt_pair: f(False), keepalive + (wsa,))
        cfg[f"splitk_chunk{chunk}_fwd_bwd"] = _graphed(lambda f=alt_pair: f(True), keepalive + (wsa,))
    return cfg, (o, dq, dkv)


def step_config(Bc, S, H, long_clips, dev, want_route):
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    from r3d_amd.train_proposed_depth import _GraphedSteps
    from oracle import synth
    args = argparse.Namespace(input_dim=D, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript",
                              long_clips=long_clips)
    torch.manual_seed(1)
    model = FUTR(K, H, PAD, dev, args, n_query=LQ, n_head=HEADS, num_encoder_layers=2, num_decoder_layers=1).to(dev).train()
    eng = model.engine()
    batches = []
    for s in range(2):                 # labels / targets as the suite's batches; the large depth frames drawn on the device
        b = [torch.from_numpy(x).to(dev) for x in synth.make_batch(Bc, S, K, PAD, 7 + s, depth_hw=(1, 1), pad_tail=True)]
        b[1] = torch.rand(Bc, S, 1, HW[0], HW[1], device=dev, generator=torch.Generator(device=dev).manual_seed(s))
        batches.append(b)
    acc_l, acc_c = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _GraphedSteps(eng, acc_l, acc_c, None, PAD)
    fn = lambda i: gs.step(batches[i % 2], 1e-3, HYPER, True)      # noqa: E731

    def check():
        assert eng.last["w"].route == want_route, eng.last["w"].route
        assert torch.isfinite(acc_l).all() and torch.isfinite(eng.arena.params[:eng.arena.n_live]).all()
    fn.check = check
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--alt-lib", default="")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from r3d_amd import ops
    alts = {int(s.split("=")[0]): AltSplitk(s.split("=")[1]) for s in a.alt_lib.split(",") if s}
    res = {"B": B, "heads": HEADS, "Lq": LQ, "rounds": a.rounds, "reps": a.reps, "step_reps": a.step_reps,
           "timing": "device events around `reps` graph replays; [median, min, max] ms per call over `rounds` alternating rounds "
                     "after a warm-up; dropout mask and key labels given",
           "pair": [], "steps": {}}
    for Lk, dh in PAIR_SHAPES:
        cfg, outs = pair_configs(Lk, dh, alts, dev)
        row = dict(Lk=Lk, dh=dh, chunk=ops.mha_splitk_chunk(Lk, dh), ms=measure(cfg, a.rounds, a.reps))
        assert all(bool(torch.isfinite(t).all()) for t in outs)
        # the rule's condition: the split-key pair beats the tiled pair at Lq 8 by more than the rounds' spread
        row["splitk_beats_tiled"] = {k: row["ms"][f"splitk_{k}"][2] < row["ms"][f"tiled_{k}"][1] for k in ("fwd", "fwd_bwd")}
        res["pair"].append(row)
        del cfg
        torch.cuda.empty_cache()
    if not a.skip_steps:
        for Bc, S, H in STEP_NEW:
            fn = step_config(Bc, S, H, True, dev, "splitk")
            res["steps"][f"B{Bc}_S{S}_H{H}_long_clips"] = measure({"step": fn}, a.rounds, a.step_reps)["step"]
            fn.check()
            del fn
            torch.cuda.empty_cache()
        Bc, S, H = STEP_OLD
        on, off = step_config(Bc, S, H, True, dev, "core"), step_config(Bc, S, H, False, dev, "core")
        got = measure({"flag_on": on, "flag_off": off}, a.rounds, a.step_reps)
        on.check(), off.check()
        res["steps"][f"B{Bc}_S{S}_H{H}"] = got
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
