#!/usr/bin/env python3
"""ms/step of the plain SA-Fuser model's graphed training step (model/futr_safuser_depth.py) next to the token-fusion
model's, in one process, at the headline shape (bench.CFG: 8 clips x 16 frames, hidden 128) and at the SAME depth
resolution for both: 224 x 224 (the token-fusion default, like for like) and 160 x 120 (the plain module's default).
Each runs train()'s graphed step (r3d_amd.train_proposed_depth._GraphedSteps, one step per graph) over 4 alternating
batches, timed with events around --steps replays after a warm-up; token fusion is timed before and after the plain
model at each resolution.  It also lists the library entry points one (eager) step of each model enqueues, in order.
Prints one JSON line and writes it to --out.
    python tools/plain_step_speed.py [--steps 200] [--out profiles/plain_step_speed.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import CFG
from r3d_amd import ops
from r3d_amd.train_proposed_depth import _GraphedSteps

HYPER = (5e-3, (0.9, 0.999), 1e-8)


def build(variant, hw, dev):
    if variant == "plain":
        from r3d_amd.model.futr_safuser_depth import FUTR
    else:
        from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    c = CFG
    args = argparse.Namespace(input_dim=c["D"], seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    torch.manual_seed(1)
    return FUTR(c["K"], c["H"], c["K"] + 1, dev, args, n_query=c["Q"], n_head=c["heads"], num_encoder_layers=c["n_enc"],
                num_decoder_layers=c["n_dec"], depth_pixels=hw[0] * hw[1]).to(dev).train()


def make_inputs(hw, dev, seed):
    c = CFG
    g = torch.Generator(device="cpu").manual_seed(seed)
    pad = c["K"] + 1
    feats = torch.randn(c["B"], c["S"], c["D"], generator=g)
    depth = torch.rand(c["B"], c["S"], 1, hw[0], hw[1], generator=g)
    lab = torch.randint(0, c["K"] - 1, (c["B"], c["S"]), generator=g)
    lab[1::2, c["S"] - max(c["S"] // 8, 1):] = pad
    tgt = torch.randint(0, c["K"] - 1, (c["B"], c["Q"]), generator=g)
    dur = torch.rand(c["B"], c["Q"], generator=g) + 0.05
    dur = dur / dur.sum(1, keepdim=True)
    return [t.to(dev) for t in (feats, depth, lab, dur, tgt)]


def launches(gs, batch):
    """The library entry points one eager step enqueues (every kernel launch of r3d_amd.ops goes through ops.check)."""
    names, real = [], ops.check
    ops.check = lambda r, name, *a, **k: (names.append(name), real(r, name, *a, **k))[1]
    try:
        gs.eng._drop_ready = None
        gs._enqueue(batch, 1e-3, HYPER, True)
        torch.cuda.synchronize()
    finally:
        ops.check = real
    return names


def time_variant(variant, hw, batches, steps, dev):
    model = build(variant, hw, dev)
    eng = model.engine()
    eng.defer_tail = True
    acc_l = torch.zeros(4, dtype=torch.float64, device=dev)
    acc_c = torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _GraphedSteps(eng, acc_l, acc_c, None, CFG["K"] + 1)
    names = launches(gs, batches[0])
    for i in range(20):
        gs.step(batches[i % len(batches)], 1e-3, HYPER, True)
    torch.cuda.synchronize()
    w = eng.last["w"]
    chains = sorted(str(k) for k in w.tables if k[0] in ("fwd_chain", "bwd_chain", "dec_chain"))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        gs.step(batches[i % len(batches)], 1e-3, HYPER, True)
    t1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(acc_l).all()
    return t0.elapsed_time(t1) / steps, chains, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"shape": dict(B=CFG["B"], S=CFG["S"], H=CFG["H"], K=CFG["K"]), "steps": a.steps}
    for hw in ((224, 224), (120, 160)):
        batches = [make_inputs(hw, dev, seed=s) for s in range(4)]
        tag = f"{hw[0]}x{hw[1]}"
        r = {}
        for v in ("tokenfusion", "plain", "tokenfusion"):
            ms, chains, names = time_variant(v, hw, batches, a.steps, dev)
            r.setdefault(v + "_ms_per_step", []).append(round(ms, 4))
            r[v + "_chains"] = chains
            r[v + "_launches"] = names
        r["plain_over_tokenfusion"] = round(r["plain_ms_per_step"][0] / min(r["tokenfusion_ms_per_step"]), 4)
        res[tag] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
