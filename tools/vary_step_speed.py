#!/usr/bin/env python3
"""ms/step of the activation-magnitude fuser variant's graphed training step (model/futr_safuser_tokenfusion_vary.py)
next to the token-fusion model's, in one process, at the headline shape (bench.CFG: 8 clips x 16 frames, hidden 128).
Both run train()'s graphed step (r3d_amd.train_proposed_depth._GraphedSteps) over 4 alternating batches, timed with
events around 200 replays after a warm-up; prints one JSON line, and also writes it to the path given by --out.
    python tools/vary_step_speed.py [--steps 200] [--out profiles/vary_step_speed.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import CFG, make_inputs
from r3d_amd.train_proposed_depth import _GraphedSteps


def build(variant, dev):
    if variant == "vary":
        from r3d_amd.model.futr_safuser_tokenfusion_vary import FUTR
    else:
        from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    c = CFG
    args = argparse.Namespace(input_dim=c["D"], seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    torch.manual_seed(1)
    return FUTR(c["K"], c["H"], c["K"] + 1, dev, args, n_query=c["Q"], n_head=c["heads"], num_encoder_layers=c["n_enc"],
                num_decoder_layers=c["n_dec"], depth_pixels=c["P"]).to(dev).train()


def time_variant(variant, batches, steps, dev):
    model = build(variant, dev)
    eng = model.engine()
    eng.defer_tail = True
    acc_l = torch.zeros(4, dtype=torch.float64, device=dev)
    acc_c = torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _GraphedSteps(eng, acc_l, acc_c, None, CFG["K"] + 1)
    hyper = (5e-3, (0.9, 0.999), 1e-8)
    for i in range(20):
        gs.step(batches[i % len(batches)], 1e-3, hyper, True)
    torch.cuda.synchronize()
    w = eng.last["w"]
    chains = sorted(str(k) for k in w.tables if k[0] in ("fwd_chain", "bwd_chain", "dec_chain"))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        gs.step(batches[i % len(batches)], 1e-3, hyper, True)
    t1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(acc_l).all()
    return t0.elapsed_time(t1) / steps, chains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    batches = [make_inputs(CFG, dev, seed=s) for s in range(4)]
    res = {"shape": dict(B=CFG["B"], S=CFG["S"], H=CFG["H"], K=CFG["K"]), "steps": a.steps}
    for v in ("tokenfusion", "vary", "tokenfusion"):          # (token fusion timed before and after)
        ms, chains = time_variant(v, batches, a.steps, dev)
        res.setdefault(v + "_ms_per_step", []).append(round(ms, 4))
        res[v + "_chains"] = chains
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
