#!/usr/bin/env python3
"""Timings of the AFFT baseline (model/afft.py) at (B, S) = (8, 16), (16, 256) and (8, 1142), hidden 128, 17 classes, 8
queries, 224 x 224 depth maps; medians over alternating rounds after a warm-up, device events around graph replays.

(a) The training step's tail alone, as a hipGraph each (the step itself is replayed as one):
      chain     -- r3d_afft_head_step: pool, heads, losses, d_actdur, d_pooled, d_fused in one launch (its loss partials are
                   reduced by the AdamW launch of the step, so nothing else belongs to it);
      composed  -- the same arithmetic from the launches that existed before it: avgpool_rows_fwd, head GEMM,
                   losses_fwd_bwd, d_pooled GEMM, avgpool_rows_bwd.
    Also what engine_afft.chain_pays() routes each shape to.
(b) The graphed AFFT training step (train()'s _GraphedSteps, dropout on, the tail as chain_pays() routes it, and with
    the chain forced on and off) next to the graphed plain SA-Fuser step (model/futr_safuser_depth.py, same depth
    resolution) at the same shape.
Prints one JSON line and writes it to --out.
    python tools/afft_step_speed.py [--reps 200] [--steps 30] [--rounds 7] [--out profiles/afft_step_speed.json]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from r3d_amd import ops
from r3d_amd._lib import GEMM_NT, GEMM_NN
from r3d_amd.engine_afft import chain_pays
from r3d_amd.train_proposed_depth import _GraphedSteps

H, K, Q, D, HW = 128, 17, 8, 2048, (224, 224)
SHAPES = [(8, 16), (16, 256), (8, 1142)]
HYPER = (5e-3, (0.9, 0.999), 1e-8)


def build(variant, dev):
    if variant == "afft":
        from r3d_amd.model.afft import FUTR
    else:
        from r3d_amd.model.futr_safuser_depth import FUTR
    args = argparse.Namespace(input_dim=D, seg=variant != "afft", anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    torch.manual_seed(1)
    return FUTR(K, H, K + 1, dev, args, n_query=Q, n_head=8, num_encoder_layers=2, num_decoder_layers=1,
                depth_pixels=HW[0] * HW[1]).to(dev).train()


def make_inputs(B, S, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    pad = K + 1
    feats = torch.randn(B, S, D, generator=g)
    depth = torch.rand(B, S, 1, HW[0], HW[1], generator=g)
    lab = torch.randint(0, K - 1, (B, S), generator=g)
    lab[1::2, S - max(S // 8, 1):] = pad
    tgt = torch.randint(0, K - 1, (B, Q), generator=g)
    dur = torch.rand(B, Q, generator=g) + 0.05
    dur = dur / dur.sum(1, keepdim=True)
    return [t.to(dev) for t in (feats, depth, lab, dur, tgt)]


def graph_of(fn):
    fn()                                  # eager once: planner, workspaces
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def window(replay, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps           # us


def tail_alone(B, S, dev, reps, rounds):
    N, BQ = B * S, B * Q
    g = torch.Generator(device="cpu").manual_seed(5)
    f = lambda *s: torch.randn(*s, generator=g).to(dev)       # noqa: E731
    fused, w_head, b_head = f(N, H), f(K + 1, H) / H ** 0.5, 0.1 * f(K + 1)
    lab, dur, tgt = make_labels(B, S, dev)
    e = lambda *s: torch.empty(*s, device=dev)                # noqa: E731
    pooled, out, d_out, d_pooled, d_fused = e(BQ, H), e(BQ, K + 1), e(BQ, K + 1), e(BQ, H), e(N, H)
    ws = torch.zeros(ops.losses_ws_floats(B, S, Q), device=dev)
    ws2 = torch.zeros(ops.losses_ws_floats(B, S, Q), device=dev)
    loss, counts = torch.zeros(4, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    gws = ops.GemmWorkspace(dev)

    def chain():
        ops.afft_head_step(fused, w_head, b_head, pooled, out, B, S, Q, lab, tgt, dur, K + 1, 47, d_out, d_fused, ws)

    def composed():
        ops.avgpool_rows_fwd(fused, pooled, B, S, Q)
        ops.gemm(GEMM_NT, pooled, w_head, out, bias=b_head, ws=gws)
        ops.losses_fwd_bwd(None, out[:, :K], out[:, K:], K + 1, lab, tgt, dur, B, S, Q, K, K + 1, 47, loss, counts,
                           d_act=d_out[:, :K], d_dur=d_out[:, K:], ld_ddur=K + 1, ws=ws2)
        ops.gemm(GEMM_NN, d_out, w_head, d_pooled, ws=gws)
        ops.avgpool_rows_bwd(d_pooled, d_fused, B, S, Q)
    composed()
    torch.cuda.synchronize()
    ref = d_fused.clone()
    chain()
    torch.cuda.synchronize()
    err = float((d_fused - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
    gc, gm = graph_of(chain), graph_of(composed)
    for _ in range(3):
        window(gc.replay, reps), window(gm.replay, reps)
    tc, tm = [], []
    for _ in range(rounds):
        tc.append(window(gc.replay, reps))
        tm.append(window(gm.replay, reps))
    return dict(chain_us=round(statistics.median(tc), 2), composed_us=round(statistics.median(tm), 2),
                chain_us_min_max=[round(min(tc), 2), round(max(tc), 2)], composed_us_min_max=[round(min(tm), 2), round(max(tm), 2)],
                chain_over_composed=round(statistics.median(tc) / statistics.median(tm), 3),
                d_fused_rel_diff=float(f"{err:.2e}"), routed_to="chain" if chain_pays(B, S, H, Q) else "composed")


def make_labels(B, S, dev):
    d = make_inputs(B, 1, "cpu", 6)
    g = torch.Generator(device="cpu").manual_seed(7)
    lab = torch.randint(0, K - 1, (B, S), generator=g)
    lab[1::2, S - max(S // 8, 1):] = K + 1
    return lab.to(dev), d[3].to(dev), d[4].to(dev)


def stepper(variant, batches, dev, head_chain=None):
    model = build(variant, dev)
    eng = model.engine()
    eng.defer_tail = True
    if variant == "afft":
        eng.use_head_chain = head_chain
    acc_l = torch.zeros(4, dtype=torch.float64, device=dev)
    acc_c = torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _GraphedSteps(eng, acc_l, acc_c, None, K + 1)
    state = dict(i=0)

    def step():
        gs.step(batches[state["i"] % len(batches)], 1e-3, HYPER, True)
        state["i"] += 1
    for _ in range(3 * len(batches) + 4):
        step()
    torch.cuda.synchronize()
    assert torch.isfinite(acc_l).all()
    return step, model


def graphed_steps(B, S, dev, steps, rounds):
    batches = [make_inputs(B, S, dev, seed=s) for s in range(2)]
    runs = {}
    keep = []
    for name, variant, hc in (("afft", "afft", None), ("afft_chain", "afft", True), ("afft_composed", "afft", False),
                              ("plain", "plain", None)):
        try:
            runs[name], m = stepper(variant, batches, dev, hc)
            keep.append(m)
        except Exception as e:      # noqa: BLE001  (a shape a model refuses is a result, not a failure of the tool)
            runs[name] = f"{type(e).__name__}: {e}"
    times = {n: [] for n, r in runs.items() if callable(r)}
    for _ in range(rounds):
        for n in times:
            times[n].append(window(runs[n], steps) / 1e3)     # ms
    res = {n + "_ms_per_step": round(statistics.median(t), 4) for n, t in times.items()}
    res.update({n + "_ms_min_max": [round(min(t), 4), round(max(t), 4)] for n, t in times.items()})
    res.update({n + "_error": r for n, r in runs.items() if not callable(r)})
    if "afft" in times and "plain" in times:
        res["afft_over_plain"] = round(res["afft_ms_per_step"] / res["plain_ms_per_step"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(hidden=H, n_class=K, n_query=Q, depth_hw=list(HW), reps=a.reps, steps=a.steps, rounds=a.rounds, shapes={})
    for B, S in SHAPES:
        r = dict(tail=tail_alone(B, S, dev, a.reps, a.rounds))
        r["step"] = graphed_steps(B, S, dev, a.steps, a.rounds)
        res["shapes"][f"B{B}xS{S}"] = r
        print(f"B{B}xS{S}", json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
