#!/usr/bin/env python3
"""Timings of the three-modality (RGB + depth + gaze) model (model/futr_safuser_tokenfusion3.py, engine_m3.py) at (B, S, H) =
(8, 16, 128), (16, 16, 1024) -- BASELINE configs[4]'s per-GPU shape -- and (8, 1142, 128); 17 classes, 8 queries, 8 heads,
224 x 224 depth maps, gaze_dim 2.  One process, device events, medians of alternating rounds after a warm-up.

(a) seam_vs_composed   the embedding seam alone, forward and forward + backward, each form replayed as a hipGraph:
      seam      -- r3d_embed_fuse3_fwd / r3d_embed_fuse3_bwd + the finalize launch of their LayerNorm partials;
      composed  -- the same arithmetic from the launches that existed before: layernorm_fwd x 2, the gaze product,
                   r3d_token_exchange3_fwd, layernorm_fwd; backward: layernorm_bwd, r3d_token_exchange3_bwd, the ReLU gate,
                   layernorm_bwd x 2.
    engine_m3.seam_pays follows forward + backward, shape by shape (tests/test_m3_cpu.py holds it to this file).
(b) step_vs_cmfuser3   the graphed training step (dropout on, routed by seam_pays) against the same model run through the
    CMFuser3 autograd module with eager torch around it and torch.optim.AdamW -- what exists without this engine.  A yardstick
    for the whole feature, NOT a kernel-for-kernel comparison.  It alternates with the engine's windows round by round, with
    max(3, steps // 4) steps per window (it is not graphed: its windows are host-bound at the short shapes).
(c) step_vs_two_modality   the graphed step next to the two-modality token-fusion step on its composed route (chains forced
    off so that like meets like) at the same shape.  The three-modality step does 1.5 x the fuser rows plus one seam input;
    the ratio is recorded, it is not a pass / fail bar.
(d) penalty   the graphed step at (16, 16, 1024) with erank_weight 0.05 (the "SVD-bound stress"): the step with and without
    the penalty, and the blocked Jacobi launch alone on the step's fused tokens.
Prints one JSON line and writes it to --out.
    python tools/m3_step_speed.py [--reps 200] [--steps 20] [--rounds 7] [--out profiles/m3_step_speed.json]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from r3d_amd import ops
from r3d_amd._lib import GEMM_NT
from r3d_amd.engine_m3 import seam_pays
from r3d_amd.train_proposed_depth import _GraphedSteps

K, Q, D, HW, G, HEADS = 17, 8, 2048, (224, 224), 2, 8
SHAPES = [(8, 16, 128), (16, 16, 1024), (8, 1142, 128)]
HYPER = (5e-3, (0.9, 0.999), 1e-8)
DSC = 1.0 / 0.9


def build(kind, H, dev):
    args = argparse.Namespace(input_dim=D, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    kw = dict(n_query=Q, n_head=HEADS, num_encoder_layers=1, num_decoder_layers=1, depth_pixels=HW[0] * HW[1])
    torch.manual_seed(1)
    if kind == "m3":
        from r3d_amd.model.futr_safuser_tokenfusion3 import FUTR
        return FUTR(K, H, K + 1, dev, args, gaze_dim=G, **kw).to(dev).train()
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    return FUTR(K, H, K + 1, dev, args, **kw).to(dev).train()


def make_inputs(B, S, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    pad = K + 1
    feats = torch.randn(B, S, D, generator=g)
    depth = torch.rand(B, S, 1, HW[0], HW[1], generator=g) - 0.5
    lab = torch.randint(0, K - 1, (B, S), generator=g)
    lab[1::2, S - max(S // 8, 1):] = pad
    tgt = torch.randint(0, K - 1, (B, Q), generator=g)
    dur = torch.rand(B, Q, generator=g) + 0.05
    dur = dur / dur.sum(1, keepdim=True)
    gaze = torch.rand(B, S, G, generator=g) * 2 - 1
    return [t.to(dev) for t in (feats, depth, lab, dur, tgt, gaze)]


def graph_of(fn):
    fn()                                  # eager once: planner, workspaces, function attributes
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


def alternate(fns, reps, rounds):
    for _ in range(3):
        for f in fns.values():
            window(f, reps)
    t = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            t[n].append(window(f, reps))
    return t


# ---- (a) the seam alone -------------------------------------------------------------------------------------------------
def seam_alone(B, S, H, dev, reps, rounds):
    N, R = B * S, 3 * B * S
    g = torch.Generator(device="cpu").manual_seed(5)
    f = lambda *s: torch.randn(*s, generator=g).to(dev)       # noqa: E731
    e = lambda *s: torch.empty(*s, device=dev)                # noqa: E731
    rgb, dep_pre0, gaze = torch.relu(f(N, H)), f(N, H), (torch.rand(N, G, generator=g) * 2 - 1).to(dev)
    w_g, b_g = f(H, G), 0.1 * f(H)
    gam = [1 + 0.1 * f(H) for _ in range(3)]
    bet = [0.1 * f(H) for _ in range(3)]
    mask = torch.zeros(3, H)
    for m in range(3):
        mask[m, torch.randperm(H, generator=g)[:H // 4]] = 1
    mask = mask.to(dev)
    keep = (torch.rand(R, H, generator=g) >= 0.1).to(torch.uint8).to(dev)
    d_h1, add1, add2 = f(R, H), f(R, H), f(R, H)
    o = {k: e(N, H) for k in ("dep_pre", "dep", "gz_pre", "gz", "d_rgb", "d_rgb_pre", "d_dep", "d_dep_pre", "d_gz", "d_gz_pre")}
    st = {k: e(N) for k in ("mean_d", "rstd_d", "mean_g", "rstd_g")}
    x0, h1, m1, r1, d_x0 = e(R, H), e(R, H), e(R), e(R), e(R, H)
    part = {k: e(2 * N * H) for k in ("n1", "dep", "gz")}
    dg = {k: e(2, H) for k in ("n1", "dep", "gz")}
    fin = ops.LnFinalizeGroup([(part[k], -N, H, dg[k][0], dg[k][1]) for k in ("n1", "dep", "gz")])
    ws = ops.GemmWorkspace(dev)

    def seam_fwd():
        ops.embed_fuse3_fwd(rgb, 0, None, dep_pre0, 1, None, gam[0], bet[0], gaze, w_g, b_g, gam[1], bet[1], mask, keep, DSC,
                            gam[2], bet[2], rgb, o["dep_pre"], st["mean_d"], st["rstd_d"], o["dep"], o["gz_pre"], st["mean_g"],
                            st["rstd_g"], o["gz"], x0, h1, m1, r1)

    def seam_bwd():
        ops.embed_fuse3_bwd(d_h1, x0, m1, r1, gam[2], add1, add2, keep, DSC, mask, rgb, o["dep_pre"], st["mean_d"], st["rstd_d"],
                            gam[0], bet[0], o["gz_pre"], st["mean_g"], st["rstd_g"], gam[1], bet[1], o["d_rgb_pre"],
                            o["d_dep_pre"], o["d_gz_pre"], part["n1"], part["dep"], part["gz"])
        fin.launch()

    def comp_fwd():
        ops.layernorm_fwd(dep_pre0, gam[0], bet[0], o["dep"], st["mean_d"], st["rstd_d"], relu=True)
        ops.gemm(GEMM_NT, gaze, w_g, o["gz_pre"], bias=b_g, ws=ws)
        ops.layernorm_fwd(o["gz_pre"], gam[1], bet[1], o["gz"], st["mean_g"], st["rstd_g"], relu=True)
        ops.token_exchange3_fwd(rgb, o["dep"], o["gz"], mask, x0, drop_mask=keep, drop_scale=DSC)
        ops.layernorm_fwd(x0, gam[2], bet[2], h1, m1, r1)

    def comp_bwd():
        ops.layernorm_bwd(d_h1, x0, m1, r1, gam[2], bet[2], d_x0, dg["n1"][0], dg["n1"][1], add1=add1, add2=add2, ws=ws)
        ops.token_exchange3_bwd(d_x0, mask, o["d_rgb"], o["d_dep"], o["d_gz"], drop_mask=keep, drop_scale=DSC)
        ops.posenc_bwd(o["d_rgb"], o["d_rgb_pre"], gate=rgb)
        ops.layernorm_bwd(o["d_dep"], dep_pre0, st["mean_d"], st["rstd_d"], gam[0], bet[0], o["d_dep_pre"], dg["dep"][0],
                          dg["dep"][1], relu=True, ws=ws)
        ops.layernorm_bwd(o["d_gz"], o["gz_pre"], st["mean_g"], st["rstd_g"], gam[1], bet[1], o["d_gz_pre"], dg["gz"][0],
                          dg["gz"][1], relu=True, ws=ws)
    comp_fwd(), comp_bwd()
    torch.cuda.synchronize()
    ref = (h1.clone(), o["d_dep_pre"].clone(), o["d_gz_pre"].clone(), o["d_rgb_pre"].clone())
    seam_fwd(), seam_bwd()
    torch.cuda.synchronize()
    got = (h1, o["d_dep_pre"], o["d_gz_pre"], o["d_rgb_pre"])
    err = max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) for a, b in zip(got, ref))
    graphs = dict(seam_fwd=graph_of(seam_fwd), composed_fwd=graph_of(comp_fwd),
                  seam_fwd_bwd=graph_of(lambda: (seam_fwd(), seam_bwd())), composed_fwd_bwd=graph_of(lambda: (comp_fwd(), comp_bwd())))
    t = alternate({n: g_.replay for n, g_ in graphs.items()}, reps, rounds)
    res = dict(B=B, S=S, H=H, rel_diff_seam_vs_composed=float(f"{err:.2e}"), routed_to="seam" if seam_pays(N, H) else "composed")
    for n, v in t.items():
        res[n + "_us"] = round(statistics.median(v), 2)
        res[n + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    res["seam_over_composed_fwd_bwd"] = round(res["seam_fwd_bwd_us"] / res["composed_fwd_bwd_us"], 3)
    return res


# ---- (b), (c), (d): whole steps ---------------------------------------------------------------------------------------------
def stepper(kind, H, batches, dev, use_seam=None, erank_weight=0.0):
    model = build(kind, H, dev)
    eng = model.engine()
    if kind == "m3":
        eng.use_seam = use_seam
    else:
        eng.defer_tail = True
        eng.use_fuser_chain = eng.use_decoder_chain = False       # the composed route: like meets like
    eng.erank_weight = erank_weight
    acc_l = torch.zeros(4, dtype=torch.float64, device=dev)
    acc_c = torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _GraphedSteps(eng, acc_l, acc_c, None, K + 1)
    n = 6 if kind == "m3" else 5
    state = dict(i=0)

    def step():
        gs.step(batches[state["i"] % len(batches)][:n], 1e-3, HYPER, True)
        state["i"] += 1
    for _ in range(3 * len(batches) + 2):
        step()
    torch.cuda.synchronize()
    assert torch.isfinite(acc_l).all()
    return step, model


def eager_cmfuser3(H, batches, dev):
    """The three-modality model as it can be run WITHOUT engine_m3: torch ops for the embeddings, decoder, heads and losses
    (oracle.futr_oracle's text on the device, float32, autograd), cmfuser3.CMFuser3 for the fuser, torch.optim.AdamW."""
    from oracle import futr_oracle as O
    from r3d_amd.model.cmfuser3 import CMFuser3
    model = build("m3", H, dev)
    p = {n: v.detach().clone().requires_grad_(n.startswith(O.LIVE_PREFIXES + ("gaze_",))) for n, v in model.named_parameters()}
    fuser = CMFuser3(H, num_heads=HEADS).to(dev).train()
    with torch.no_grad():
        for n, v in fuser.named_parameters():
            v.copy_(p["fuser." + n])
    live = [v for v in p.values() if v.requires_grad] + [v for n, v in fuser.named_parameters()
                                                        if ("fuser." + n).startswith(O.LIVE_PREFIXES)]
    opt = torch.optim.AdamW(live, lr=1e-3, weight_decay=HYPER[0])
    state = dict(i=0)

    def step():
        feats, depth, lab, dur, tgt, gaze = batches[state["i"] % len(batches)]
        state["i"] += 1
        B, S = lab.shape
        rgb = F.relu(F.linear(feats, p["input_embed.weight"], p["input_embed.bias"]))
        d = F.linear(depth.reshape(B, S, -1), p["depth_projection.weight"], p["depth_projection.bias"])
        d = F.relu(O.layer_norm(d, p["depth_layernorm.weight"], p["depth_layernorm.bias"]))
        gz = F.relu(O.layer_norm(F.linear(gaze, p["gaze_projection.weight"], p["gaze_projection.bias"]),
                                 p["gaze_layernorm.weight"], p["gaze_layernorm.bias"]))
        fused = fuser({"rgb": rgb, "depth": d, "gaze": gz}, "train")
        tgt_ = O.decoder(p, fused, p["pos_embedding"][:, :S], p["query_embed.weight"].unsqueeze(0), lab == K + 1, HEADS, 1)
        out = {"action": F.linear(tgt_, p["fc.weight"], p["fc.bias"]),
               "duration": F.linear(tgt_, p["fc_len.weight"], p["fc_len.bias"]).squeeze(2),
               "seg": F.linear(fused, p["fc_seg.weight"], p["fc_seg.bias"])}
        gold = lab.reshape(-1).clone()
        gold[(gold == K + 1) | (gold == O.EXCLUDE_CLASS_IDX)] = -1
        l_seg = F.cross_entropy(out["seg"].reshape(-1, K), gold, ignore_index=-1, reduction="none").mean()
        tg = tgt.reshape(-1).clone()
        tg[(tg == K + 1) | (tg == O.EXCLUDE_CLASS_IDX)] = -1
        l_act = F.cross_entropy(out["action"].reshape(-1, K), tg, ignore_index=-1, reduction="none").mean()
        dm = (dur != K + 1).float()
        od = F.normalize(torch.exp(out["duration"]) * dm, p=1, dim=-1)
        l_dur = torch.sum((od - dur * dm) ** 2) / dm.sum()
        opt.zero_grad(set_to_none=True)
        (l_seg + l_act + l_dur).backward()
        opt.step()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    return step


def whole_steps(B, S, H, dev, steps, rounds):
    batches = [make_inputs(B, S, dev, seed=s) for s in range(2)]
    runs, keep = {}, []
    for name, mk in (("m3", lambda: stepper("m3", H, batches, dev)), ("m3_seam", lambda: stepper("m3", H, batches, dev, True)),
                     ("m3_composed", lambda: stepper("m3", H, batches, dev, False)),
                     ("two_modality_composed", lambda: stepper("m2", H, batches, dev))):
        try:
            runs[name], m = mk()
            keep.append(m)
        except Exception as e:      # noqa: BLE001  (a shape a model refuses is a result, not a failure of the tool)
            runs[name] = f"{type(e).__name__}: {e}"
    try:                                # the eager yardstick takes its turn in every round, with fewer steps per window
        runs["eager_cmfuser3"] = eager_cmfuser3(H, batches, dev)
    except Exception as e:              # noqa: BLE001
        runs["eager_cmfuser3"] = f"{type(e).__name__}: {e}"
    times = {n: [] for n, r in runs.items() if callable(r)}
    for _ in range(rounds):
        for n in times:
            k = max(3, steps // 4) if n == "eager_cmfuser3" else steps
            times[n].append(window(runs[n], k) / 1e3)         # ms
    res = {n + "_ms_per_step": round(statistics.median(t), 4) for n, t in times.items()}
    res.update({n + "_ms_min_max": [round(min(t), 4), round(max(t), 4)] for n, t in times.items()})
    res.update({n + "_error": r for n, r in runs.items() if not callable(r)})
    if "m3" in times and "two_modality_composed" in times:
        res["m3_over_two_modality"] = round(res["m3_ms_per_step"] / res["two_modality_composed_ms_per_step"], 4)
    if "m3" in times and "eager_cmfuser3" in times:
        res["eager_cmfuser3_over_m3"] = round(res["eager_cmfuser3_ms_per_step"] / res["m3_ms_per_step"], 2)
    return res


def penalty(B, S, H, dev, steps, rounds):
    batches = [make_inputs(B, S, dev, seed=s) for s in range(2)]
    plain, m0 = stepper("m3", H, batches, dev)
    pen, m1 = stepper("m3", H, batches, dev, erank_weight=0.05)
    t = alternate(dict(plain=plain, penalised=pen), steps, rounds)
    eng = m1.engine()
    w = eng.last["w"]
    res = dict(B=B, S=S, H=H, erank_weight=0.05, step_ms=round(statistics.median(t["plain"]) / 1e3, 4),
               penalised_step_ms=round(statistics.median(t["penalised"]) / 1e3, 4), erank=round(float(eng.erank_value()), 3),
               sweeps=float(w.er_stats[0, 3]), blocked=w.er_blk is not None, transposed=bool(getattr(w, "er_flip", False)))
    if w.er_blk is not None:
        gj = graph_of(lambda: ops.erank_blocked_into(w.fused, w.er_blk, transposed=w.er_flip))
        tj = [window(gj.replay, 20) for _ in range(rounds)]
        res["blocked_jacobi_us"] = round(statistics.median(tj), 1)
        res["blocked_jacobi_share_of_step"] = round(res["blocked_jacobi_us"] / 1e3 / res["penalised_step_ms"], 3)
    res["penalty_share_of_step"] = round(1 - res["step_ms"] / res["penalised_step_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(n_class=K, n_query=Q, heads=HEADS, depth_hw=list(HW), gaze_dim=G, reps=a.reps, steps=a.steps, rounds=a.rounds,
               seam_vs_composed=[], steps_by_shape={})
    for B, S, H in SHAPES:
        r = seam_alone(B, S, H, dev, a.reps, a.rounds)
        res["seam_vs_composed"].append(r)
        print("seam", json.dumps(r), flush=True)
    for B, S, H in SHAPES:
        r = whole_steps(B, S, H, dev, a.steps, a.rounds)
        res["steps_by_shape"][f"B{B}xS{S}xH{H}"] = r
        print(f"B{B}xS{S}xH{H}", json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    res["penalty"] = penalty(16, 16, 1024, dev, a.steps, a.rounds)
    print("penalty", json.dumps(res["penalty"]), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
