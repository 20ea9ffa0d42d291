#!/usr/bin/env python3
"""What the supervised contrastive loss's wide route (csrc/supcon.hip, 257 <= D <= 2048; ops wide=True) costs, in one process,
with device events, as medians of --rounds alternating rounds after a warm-up (tools/rnn_wide_step_speed.py's measure(): each
figure with its rounds' min and max); no profiler anywhere.

(a) The kernel pair, forward and forward + backward, at (N, D) = (1024, 512), (4096, 512), (9136, 512), (4096, 1024),
    (9136, 1024), (4096, 2048) -- 9136 = 8 clips x 1142 frames -- on L2-normalised rows, 122 classes, T = 0.07, and forward +
    backward with normalize on the same rows (the engines' use: the row epilogue launch and the dz staging).  The yardstick is
    tools/supcon_speed.py's torch_supcon: the same formula in eager fp32 torch ops on the same GPU with its own N x N tensors;
    its allocator peak is reported next to the kernel's workspace and gradient.
(b) The RNN model's graphed training step (--wide_rnn --wide_supcon) at hidden 512 and 1024, (B, S) = (8, 16) and (32, 32),
    with --supcon_weight 0 and 0.5.
(c) --narrow-only: the graphed step at hidden 128 with --supcon_weight 0.5 alone (no wide flag is touched, so this runs on
    any commit): the narrow launches, to be compared between two commits.
Prints one JSON line and writes it to --out.
    python tools/supcon_wide_speed.py [--rounds 7] [--reps 20] [--narrow-only] [--out profiles/supcon_wide_speed.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import rnn_step_speed as RS                        # make_inputs, K, HYPER
import rnn_wide_step_speed as RW                   # measure, _model_args
from supcon_speed import torch_supcon, peak_bytes, K, T

SHAPES = ((1024, 512), (4096, 512), (9136, 512), (4096, 1024), (9136, 1024), (4096, 2048))
STEP_SHAPES = ((8, 16), (32, 32))


def kernel_shape(N, D, rounds, reps, dev):
    from r3d_amd import ops
    g = torch.Generator().manual_seed(N + D)
    z = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).to(dev)
    y = torch.randint(0, K, (N,), generator=g).to(dev)
    ws = torch.empty(ops.supcon_ws_floats(N, D, False, wide=True), device=dev)
    ws_n = torch.empty(ops.supcon_ws_floats(N, D, True, wide=True), device=dev)
    loss, dz = torch.empty(1, device=dev), torch.empty(N, D, device=dev)

    def fwd(i=0):
        ops.supcon_fwd(z, y, N, N, ws, loss, temperature=T, wide=True)

    def fwd_bwd(i=0):
        fwd()
        ops.supcon_bwd(z, y, N, N, ws, dz, temperature=T, wide=True)

    def fwd_bwd_normalize(i=0):
        ops.supcon_fwd(z, y, N, N, ws_n, loss, temperature=T, normalize=True, wide=True)
        ops.supcon_bwd(z, y, N, N, ws_n, dz, temperature=T, normalize=True, wide=True)
    zt = z.clone().requires_grad_(True)

    def t_fwd(i=0):
        torch_supcon(zt.detach(), y)

    def t_fwd_bwd(i=0):
        zt.grad = None
        torch_supcon(zt, y).backward()
    got = RW.measure(dict(hip_fwd=fwd, hip_fwd_bwd=fwd_bwd, hip_fwd_bwd_normalize=fwd_bwd_normalize, torch_fwd=t_fwd,
                          torch_fwd_bwd=t_fwd_bwd), rounds, reps)
    out = dict(N=N, D=D)
    for n, (med, lo, hi) in got.items():
        out[n + "_ms"] = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
    out["hip_workspace_and_gradient_bytes"] = 4 * (ws.numel() + dz.numel())
    out["hip_normalize_workspace_and_gradient_bytes"] = 4 * (ws_n.numel() + dz.numel())
    out["torch_fwd_bwd_peak_bytes"] = peak_bytes(t_fwd_bwd)
    out["torch_over_hip_fwd"] = round(got["torch_fwd"][0] / got["hip_fwd"][0], 3)
    out["torch_over_hip_fwd_bwd"] = round(got["torch_fwd_bwd"][0] / got["hip_fwd_bwd"][0], 3)
    fwd_bwd()
    t_fwd_bwd()
    torch.cuda.synchronize()
    out["loss_hip"], out["loss_torch"] = round(float(loss), 6), round(float(torch_supcon(zt.detach(), y)), 6)
    out["grad_max_abs_diff_over_max_abs"] = float((dz - zt.grad).abs().max() / zt.grad.abs().max())
    return out


def step_config(B, S, H, batches, dev, weight):
    from r3d_amd.model.rnn import FUTR
    from r3d_amd.train_unimodal import _UnimodalSteps
    torch.manual_seed(1)
    model = FUTR(K, H, K + 1, dev, RW._model_args(H, H > 256), n_query=8, n_head=8, num_encoder_layers=2,
                 num_decoder_layers=1).to(dev)
    eng = model.engine()
    if H > 256:
        eng.wide_supcon = True
    eng.supcon_weight, eng.supcon_temperature = weight, T
    acc = (torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev),
           torch.zeros(1, dtype=torch.float64, device=dev))
    gs = _UnimodalSteps(eng, *acc)
    fn = lambda i: gs.step(batches[i % len(batches)], 1e-3, RS.HYPER, True)      # noqa: E731
    fn.check = lambda: bool(torch.isfinite(acc[0]).all() and torch.isfinite(acc[2]).all())
    return fn


def steps(Hs, weights, rounds, reps, dev):
    res = {}
    for B, S in STEP_SHAPES:
        batches = [RS.make_inputs(B, S, dev, seed=s) for s in range(4)]
        cfg = {f"H{H}_w{w}": step_config(B, S, H, batches, dev, w) for H in Hs for w in weights}
        res[f"B{B}_S{S}"] = {n: dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
                             for n, (med, lo, hi) in RW.measure(cfg, rounds, reps).items()}
        assert all(fn.check() for fn in cfg.values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--narrow-only", action="store_true", help="the graphed step at hidden 128, weight 0.5, alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(rounds=a.rounds, reps=a.reps, classes=K, temperature=T,
               timing="per figure: median (min, max) over the rounds of the mean of `reps` calls between one event pair; the "
                      "configurations of a group alternate inside every round")
    if a.narrow_only:
        res["narrow_rnn_step"] = steps((128,), (0.5,), a.rounds, a.reps, dev)
    else:
        res["kernels"] = [kernel_shape(N, D, a.rounds, max(a.reps // 2, 3), dev) for N, D in SHAPES]
        res["rnn_step"] = steps((512, 1024), (0.0, 0.5), a.rounds, a.reps, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
