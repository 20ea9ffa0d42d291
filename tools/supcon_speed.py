#!/usr/bin/env python3
"""ms per launch of the supervised contrastive loss (csrc/supcon.hip): forward, and forward + backward, at (N, D) =
(128, 128), (4096, 128), (9136, 128) and (9136, 256) -- 9136 = 8 clips x 1142 frames, the DARai observation length --
as the median of --launches event pairs after a warm-up, rows L2-normalised, 122 classes, T = 0.07.  The yardstick is the
same formula in eager fp32 torch ops on the same GPU, with its own N x N logits, masks, exp and log-probabilities (and
what autograd keeps of them); its peak memory is reported next to the kernel's.

Then the graphed RNN step (tools/rnn_step_speed.py's model and batches) at (B, S, H) = (8, 16, 128) and (32, 32, 128)
with --supcon_weight 0 and 0.5, each measured twice in alternation: w = 0 runs the launches of the step without the flag,
so the spread of its two figures (and their distance from profiles/rnn_step_speed.json) is run-to-run noise.
Prints one JSON line and writes it to --out.
    python tools/supcon_speed.py [--launches 100] [--steps 200] [--out profiles/supcon_speed.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tools import rnn_step_speed as RS

SHAPES = ((128, 128), (4096, 128), (9136, 128), (9136, 256))
K, T = 122, 0.07


def torch_supcon(z, y, temperature=T, base_temperature=T):
    """The formula in torch ops, diagonal excluded from the log-sum-exp: the yardstick (its own restatement, N x N tensors)."""
    N = z.shape[0]
    s = (z @ z.t()) / temperature
    off = ~torch.eye(N, dtype=torch.bool, device=z.device)
    pos = (y[:, None] == y[None, :]) & off
    lse = torch.logsumexp(s.masked_fill(~off, float("-inf")), dim=1)
    P = pos.sum(1)
    mean_pos = (s * pos).sum(1) / P.clamp_min(1)
    return (-(temperature / base_temperature) * (mean_pos - lse) * (P > 0)).mean()


def median_ms(fn, launches, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    return statistics.median(ts)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def kernel_shape(N, D, launches, dev):
    from r3d_amd import ops
    g = torch.Generator().manual_seed(N + D)
    z = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).to(dev)
    y = torch.randint(0, K, (N,), generator=g).to(dev)
    ws = torch.empty(ops.supcon_ws_floats(N), device=dev)
    loss, dz = torch.empty(1, device=dev), torch.empty(N, D, device=dev)
    fwd = lambda: ops.supcon_fwd(z, y, N, N, ws, loss, temperature=T)                    # noqa: E731

    def fwd_bwd():
        fwd()
        ops.supcon_bwd(z, y, N, N, ws, dz, temperature=T)
    zt = z.clone().requires_grad_(True)
    t_fwd = lambda: torch_supcon(zt.detach(), y)                                         # noqa: E731

    def t_fwd_bwd():
        zt.grad = None
        torch_supcon(zt, y).backward()
    out = dict(N=N, D=D, hip_fwd_ms=round(median_ms(fwd, launches), 4), hip_fwd_bwd_ms=round(median_ms(fwd_bwd, launches), 4),
               torch_fwd_ms=round(median_ms(t_fwd, launches), 4), torch_fwd_bwd_ms=round(median_ms(t_fwd_bwd, launches), 4),
               hip_workspace_and_gradient_bytes=4 * (ws.numel() + dz.numel()), torch_fwd_bwd_peak_bytes=peak_bytes(t_fwd_bwd))
    out["torch_over_hip_fwd"] = round(out["torch_fwd_ms"] / out["hip_fwd_ms"], 3)
    out["torch_over_hip_fwd_bwd"] = round(out["torch_fwd_bwd_ms"] / out["hip_fwd_bwd_ms"], 3)
    fwd_bwd()
    t_fwd_bwd()
    torch.cuda.synchronize()
    out["loss_hip"], out["loss_torch"] = round(float(loss), 6), round(float(torch_supcon(zt.detach(), y)), 6)
    out["grad_max_abs_diff_over_max_abs"] = float((dz - zt.grad).abs().max() / zt.grad.abs().max())
    return out


def time_step(B, S, batches, steps, dev, weight):
    from r3d_amd.model.rnn import FUTR
    from r3d_amd.train_unimodal import _UnimodalSteps
    torch.manual_seed(1)
    model = FUTR(RS.K, RS.H, RS.K + 1, dev, RS._args(), n_query=8, n_head=8, num_encoder_layers=2, num_decoder_layers=1).to(dev)
    eng = model.engine()
    eng.supcon_weight, eng.supcon_temperature = weight, T
    acc = (torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev),
           torch.zeros(1, dtype=torch.float64, device=dev))
    gs = _UnimodalSteps(eng, *acc)
    for i in range(20):
        gs.step(batches[i % len(batches)], 1e-3, RS.HYPER, True)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        gs.step(batches[i % len(batches)], 1e-3, RS.HYPER, True)
    t1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(acc[0]).all() and torch.isfinite(acc[2]).all()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(launches=a.launches, steps=a.steps, classes=K, temperature=T,
               timing="median of per-launch event pairs after a warm-up; steps: events around the replays",
               kernels=[kernel_shape(N, D, a.launches, dev) for N, D in SHAPES], rnn_step=[])
    for B, S in RS.SHAPES:
        batches = [RS.make_inputs(B, S, dev, seed=s) for s in range(4)]
        ms = {0.0: [], 0.5: []}
        for _ in range(2):
            for w in (0.0, 0.5):
                ms[w].append(round(time_step(B, S, batches, a.steps, dev, w), 4))
        res["rnn_step"].append(dict(B=B, S=S, H=RS.H, graphed_ms_per_step_w0=ms[0.0], graphed_ms_per_step_w05=ms[0.5]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
