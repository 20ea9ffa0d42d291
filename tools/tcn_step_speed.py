#!/usr/bin/env python3
"""ms/step of the TCN baseline's graphed training step (r3d_amd.model.tcn through r3d_amd.train_tcn's graphed steps: one
hipGraph per step, dropout on, 17 classes) at (B, S) = (8, 16), (16, 256) and (16, 1024): the median of --steps replays
over 4 alternating batches after a warm-up, each timed with its own pair of events.  As a yardstick only, the same model's
eager step through PyTorch's own layers on the same GPU and batches -- nn.Conv1d + torch.nn.utils.weight_norm (MIOpen
convolutions), nn.Dropout, the same loss, torch.optim.AdamW(foreach).  With --kernel-stats it also runs one process per
listed shape under `rocprofv3 --kernel-trace --stats` that replays the HIP step --prof-steps times, and keeps the per-kernel
summary (calls, total and mean ns).  Prints one JSON line and writes it to --out.
    python tools/tcn_step_speed.py [--steps 120] [--kernel-stats] [--out profiles/tcn_step_speed.json]"""
import argparse, csv, glob, json, os, shutil, statistics, subprocess, sys, tempfile, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

HYPER = (5e-3, (0.9, 0.999), 1e-8)
K, Q, D = 17, 8, 2048
PAD = K + 1
SHAPES = ((8, 16), (16, 256), (16, 1024))
STAT_SHAPES = ((8, 16), (16, 1024))
WIDTHS = (256, 512, 512, 256)


def make_inputs(B, S, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    feats = torch.randn(B, S, D, generator=g)
    tgt = torch.randint(0, K - 1, (B, Q), generator=g)
    tgt[1::2, Q - 3:] = PAD
    return [feats.to(dev), tgt.to(dev)]


def _median_ms(step, batches, steps, warmup=20):
    for i in range(warmup):
        step(batches[i % len(batches)])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for i, (a, b) in enumerate(ev):
        a.record()
        step(batches[i % len(batches)])
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def time_hip(batches, steps, dev):
    from r3d_amd.model.tcn import MustafaNet1DTCN
    from r3d_amd.train_tcn import _TcnSteps
    torch.manual_seed(1)
    model = MustafaNet1DTCN(num_classes=K, anticipated_frames=Q).to(dev).train()
    eng = model.engine()
    acc_l = torch.zeros(4, dtype=torch.float64, device=dev)
    acc_c = torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _TcnSteps(eng, acc_l, acc_c, pad_idx=PAD)
    ms = _median_ms(lambda b: gs.step(b, 1e-3, HYPER, True), batches, steps)
    assert torch.isfinite(acc_l).all() and torch.isfinite(eng.arena.params).all()
    return ms


class _Level(torch.nn.Module):
    def __init__(self, c_in, c_out, d):
        super().__init__()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wn = torch.nn.utils.weight_norm
            self.a = wn(torch.nn.Conv1d(c_in, c_out, 3, padding=2 * d, dilation=d))
            self.b = wn(torch.nn.Conv1d(c_out, c_out, 3, padding=2 * d, dilation=d))
        self.skip = torch.nn.Conv1d(c_in, c_out, 1) if c_in != c_out else None
        self.cut, self.drop = 2 * d, torch.nn.Dropout(0.2)

    def forward(self, x):
        y = self.drop(F.relu(self.a(x)[:, :, :-self.cut]))
        y = self.drop(F.relu(self.b(y)[:, :, :-self.cut]))
        return F.relu(y + (x if self.skip is None else self.skip(x)))


class TorchTCN(torch.nn.Module):
    """The same network in PyTorch's own layers: the yardstick, not the product."""

    def __init__(self):
        super().__init__()
        chans = (D,) + WIDTHS
        self.levels = torch.nn.Sequential(*[_Level(chans[i], chans[i + 1], 2 ** i) for i in range(4)])
        self.head = torch.nn.Conv1d(WIDTHS[-1], K * Q, 1)

    def forward(self, x):
        y = self.head(self.levels(x.permute(0, 2, 1)))
        return y.view(y.size(0), Q, K, y.size(2)).mean(dim=3)


def torch_step(model, opt, batch):
    feats, tgt = batch
    out = model(feats).reshape(-1, K)
    gold = torch.where(tgt == PAD, -1, tgt).reshape(-1)
    loss = F.cross_entropy(out, gold, ignore_index=-1, reduction="none").mean()
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()


def time_torch(batches, steps, dev):
    torch.manual_seed(1)
    model = TorchTCN().to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), 1e-3, weight_decay=5e-3, foreach=True)
    return _median_ms(lambda b: torch_step(model, opt, b), batches, steps)


def kernel_stats(B, S, prof_steps):
    """rocprofv3 --kernel-trace --stats over a child that replays the HIP step prof_steps times (after its warm-up)."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="tcn_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
           os.path.abspath(__file__), "--child", str(B), str(S), str(prof_steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=ROOT)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return dict(B=B, S=S, error=f"rocprofv3 rc={r.returncode}", tail=(r.stderr or r.stdout)[-600:])
    rows = list(csv.DictReader(open(files[0])))
    shutil.rmtree(d, ignore_errors=True)
    keep = [dict(name=row.get("Name", "")[:90], calls=int(row.get("Calls", 0)),
                 total_ns=int(float(row.get("TotalDurationNs", 0))), mean_ns=int(float(row.get("AverageNs", 0)))) for row in rows]
    keep.sort(key=lambda x: -x["total_ns"])
    return dict(B=B, S=S, replays=prof_steps + 20, kernels=keep[:16])


def child(B, S, steps):
    dev = torch.device("cuda", 0)
    time_hip([make_inputs(B, S, dev, seed=s) for s in range(4)], steps, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--prof-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, type=int, default=None)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    dev = torch.device("cuda", 0)
    res = {"num_classes": K, "steps": a.steps, "timing": "median of per-step event pairs, dropout on"}
    for B, S in SHAPES:
        batches = [make_inputs(B, S, dev, seed=s) for s in range(4)]
        hip = time_hip(batches, a.steps, dev)
        try:
            ref = time_torch(batches, a.steps, dev)
        except Exception as e:                      # noqa: BLE001  (the yardstick only: report, keep the HIP numbers)
            res[f"B{B}_S{S}"] = dict(hip_graphed_ms_per_step=round(hip, 4), torch_error=f"{type(e).__name__}: {e}"[:300])
            continue
        res[f"B{B}_S{S}"] = dict(hip_graphed_ms_per_step=round(hip, 4), torch_conv1d_eager_ms_per_step=round(ref, 4),
                                 torch_over_hip=round(ref / hip, 3))
        torch.cuda.empty_cache()
    if a.kernel_stats:
        res["kernel_stats"] = [kernel_stats(B, S, a.prof_steps) for B, S in STAT_SHAPES]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
