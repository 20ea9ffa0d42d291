#!/usr/bin/env python3
"""ms/step of the RNN baseline's graphed training step (model/rnn.py through r3d_amd.train_unimodal's graphed steps: one
hipGraph per step) at 8 clips x 16 frames and 32 clips x 32 frames, hidden 128, K = 122 (NTU), timed with events around
--steps replays over 4 alternating batches after a warm-up.  As a yardstick only, the same model's eager step through
PyTorch's own layers -- nn.LSTM (MIOpen), nn.Linear, adaptive pooling, the same three losses, torch AdamW(foreach) -- on
the same GPU and batches.  With --kernel-stats it also runs one process under `rocprofv3 --kernel-trace --stats` that
replays the HIP step --prof-steps times, and keeps the per-kernel summary (calls, total and mean ns).
Prints one JSON line and writes it to --out.
    python tools/rnn_step_speed.py [--steps 200] [--kernel-stats] [--out profiles/rnn_step_speed.json]"""
import argparse, csv, glob, json, os, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

HYPER = (5e-3, (0.9, 0.999), 1e-8)
K, H, D = 122, 128, 2048
SHAPES = ((8, 16), (32, 32))


def _args():
    return argparse.Namespace(input_dim=D, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript",
                              hidden_dim=H, n_query=8, n_head=8)


def make_inputs(B, S, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    pad = K + 1
    feats = torch.randn(B, S, D, generator=g)
    lab = torch.randint(0, K - 1, (B, S), generator=g)
    lab[1::2, S - max(S // 8, 1):] = pad
    tgt = torch.randint(0, K - 1, (B, 8), generator=g)
    dur = torch.rand(B, 8, generator=g) + 0.05
    dur = dur / dur.sum(1, keepdim=True)
    return [t.to(dev) for t in (feats, lab, dur, tgt)]


def time_hip(B, S, batches, steps, dev):
    from r3d_amd.model.rnn import FUTR
    from r3d_amd.train_unimodal import _UnimodalSteps
    torch.manual_seed(1)
    model = FUTR(K, H, K + 1, dev, _args(), n_query=8, n_head=8, num_encoder_layers=2, num_decoder_layers=1).to(dev)
    eng = model.engine()
    acc_l = torch.zeros(4, dtype=torch.float64, device=dev)
    acc_c = torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _UnimodalSteps(eng, acc_l, acc_c)
    for i in range(20):
        gs.step(batches[i % len(batches)], 1e-3, HYPER, True)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        gs.step(batches[i % len(batches)], 1e-3, HYPER, True)
    t1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(acc_l).all()
    return t0.elapsed_time(t1) / steps


class TorchRNN(torch.nn.Module):
    """The reference's live path in PyTorch's own layers (nn.LSTM runs on MIOpen): the yardstick, not the product."""

    def __init__(self):
        super().__init__()
        self.rnn = torch.nn.LSTM(H, H // 2, num_layers=2, batch_first=True, bidirectional=True)
        self.rnn_fc, self.input_embed = torch.nn.Linear(H, H), torch.nn.Linear(D, H)
        self.fc_seg, self.fc, self.fc_len = torch.nn.Linear(H, K - 1), torch.nn.Linear(H, K), torch.nn.Linear(H, 1)

    def forward(self, src):
        x = F.relu(self.input_embed(src))
        y, _ = self.rnn(x)
        tgt = self.rnn_fc(y)
        pooled = F.adaptive_avg_pool1d(tgt.permute(0, 2, 1), 8).permute(0, 2, 1)
        return self.fc(pooled), self.fc_len(pooled).squeeze(2), self.fc_seg(x)


def torch_step(model, opt, batch):
    feats, lab, dur, tgt = batch
    pad = K + 1
    act, d, seg = model(feats)
    ls = F.cross_entropy(seg.reshape(-1, K - 1), torch.where((lab == pad) | (lab == 120), -1, lab).reshape(-1),
                         ignore_index=-1, reduction="none").mean()
    la = F.cross_entropy(act.reshape(-1, K), torch.where((tgt == pad) | (tgt == 120), -1, tgt).reshape(-1), ignore_index=-1)
    m = (dur != pad).float()
    od = F.normalize(torch.exp(d) * m, p=1, dim=-1)
    ld = ((od - dur * m) ** 2).sum() / m.sum()
    opt.zero_grad(set_to_none=True)
    (ls + la + ld).backward()
    opt.step()


def time_torch(batches, steps, dev):
    torch.manual_seed(1)
    model = TorchRNN().to(dev)
    opt = torch.optim.AdamW(model.parameters(), 1e-3, weight_decay=5e-3, foreach=True)
    for i in range(20):
        torch_step(model, opt, batches[i % len(batches)])
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        torch_step(model, opt, batches[i % len(batches)])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def kernel_stats(B, S, prof_steps):
    """rocprofv3 --kernel-trace --stats over a child that replays the HIP step prof_steps times (after its warm-up)."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="rnn_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
           os.path.abspath(__file__), "--child", str(B), str(S), str(prof_steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=ROOT)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return dict(error=f"rocprofv3 rc={r.returncode}", tail=(r.stderr or r.stdout)[-600:])
    rows = list(csv.DictReader(open(files[0])))
    shutil.rmtree(d, ignore_errors=True)
    keep = []
    for row in rows:
        keep.append(dict(name=row.get("Name", "")[:90], calls=int(row.get("Calls", 0)),
                         total_ns=int(float(row.get("TotalDurationNs", 0))), mean_ns=int(float(row.get("AverageNs", 0)))))
    keep.sort(key=lambda x: -x["total_ns"])
    return dict(B=B, S=S, replays=prof_steps + 20, kernels=keep[:24])


def child(B, S, steps):
    dev = torch.device("cuda", 0)
    batches = [make_inputs(B, S, dev, seed=s) for s in range(4)]
    time_hip(B, S, batches, steps, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--prof-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, type=int, default=None)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    dev = torch.device("cuda", 0)
    res = {"H": H, "K": K, "steps": a.steps}
    for B, S in SHAPES:
        batches = [make_inputs(B, S, dev, seed=s) for s in range(4)]
        hip = time_hip(B, S, batches, a.steps, dev)
        try:
            ref = time_torch(batches, a.steps, dev)
        except Exception as e:                      # noqa: BLE001  (the yardstick only: report, keep the HIP numbers)
            res[f"B{B}_S{S}"] = dict(hip_graphed_ms_per_step=round(hip, 4), torch_error=f"{type(e).__name__}: {e}"[:300])
            continue
        res[f"B{B}_S{S}"] = dict(hip_graphed_ms_per_step=round(hip, 4), torch_nn_lstm_eager_ms_per_step=round(ref, 4),
                                 torch_over_hip=round(ref / hip, 3))
    if a.kernel_stats:
        res["kernel_stats"] = kernel_stats(8, 16, a.prof_steps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
