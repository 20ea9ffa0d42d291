#!/usr/bin/env python3
"""ms/step of the CNN baseline's graphed training step (model/cnn.py through r3d_amd.train_unimodal's graphed steps: one
hipGraph per step) at hidden 128, K = 122 (NTU) and (B, S) = (8, 16), (16, 256), (8, 1142):

  (a) the chain route (r3d_afft_head_step + r3d_cnn_seg_step) against the composed route, two engines in the same
      process, each warmed up on the shape, then --rounds alternating rounds of --steps replays each timed with events;
      the figure of a route is the median of its rounds;
  (b) as a yardstick only, the same model's eager step through PyTorch's own layers -- nn.Linear, adaptive pooling, the
      same three losses, torch.optim.AdamW(foreach) -- on the same GPU and batches, timed the same way once.

Also reports what engine_cnn.chain_pays says for each shape next to the route that was faster.
Prints one JSON line and writes it to --out.
    python tools/cnn_step_speed.py [--steps 100] [--rounds 7] [--out profiles/cnn_step_speed.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

HYPER = (5e-3, (0.9, 0.999), 1e-8)
K, H, D = 122, 128, 2048
SHAPES = ((8, 16), (16, 256), (8, 1142))


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


def _timed(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def hip_stepper(chain, batches, dev):
    from r3d_amd.model.cnn import FUTR
    from r3d_amd.train_unimodal import _UnimodalSteps
    torch.manual_seed(1)
    model = FUTR(K, H, K + 1, dev, _args(), n_query=8, n_head=8, num_encoder_layers=2, num_decoder_layers=1).to(dev)
    eng = model.engine()
    eng.use_seg_chain = chain
    acc_l = torch.zeros(4, dtype=torch.float64, device=dev)
    acc_c = torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _UnimodalSteps(eng, acc_l, acc_c)
    step = lambda i: gs.step(batches[i % len(batches)], 1e-3, HYPER, True)      # noqa: E731
    for i in range(20):                                                          # eager, capture, replays
        step(i)
    torch.cuda.synchronize()
    assert torch.isfinite(acc_l).all() and eng.last["chained"] == bool(chain)
    return step


class TorchCNN(torch.nn.Module):
    """The reference's live path in PyTorch's own layers: the yardstick, not the product."""

    def __init__(self):
        super().__init__()
        self.input_embed = torch.nn.Linear(D, H)
        self.fc_seg, self.fc, self.fc_len = torch.nn.Linear(H, K - 1), torch.nn.Linear(H, K), torch.nn.Linear(H, 1)

    def forward(self, src):
        x = F.relu(self.input_embed(src))
        pooled = F.adaptive_avg_pool1d(x.permute(0, 2, 1), 8).permute(0, 2, 1)
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
    model = TorchCNN().to(dev)
    opt = torch.optim.AdamW(model.parameters(), 1e-3, weight_decay=5e-3, foreach=True)
    step = lambda i: torch_step(model, opt, batches[i % len(batches)])          # noqa: E731
    for i in range(20):
        step(i)
    torch.cuda.synchronize()
    return _timed(step, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from r3d_amd.engine_cnn import chain_pays
    dev = torch.device("cuda", 0)
    res = {"H": H, "K": K, "steps": a.steps, "rounds": a.rounds,
           "what": "median over alternating rounds of the graphed step's ms/step, chain against composed, same process"}
    for B, S in SHAPES:
        batches = [make_inputs(B, S, dev, seed=s) for s in range(4)]
        steppers = {"chain": hip_stepper(True, batches, dev), "composed": hip_stepper(False, batches, dev)}
        ms = {"chain": [], "composed": []}
        for _ in range(a.rounds):
            for route in ("chain", "composed"):
                ms[route].append(_timed(steppers[route], a.steps))
        med = {r: statistics.median(v) for r, v in ms.items()}
        row = dict(chain_ms_per_step=round(med["chain"], 4), composed_ms_per_step=round(med["composed"], 4),
                   chain_rounds=[round(v, 4) for v in ms["chain"]], composed_rounds=[round(v, 4) for v in ms["composed"]],
                   faster="chain" if med["chain"] < med["composed"] else "composed",
                   chain_pays=bool(chain_pays(B, S, H, K - 1)))
        try:
            ref = time_torch(batches, a.steps, dev)
            row["torch_eager_ms_per_step"] = round(ref, 4)
            row["torch_over_best_hip"] = round(ref / min(med.values()), 3)
        except Exception as e:                      # noqa: BLE001  (the yardstick only: report, keep the HIP numbers)
            row["torch_error"] = f"{type(e).__name__}: {e}"[:300]
        res[f"B{B}_S{S}"] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
