#!/usr/bin/env python3
"""What the stepwise LSTM route (csrc/lstm_steps.hip, opts --wide_rnn) costs, in one process, with device events, as medians
of --rounds alternating rounds after a warm-up; no profiler anywhere.

(a) One bidirectional layer's recurrence, forward and forward + backward (the GEMMs around it excluded), each captured as one
    hipGraph and replayed: the steps route at hidden 128 / 256 / 512 / 1024, the registers route (csrc/lstm.hip) at 128 / 256,
    at (B, S) = (8, 16), (32, 32), (16, 64); us per time step is derived from each.
(b) The RNN model's graphed training step (122 classes) at hidden 512 and 1024 (--wide_rnn) and at hidden 256 (the registers
    route: the same launches as before the flag existed), same shapes, beside the eager step of the same model in PyTorch's own
    layers (nn.LSTM on MIOpen + torch.optim.AdamW) on the same GPU: a yardstick, not a kernel-for-kernel comparison.
Prints one JSON line and writes it to --out.
    python tools/rnn_wide_step_speed.py [--rounds 7] [--only-h256] [--out profiles/rnn_wide_step_speed.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import torch.nn.functional as F

import rnn_step_speed as RS                        # make_inputs, torch_step, K, D, HYPER

SHAPES = ((8, 16), (32, 32), (16, 64))
K, D = RS.K, RS.D


def _events(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(reps):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def layer_config(B, S, H, route, with_bwd, dev):
    """A closure replaying one layer's recurrence (forward, or forward + backward) from a captured graph."""
    from r3d_amd import ops
    h, N = H // 2, B * S
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + S * 7 + H)
    r = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / h ** 0.5).to(dev)      # noqa: E731
    gin, dy = (torch.rand(N, 4 * H, generator=g) * 2 - 1).to(dev), (torch.rand(N, H, generator=g) - 0.5).to(dev)
    whh, bhh = [r(4 * h, h), r(4 * h, h)], [r(4 * h), r(4 * h)]
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)      # noqa: E731
    y, gates, cell, hp, dg = e(N, H), e(N, 4 * H), e(N, H), e(N, H), e(N, 4 * H)
    lws = e(ops.lstm_steps_ws_floats(B, H)) if route == "steps" else None

    def run():
        if route == "steps":
            ops.lstm_steps_layer_fwd(gin, whh[0], whh[1], bhh[0], bhh[1], y, gates, cell, hp, B, S)
            if with_bwd:
                ops.lstm_steps_layer_bwd(dy, whh[0], whh[1], gates, cell, dg, B, S, lws)
        else:
            ops.lstm_layer_fwd(gin, whh[0], whh[1], bhh[0], bhh[1], y, gates, cell, hp, B, S)
            if with_bwd:
                ops.lstm_layer_bwd(dy, whh[0], whh[1], gates, cell, dg, B, S)
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    fn = lambda i: graph.replay()      # noqa: E731
    # the graph holds raw addresses: its buffers must outlive it (the next capture's empty_cache() would release them)
    fn.keep = (gin, dy, whh, bhh, y, gates, cell, hp, dg, lws)
    return fn


def _model_args(H, wide):
    return argparse.Namespace(input_dim=D, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript",
                              hidden_dim=H, n_query=8, n_head=8, wide_rnn=wide)


def hip_step_config(B, S, H, batches, dev):
    from r3d_amd.model.rnn import FUTR
    from r3d_amd.train_unimodal import _UnimodalSteps
    torch.manual_seed(1)
    model = FUTR(K, H, K + 1, dev, _model_args(H, H > 256), n_query=8, n_head=8, num_encoder_layers=2,
                 num_decoder_layers=1).to(dev)
    eng = model.engine()
    acc_l = torch.zeros(4, dtype=torch.float64, device=dev)
    acc_c = torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _UnimodalSteps(eng, acc_l, acc_c)
    fn = lambda i: gs.step(batches[i % len(batches)], 1e-3, RS.HYPER, True)      # noqa: E731
    fn.check = lambda: bool(torch.isfinite(acc_l).all())
    return fn


class TorchRNN(torch.nn.Module):
    """rnn_step_speed.TorchRNN at hidden H: the reference's live path in PyTorch's own layers (the yardstick)."""

    def __init__(self, H):
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


def torch_step_config(H, batches, dev):
    torch.manual_seed(1)
    model = TorchRNN(H).to(dev)
    opt = torch.optim.AdamW(model.parameters(), 1e-3, weight_decay=5e-3, foreach=True)
    return lambda i: RS.torch_step(model, opt, batches[i % len(batches)])


def measure(configs, rounds, reps):
    """configs: {name: fn(i)}.  A warm-up pass, then `rounds` passes over all of them in turn; (median, min, max) ms per call."""
    for fn in configs.values():
        _events(fn, max(reps // 4, 3))
    got = {n: [] for n in configs}
    for _ in range(rounds):
        for n, fn in configs.items():
            got[n].append(_events(fn, reps))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-h256", action="store_true", help="the graphed step at hidden 256 alone (runs on any commit)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"K": K, "rounds": a.rounds, "reps": a.reps}
    if not a.only_h256:
        layer = {}
        for B, S in SHAPES:
            cfg = {}
            for route, Hs in (("steps", (128, 256, 512, 1024)), ("registers", (128, 256))):
                for H in Hs:
                    for bwd in (False, True):
                        cfg[f"{route}_H{H}_{'fwd_bwd' if bwd else 'fwd'}"] = layer_config(B, S, H, route, bwd, dev)
            out = {}
            for n, (med, lo, hi) in measure(cfg, a.rounds, a.reps).items():
                launches = S * (2 if n.endswith("fwd_bwd") else 1)
                out[n] = dict(us=round(med * 1e3, 2), us_min=round(lo * 1e3, 2), us_max=round(hi * 1e3, 2),
                              us_per_step=round(med * 1e3 / launches, 3))
            layer[f"B{B}_S{S}"] = out
        res["layer"] = layer
    step = {}
    for B, S in SHAPES:
        batches = [RS.make_inputs(B, S, dev, seed=s) for s in range(4)]
        cfg = {}
        for H in ((256,) if a.only_h256 else (256, 512, 1024)):
            cfg[f"hip_graphed_H{H}"] = hip_step_config(B, S, H, batches, dev)
            if not a.only_h256:
                cfg[f"torch_eager_H{H}"] = torch_step_config(H, batches, dev)
        out = {n: dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
               for n, (med, lo, hi) in measure(cfg, a.rounds, a.reps).items()}
        assert all(fn.check() for fn in cfg.values() if hasattr(fn, "check"))
        step[f"B{B}_S{S}"] = out
    res["step"] = step
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
