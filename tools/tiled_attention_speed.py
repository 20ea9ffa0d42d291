#!/usr/bin/env python3
"""Kernel times of the tiled attention core (r3d_mha_tiled_fwd / _bwd, csrc/attention_tiled.hip) at B 8, heads 8, head
width 16, S in {64, 512, 1142}, and at head width 128, S 512: after a warm-up, the median of --launches launches, each timed
with its own pair of events on the launch stream (dropout mask and key labels given, q / k / v slices of one [N, 3H] buffer
as the engine lays them out).  Next to them the S x S core (r3d_mha_core_fwd / _bwd) at S 64, the only shape both run, and as
a yardstick fp32 torch.nn.functional.scaled_dot_product_attention, forward and forward + backward, at every shape on the same
GPU.  Then the depth-query model's graphed training step (--long_clips, hidden 128, 8 heads, one decoder layer, 160 x 120
depth frames, dropout on) at (B, S) = (8, 512) and (8, 1142): the median of --steps replays over 2 alternating batches.
Prints one JSON line and writes it to --out.
    python tools/tiled_attention_speed.py [--launches 100] [--steps 50] [--out profiles/tiled_attention_speed.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

B, HEADS = 8, 8
KERNEL_SHAPES = ((64, 16), (512, 16), (1142, 16), (512, 128))          # (S, head width)
STEP_SHAPES = ((8, 512), (8, 1142))
HYPER = (5e-3, (0.9, 0.999), 1e-8)
K, Q, D, HW = 17, 8, 2048, (120, 160)
PAD = K + 1


def median_ms(fn, n, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return round(statistics.median(a.elapsed_time(b) for a, b in ev), 4)


def kernel_times(S, dh, n, dev):
    from r3d_amd import ops
    H = HEADS * dh
    g = torch.Generator().manual_seed(S + dh)
    qkv = torch.randn(B * S, 3 * H, generator=g).to(dev)
    d_o = torch.randn(B * S, H, generator=g).to(dev)
    keep = (torch.rand(B, HEADS, S, S, generator=g) > 0.1).to(torch.uint8).to(dev)
    lab = torch.zeros(B, S, dtype=torch.int64)
    lab[1::2, S - S // 4:] = PAD                                        # every other clip: a padded last quarter
    lab = lab.to(dev)
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    o, lse, delta = torch.empty(B * S, H, device=dev), torch.empty(B, HEADS, S, device=dev), torch.empty(B, HEADS, S, device=dev)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:]
    kw = dict(key_labels=lab, pad_idx=PAD, drop_mask=keep, drop_scale=1 / 0.9)
    res = dict(S=S, dh=dh)
    res["tiled_fwd_ms"] = median_ms(lambda: ops.mha_tiled_fwd(q, k, v, o, lse, B, HEADS, S, S, dh, **kw), n)
    res["tiled_bwd_ms"] = median_ms(lambda: ops.mha_tiled_bwd(q, k, v, o, lse, d_o, delta, dq, dk, dv, B, HEADS, S, S, dh, **kw), n)
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all()
    if ops.mha_core_supported(S, S, dh, True):
        probs = torch.empty(B, HEADS, S, S, device=dev)
        res["core_fwd_ms"] = median_ms(lambda: ops.mha_core_fwd(q, k, v, probs, o, B, HEADS, S, S, dh, **kw), n)
        res["core_bwd_ms"] = median_ms(lambda: ops.mha_core_bwd(q, k, v, probs, d_o, dq, dk, dv, B, HEADS, S, S, dh, drop_mask=keep,
                                                                drop_scale=1 / 0.9), n)
    # yardstick: torch's own fp32 attention on [B, heads, S, dh] tensors, key mask as an additive bias, dropout inside
    try:
        tq, tk, tv = (t.reshape(B, S, HEADS, dh).transpose(1, 2).contiguous().requires_grad_(True) for t in (q, k, v))
        tdo = d_o.reshape(B, S, HEADS, dh).transpose(1, 2).contiguous()
        bias = torch.zeros(B, 1, 1, S, device=dev).masked_fill((lab == PAD)[:, None, None, :], float("-inf"))
        sdpa = lambda: F.scaled_dot_product_attention(tq, tk, tv, attn_mask=bias, dropout_p=0.1)       # noqa: E731
        with torch.no_grad():
            res["torch_sdpa_fwd_ms"] = median_ms(sdpa, n)

        def both():
            tq.grad = tk.grad = tv.grad = None
            sdpa().backward(tdo)
        res["torch_sdpa_fwd_bwd_ms"] = median_ms(both, n)
    except Exception as e:                      # noqa: BLE001  (the yardstick only: report, keep the HIP numbers)
        res["torch_error"] = f"{type(e).__name__}: {e}"[:300]
    return res


def step_time(Bc, S, steps, dev):
    from r3d_amd.model.futr_unsupervised_depth import FUTR
    from r3d_amd.train_proposed_depth import _GraphedSteps
    from oracle import synth
    args = argparse.Namespace(input_dim=D, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript", long_clips=True)
    torch.manual_seed(1)
    model = FUTR(K, 128, PAD, dev, args, n_query=Q, n_head=HEADS, num_encoder_layers=2, num_decoder_layers=1,
                 depth_pixels=HW[0] * HW[1]).to(dev).train()
    eng = model.engine()
    batches = []
    for s in range(2):                 # labels / targets as the suite's batches; the large depth frames drawn on the device
        b = [torch.from_numpy(x).to(dev) for x in synth.make_batch(Bc, S, K, PAD, 7 + s, depth_hw=(1, 1), pad_tail=True)]
        b[1] = torch.rand(Bc, S, 1, HW[0], HW[1], device=dev, generator=torch.Generator(device=dev).manual_seed(s))
        batches.append(b)
    acc_l, acc_c = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    gs = _GraphedSteps(eng, acc_l, acc_c, None, PAD)
    i = [0]

    def step():
        gs.step(batches[i[0] % 2], 1e-3, HYPER, True)
        i[0] += 1
    ms = median_ms(step, steps, warmup=6)
    w = eng.last["w"]
    assert w.route == "tiled" and torch.isfinite(acc_l).all() and torch.isfinite(eng.arena.params[:eng.arena.n_live]).all()
    return dict(B=Bc, S=S, graphed_ms_per_step=ms, probs_floats_not_allocated=2 * Bc * HEADS * S * S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"B": B, "heads": HEADS, "launches": a.launches, "steps": a.steps,
           "timing": "median of per-launch (per-step) event pairs after a warm-up; dropout mask and key labels given"}
    res["kernels"] = [kernel_times(S, dh, a.launches, dev) for S, dh in KERNEL_SHAPES]
    torch.cuda.empty_cache()
    res["depth_query_step"] = []
    for Bc, S in STEP_SHAPES:
        res["depth_query_step"].append(step_time(Bc, S, a.steps, dev))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
