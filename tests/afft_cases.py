"""Shapes of the AFFT baseline's new ground: the pooled-head chain (csrc/afft.hip: r3d_afft_head_fwd / r3d_afft_head_step)
and the engine's shape admission (r3d_amd/engine_afft.check_afft_shape).  tests/test_afft_gpu.py runs every kernel row on the
device against the float64 restatement tests/afft_oracle.tail; tests/test_afft_cpu.py checks the admission rows.

A cross, not the full product, of S in {1, 6, 8, 16, 37, 200, 520}, Q in {1, 3, 8, 32}, K + 1 in {18, 50, 123}, H in {8, 64,
128, 136, 1024}, B in {1, 13}: every branch of the kernel is reached -- S < Q (repeated frames), S == Q, S % Q != 0
(windows overlapping by one frame), windows of 65 and 67 frames, one to sixteen channel chunks per lane in the head
products, K <= 64 and K > 64 in ce_row, more clips than any one wave handles, and LDS requests past the 64 KiB default.

flavour: "" plain synthetic labels; "padtgt": clip 0's targets and durations all pad_idx; "padpast": clip 0's past labels
all pad_idx (its CE weight compares pad_idx with the first target); "oob": one target outside [0, K), which the kernels
ignore (PyTorch would raise: the restatement is handed pad_idx in its place)."""
import collections

import numpy as np
import torch

Kernel = collections.namedtuple("Kernel", "B S Q K1 H flavour why")

KERNEL_CASES = [
    Kernel(1, 1, 1, 18, 8, "", "the smallest of everything: one frame, one query, one lane chunk"),
    Kernel(2, 6, 8, 18, 64, "", "S < Q: frames repeat (the afft_tiny fixture's shape)"),
    Kernel(13, 8, 8, 18, 128, "", "S == Q: windows of one frame; 13 clips"),
    Kernel(8, 16, 8, 18, 128, "", "the headline shape"),
    Kernel(3, 37, 8, 123, 136, "", "off-grid width, overlapping windows, K > 64 in ce_row"),
    Kernel(2, 200, 3, 50, 128, "", "windows of 67 frames, Q = 3: fewer queries than waves"),
    Kernel(1, 520, 32, 18, 64, "", "a long clip on 32 queries: windows of 17 frames, overlapping"),
    Kernel(1, 16, 32, 123, 136, "", "S < Q at 32 queries, 123 head outputs"),
    Kernel(2, 16, 8, 18, 1024, "", "the widest hidden: sixteen chunks per lane"),
    Kernel(1, 37, 32, 50, 1024, "", "134 KiB of LDS: past the 64 KiB default request"),
    Kernel(13, 37, 3, 50, 8, "", "the narrowest hidden on 13 clips"),
    Kernel(2, 16, 8, 18, 128, "padtgt", "a clip whose targets are all pad_idx"),
    Kernel(2, 16, 8, 18, 128, "padpast", "a clip whose past labels are all pad_idx"),
    Kernel(2, 16, 8, 18, 128, "oob", "one target outside [0, K)"),
]


def kernel_id(c):
    return f"B{c.B}-S{c.S}-Q{c.Q}-K1_{c.K1}-H{c.H}" + (f"-{c.flavour}" if c.flavour else "")


def kernel_inputs(c, seed=0):
    """CPU tensors of a kernel case: fused [B, S, H], w_head [K + 1, H], b_head [K + 1], past_label [B, S], dur [B, Q],
    tgt [B, Q] (what the device gets) and tgt_oracle (what the restatement gets), pad_idx."""
    K = c.K1 - 1
    pad = K + 1
    g = torch.Generator().manual_seed(1000 + seed + 7 * c.B + 13 * c.S + 17 * c.Q + 19 * c.K1 + 23 * c.H)
    fused = torch.randn(c.B, c.S, c.H, generator=g)
    w_head = torch.randn(c.K1, c.H, generator=g) / float(np.sqrt(c.H))
    b_head = 0.1 * torch.randn(c.K1, generator=g)
    lab = torch.randint(0, max(K - 1, 1), (c.B, c.S), generator=g)
    for b in range(1, c.B, 2):
        lab[b, c.S - max(c.S // 8, 1):] = pad                # odd clips end in padding (when that leaves a frame, or not)
    nq = torch.randint(1, c.Q + 1, (c.B,), generator=g)
    tgt = torch.randint(0, max(K - 1, 1), (c.B, c.Q), generator=g)
    dur = torch.rand(c.B, c.Q, generator=g) + 0.05
    for b in range(c.B):
        k = int(nq[b])
        dur[b, :k] = dur[b, :k] / dur[b, :k].sum()
        if k < c.Q:
            tgt[b, k - 1] = K - 1
            tgt[b, k:] = pad
            dur[b, k:] = float(pad)
    if c.flavour == "padtgt":
        tgt[0, :] = pad
        dur[0, :] = float(pad)
    if c.flavour == "padpast":
        lab[0, :] = pad
    tgt_oracle = tgt.clone()
    if c.flavour == "oob":
        dur[0] = 1.0 / c.Q                                   # (clip 0: every query live)
        tgt[0] = torch.arange(c.Q) % max(K - 1, 1)
        tgt_oracle = tgt.clone()
        tgt[0, 1] = K + 5
        tgt_oracle[0, 1] = pad
    return dict(fused=fused, w_head=w_head, b_head=b_head, lab=lab, dur=dur.float(), tgt=tgt, tgt_oracle=tgt_oracle, pad=pad)


# ---- tolerances of the new kernels ---------------------------------------------------------------------------------------
# Error of the SAME formulas in float32 torch on the CPU against the float64 restatement (afft_oracle.tail at both
# precisions), max |err| / max |float64 value| per quantity, worst over KERNEL_CASES -- measured by
# `python -m tests.afft_cases`, never against the kernel's output:
FP32_CPU_WORST = {              # (the case that sets it)
    "pooled": 2.40e-07,         # B2-S200-Q3-K1_50-H128
    "actdur": 3.82e-07,         # B2-S16-Q8-K1_18-H128-padtgt
    "d_actdur": 2.57e-07,       # B13-S8-Q8-K1_18-H128
    "d_fused": 4.04e-07,        # B1-S16-Q32-K1_123-H136
    "losses": 1.26e-07,         # B8-S16-Q8-K1_18-H128
}
# The kernels add the same terms in another order than torch's blocked CPU sums: sequentially over a window's frames, lane
# strided then a butterfly over hidden.  Rounding grows like sqrt(depth) of a summation order; the deepest sequential run
# here is 1024 terms against torch's ~10 levels, sqrt(1024 / 10) ~ 10, and expf / logf are within 2 ulp on both sides: 16 x.
FACTOR = 16.0
KERNEL_RTOL = {k: FACTOR * v for k, v in FP32_CPU_WORST.items()}

# ---- engine admission ------------------------------------------------------------------------------------------------------
# (B, S, H, n_head, n_query, n_class) the engine must admit ...
ADMITTED = [(c.B, c.S, c.H, 8 if c.H % 8 == 0 and c.H >= 8 else 1, c.Q, c.K1 - 1) for c in KERNEL_CASES] + [
    (1, 1, 8, 1, 1, 17), (8, 16, 128, 8, 8, 17), (3, 37, 136, 8, 8, 122), (2, 6, 64, 8, 8, 17), (8, 1142, 128, 8, 8, 17),
    (16, 256, 128, 8, 8, 17), (1, 5000, 128, 8, 8, 17),            # past max_pos_len 2000: pos_embedding is never used
    (13, 520, 1024, 16, 32, 17), (1, 16, 1024, 8, 32, 122), (2, 16, 512, 8, 64, 17)]
# ... and the ones it refuses, with a word of the message that names the limit
REFUSED = [
    ((2, 16, 1032, 8, 8, 17), "1024"),                 # past the plain seam
    ((2, 16, 132, 8, 8, 17), "% 8"),                   # hidden % 8
    ((2, 16, 136, 16, 8, 17), "n_head"),               # hidden % n_head
    ((0, 16, 128, 8, 8, 17), "at least one clip"),
    ((2, 0, 128, 8, 8, 17), "at least one"),
    ((2, 16, 128, 8, 0, 17), "n_query"),
    ((2, 16, 128, 8, 65, 17), "n_query"),
    ((2, 16, 128, 8, 8, 1024), "head outputs"),
    ((2, 16, 1024, 8, 64, 122), "LDS"),                # 64 x (1024 + 123) floats = 287 KiB
    ((2, 16, 1024, 8, 40, 17), "LDS"),                 # 40 x (1024 + 18) floats = 163 KiB > 152 KiB
]

# ---- step cases of the engine beyond the fixtures: (B, S, H, n_class, depth_hw) -- small depth maps through depth_pixels
STEP_CASES = [(1, 1, 64, 17, (6, 8)), (13, 8, 128, 17, (6, 8)), (2, 200, 128, 49, (6, 8)), (2, 16, 1024, 17, (6, 8))]


def measure():
    """Prints the float32-CPU errors the tolerances above come from."""
    from tests import afft_oracle as AO
    worst = {}
    for c in KERNEL_CASES:
        x = kernel_inputs(c)
        r64 = AO.tail(x["fused"].double(), x["w_head"].double(), x["b_head"].double(), c.Q, x["lab"], x["dur"], x["tgt_oracle"],
                      x["pad"])
        r32 = AO.tail(x["fused"], x["w_head"], x["b_head"], c.Q, x["lab"], x["dur"], x["tgt_oracle"], x["pad"])
        line = []
        for k in FP32_CPU_WORST:
            a, b = torch.as_tensor(r32[k]).double(), torch.as_tensor(r64[k]).double()
            e = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
            line.append(f"{k} {e:.2e}")
            if e > worst.get(k, (0.0, ""))[0]:
                worst[k] = (e, kernel_id(c))
        print(kernel_id(c), " ".join(line))
    print({k: (f"{v[0]:.2e}", v[1]) for k, v in worst.items()})


if __name__ == "__main__":
    measure()
