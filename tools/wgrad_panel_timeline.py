#!/usr/bin/env python3
"""In-kernel timeline of the persistent bf16x3 weight-gradient panel kernel (wgrad_panel_bf3_kernel, tile 7) at the headline
shape (K = 128 tokens, M = 128, N = 50176); needs a build with R3D_EXTRA_DEFS=-DR3D_NT_PROBE=16.  Workgroup 16, consumer
wave 0 and producer wave 4; wall_clock64 marks (100 MHz, printed in us since the producer's first mark, medians of 10 launches).
Marks of turn p -- consumer: 1 + 5 p turn start, 2 + 5 p MFMAs issued, 3 + 5 p past the mid-turn barrier, 4 + 5 p C tile
written to LDS, 5 + 5 p past the second barrier; producer: 0 kernel start, 1 + 5 p turn start, 2 + 5 p previous C tile drained,
3 + 5 p next image split and stored and the refill loads issued, 4 + 5 p / 5 + 5 p past the two barriers, 30 last C tile drained."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from r3d_amd import ops  # noqa: E402
from r3d_amd._lib import GEMM_TN  # noqa: E402

K, M, N = 128, 128, 50176
a = torch.randn(K, M, device="cuda") * 0.05
b = torch.rand(K, N, device="cuda")
cbig = torch.zeros(M + 1, N, device="cuda")               # one spare row behind C for the marks
c = cbig[:M]
ws = ops.GemmWorkspace("cuda")
rows = []
for it in range(12):
    d = ops.gemm(GEMM_TN, a, b, c, ws=ws, prec=1)
    torch.cuda.synchronize()
    marks = cbig[M, :256].view(torch.int64).cpu().double() / 100.0
    if it >= 2:
        rows.append(marks)
x = torch.stack(rows)
assert d.tile == 7, d.tile
print(f"tile {d.tile} K {K} M {M} N {N} ({(N + 63) // 64} panels)")
base = x[:, 64]
for role, name in ((0, "consumer wave 0"), (1, "producer wave 4")):
    seg = x[:, role * 64: role * 64 + 64]
    used = [i for i in range(64) if float(seg[:, i].max()) > 0]
    print(f"  {name}: " + "  ".join(f"[{i}] {float((seg[:, i] - base).median()):.2f}" for i in used))
