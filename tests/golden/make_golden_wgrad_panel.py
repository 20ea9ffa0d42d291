#!/usr/bin/env python3
"""Records the output of the bf16x3 weight-gradient panel kernel (tile 7) for a seeded (K, M, N) = (128, 128, 2112) on the GPU:

    python tests/golden/make_golden_wgrad_panel.py [OUT.npz]

tests/test_wgrad_panel_gpu.py holds later versions of the kernel to this recording bit for bit.  The raw output (1.03 MiB of
fp32 with random mantissas) does not compress, so the file stores it LOSSLESSLY as the integer distance of every element's bit
pattern from a base that any machine recomputes exactly: the float64 product summed over k in order with numpy's elementwise
multiply and add (one IEEE operation each, no BLAS, no contraction), rounded to fp32.  The distances are a few units in the
last place and compress well; sha256 sums of the operands and of the raw output guard the seeded generators and the encoding."""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

K, M, N = 128, 128, 2112


def operands():
    a = torch.randn(K, M, generator=torch.Generator().manual_seed(1287)) * 0.05
    b = torch.rand(K, N, generator=torch.Generator().manual_seed(2112))          # depth-like inputs in [0, 1)
    return a, b


def base_bits(a, b):
    """int32 bit patterns of fp32(sum_k a[k, m] * b[k, n]), the sum in float64 and in k order."""
    a64, b64 = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
    s = np.zeros((M, N), dtype=np.float64)
    for k in range(K):
        s = s + a64[k][:, None] * b64[k][None, :]
    return s.astype(np.float32).view(np.int32)


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def decode(z, a, b):
    """The recorded output as int32 bit patterns (checks the operands' and the output's sums)."""
    assert str(z["sha_a"]) == sha(a.numpy()) and str(z["sha_b"]) == sha(b.numpy()), "the seeded operands differ from the recording's"
    bits = base_bits(a, b) + z["delta"]
    assert str(z["sha_c"]) == sha(bits), "the recording does not decode to the recorded output"
    return bits


if __name__ == "__main__":
    from r3d_amd import ops
    from r3d_amd._lib import GEMM_TN
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wgrad_panel_128x128x2112.npz")
    a, b = operands()
    c = torch.empty(M, N, device="cuda")
    d = ops.gemm(GEMM_TN, a.cuda(), b.cuda(), c, ws=ops.GemmWorkspace("cuda"), prec=1)
    torch.cuda.synchronize()
    assert d.tile == 7, d.tile
    bits = c.cpu().numpy().view(np.int32)
    delta = bits - base_bits(a, b)                    # (int32, wraps where the signs differ; decode() wraps back)
    np.savez_compressed(out, delta=delta, sha_a=sha(a.numpy()), sha_b=sha(b.numpy()), sha_c=sha(bits))
    z = np.load(out)
    assert np.array_equal(decode(z, a, b), bits)
    print(f"{out}: {os.path.getsize(out)} bytes, median |delta| {int(np.median(np.abs(delta)))} ulp")
