"""The persistent bf16x3 weight-gradient panel kernel (wgrad_panel_bf3_kernel, tile 7: C[M, N] = alpha A[K, M]^T . B[K, N] for
K, M <= 128 and N >= 2048) over the shapes it admits: single rows, ragged row blocks, a ragged last panel, fewer panels than
workgroups, panel counts the grid does not divide, one to three turns per workgroup.  Every case is held against a float64
product of the same fp32 operands under the bound of test_gemm_bf16x3_weight_gradient_panels, which is READ from that test's
source (an absolute part, and a part relative to the fp32 MFMA path's own error measured beside it); one case is held bit for bit
against an output recorded from the kernel as it was before its C tiles were stored write-through."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def bound():
    """(absolute, factor on the fp32 path's error, slack) of `assert e1 < A and e1 < F * e0 + S` in the panel test."""
    from tests import test_kernels_gpu as T
    src = inspect.getsource(T.test_gemm_bf16x3_weight_gradient_panels)
    m = re.search(r"assert e1 < ([0-9.e+-]+) and e1 < ([0-9.e+-]+) \* e0 \+ ([0-9.e+-]+),", src)
    assert m, "the bound of test_gemm_bf16x3_weight_gradient_panels was not found in its source"
    return tuple(float(g) for g in m.groups())


@functools.lru_cache(maxsize=None)
def problem(K, M, N):
    """Seeded operands (as in test_gemm_bf16x3_weight_gradient_panels), the float64 product and its scale; shared, never modified."""
    a = torch.randn(K, M, generator=torch.Generator().manual_seed(K + M)) * 0.05
    b = torch.rand(K, N, generator=torch.Generator().manual_seed(N))          # depth-like inputs in [0, 1)
    want = a.double().t() @ b.double()
    return a, b, want, float(want.abs().max())


def check(ops, K, M, N, alpha=1.0):
    from r3d_amd._lib import GEMM_TN
    a, b, want, scale = problem(K, M, N)
    ad, bd = a.cuda(), b.cuda()
    c1, c0 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    ws = ops.GemmWorkspace("cuda")
    d1 = ops.gemm(GEMM_TN, ad, bd, c1, ws=ws, prec=1, alpha=alpha)
    d0 = ops.gemm(GEMM_TN, ad, bd, c0, ws=ws, prec=0, alpha=alpha)
    torch.cuda.synchronize()
    assert d1.tile == 7 and d0.tile == 6, (d1.tile, d0.tile)
    e1 = float((c1.cpu().double() - alpha * want).abs().max()) / (abs(alpha) * scale)
    e0 = float((c0.cpu().double() - alpha * want).abs().max()) / (abs(alpha) * scale)
    A, F, S = bound()
    print(f"K {K} M {M} N {N} alpha {alpha}: bf16x3 {e1:.3e} fp32 {e0:.3e} (bound {A:g}, {F:g} e0 + {S:g})")
    assert e1 < A and e1 < F * e0 + S, (e1, e0)


@pytest.mark.parametrize("M", [1, 33, 128])
@pytest.mark.parametrize("K", [1, 17, 128])
def test_wgrad_panel_rows_and_depths(ops, K, M):
    """Every K x M corner at an N with a ragged last panel (2052 = 32 panels + 4 columns, one turn per workgroup)."""
    check(ops, K, M, 2052)


# 2048: the smallest N the kernel admits; 2052 and 2244: a ragged last panel, fewer panels than workgroups; 64 * 257: two turns and
# a panel count the grid does not divide (129 workgroups, the last with one turn); 64 * 513 + 4: three turns, the accumulator sets
# alternate twice, and a ragged last panel
@pytest.mark.parametrize("N", [2048, 2052, 2048 + 64 * 3 + 4, 64 * 257, 64 * 513 + 4])
@pytest.mark.parametrize("K,M", [(128, 128), (17, 33)])
def test_wgrad_panel_widths(ops, K, M, N):
    check(ops, K, M, N)


def test_wgrad_panel_alpha(ops):
    check(ops, 128, 128, 64 * 257, alpha=-0.375)


@pytest.mark.parametrize("K,M,N", [(128, 128, 2052), (17, 33, 64 * 257), (128, 100, 64 * 257 + 8)])
def test_wgrad_panel_leaves_the_rest_of_c_alone(ops, K, M, N):
    """C is a window of a larger, pre-poisoned allocation: rows past M and columns past N keep every bit."""
    from r3d_amd._lib import GEMM_TN
    a, b, want, scale = problem(K, M, N)
    mark = 0x7FC12345                                                          # a NaN with a payload
    poison = torch.full((M + 5, N + 72), mark, dtype=torch.int32, device="cuda").view(torch.float32)
    d = ops.gemm(GEMM_TN, a.cuda(), b.cuda(), poison[:M, :N], ws=ops.GemmWorkspace("cuda"), prec=1)
    torch.cuda.synchronize()
    assert d.tile == 7
    got = poison.cpu()
    bits = got.view(torch.int32)
    assert bool((bits[M:] == mark).all()) and bool((bits[:, N:] == mark).all())
    A, _, _ = bound()
    assert float((got[:M, :N].double() - want).abs().max()) / scale < A


def test_wgrad_panel_matches_the_recorded_output_bit_for_bit(ops):
    """Seeded (K, M, N) = (128, 128, 2112) against the output recorded on the GPU from the kernel before this file existed
    (tests/golden/make_golden_wgrad_panel.py)."""
    from r3d_amd._lib import GEMM_TN
    from tests.golden import make_golden_wgrad_panel as G
    a, b = G.operands()
    want = G.decode(np.load(os.path.join(GOLDEN, "wgrad_panel_128x128x2112.npz")), a, b)
    c = torch.empty(G.M, G.N, device="cuda")
    d = ops.gemm(GEMM_TN, a.cuda(), b.cuda(), c, ws=ops.GemmWorkspace("cuda"), prec=1)
    torch.cuda.synchronize()
    assert d.tile == 7
    got = c.cpu().numpy().view(np.int32)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} elements differ"
