"""The bf16x3 GEMM kernels (csrc/gemm_bf3.hip: wgrad_panel_bf3_kernel, gemm_bf3_nt_kernel at both tile sizes,
gemm_bf3_nt_u_kernel, gemm_bf3_tn_kernel with one and two LDS stages, and the pair launch) over tests/gemm_bf3_cases.py.

General rows: every launch against the float64 product of the same fp32 operands under the componentwise metric and the
bound of gemm_bf3_cases (8 * e32 + 2^-21, e32 the error of a float32 CPU matmul).  Outputs and split-K slabs live in
larger allocations filled with a payload NaN: nothing inside may keep it (a tile that was skipped), everything outside keeps
its bits, operand padding is NaN (a load past a row's end shows), and a second launch gives the same bits.
Exactness rows: products that have no rounding at all, held bit for bit (-0 = +0) on every kernel, tile 7 included.
The AdamW epilogue of tiles 10 and 12: two steps against a float64 AdamW fed the gradient the same tile stores.
The pair launch: both products' slab sums under the bound, the same bits as two separate launches, the C entry's refusals,
the wrapper's ways of returning None.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_bf3_cases as G  # noqa: E402
from tests import loss_optim_oracle as R  # noqa: E402
from tests.helpers import assert_close  # noqa: E402

FIGURES = []              # (case, mode, E, e32, bound)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    yield o
    print("\n[gemm_bf3] case, mode: E(kernel), e32, bound = 8 e32 + 2^-21")
    for what, mode, e, e32, bound in FIGURES:
        print(f"[gemm_bf3]   {what:<44s} {mode:<14s} E {e:.3e}  e32 {e32:.3e}  bound {bound:.3e}  ({e / bound:5.3f})")


def poisoned(*shape):
    return torch.full(shape, G.POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def is_poison(t):
    return t.view(torch.int32) == G.POISON


def place(x, pad=0, off=0):
    """x on the device as a view of leading dimension columns + pad that starts `off` floats into an allocation of NaN"""
    rows, cols = x.shape
    buf = torch.full((off + rows * (cols + pad),), float("nan"), device="cuda")
    v = buf[off:].view(rows, cols + pad)[:, :cols]
    v.copy_(x)
    assert v.data_ptr() % 16 == 0
    return v


def slab_ws(ops, nfloats, extra=192):
    """a workspace whose buffer is `extra` floats larger than the slabs and poisoned throughout"""
    ws = ops.GemmWorkspace("cuda")
    ws.buf = poisoned(nfloats + extra)
    return ws


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: a second launch gave other bits"


def held(what, mode, X, ref, S, p):
    """E(X) of the module docstring against the case's bound, after refusing NaN; the figures are printed at the end"""
    X = X.double().cpu()
    nnan = int(torch.isnan(X).sum())
    assert nnan == 0, f"{what} {mode}: {nnan}/{X.numel()} elements are NaN (never written, or padding was read)"
    e = float(((X - ref).abs() / S).max())
    FIGURES.append((what, mode, e, p.e32, p.bound))
    print(f"{what} {mode}: E {e:.3e} e32 {p.e32:.3e} bound {p.bound:.3e}")
    assert e <= p.bound, f"{what} {mode}: E {e:.3e} > bound {p.bound:.3e} (e32 {p.e32:.3e})"


# ----------------------------------------------------------------------------------------------------------
# a. NT tiles 8, 9, 11
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.NT_CASES, ids=G.case_id)
def test_nt_case(ops, c):
    p = G.case_problem(c)
    M, N, K = c.M, c.N, c.K
    ns, kps = G.nt_split(c.tile, K, c.splitk)
    Ad, Bd = place(p.A, c.pad, c.off), place(p.B, c.pad, c.off)
    what = G.case_id(c)
    # raw slabs
    runs = []
    for _ in range(2):
        ws = slab_ws(ops, ns * M * N)
        d = ops.gemm(G.NT, Ad, Bd, torch.empty(M, N, device="cuda"), prec=1, tile=c.tile, splitk=c.splitk, defer_reduce=True, ws=ws)
        torch.cuda.synchronize()
        assert (d.tile, d.splitk, d.k_per_split) == (c.tile, ns, kps)
        runs.append(ws.buf)
    slabs = runs[0][:ns * M * N].view(ns, M, N)
    assert bool(is_poison(runs[0][ns * M * N:]).all()), f"{what}: written past the slabs"
    held(what, "slab sum", slabs.double().sum(0), p.ref, p.S, p)
    same_bits(runs[0], runs[1], what + " slabs")
    # the reducer with bias + ReLU into a window of a wider C
    bias = G.bias_of(N, K + N)
    pre, S = p.ref + bias.double(), p.S + bias.double().abs()
    ws = ops.GemmWorkspace("cuda")
    runs = []
    for _ in range(2):
        Cw = poisoned(M + 3, N + 8)
        ops.gemm(G.NT, Ad, Bd, Cw[:M, :N], prec=1, tile=c.tile, splitk=c.splitk, ws=ws, bias=bias.cuda(), act=1)
        torch.cuda.synchronize()
        runs.append(Cw)
    Cw = runs[0]
    assert bool(is_poison(Cw[M:]).all()) and bool(is_poison(Cw[:, N:]).all()), f"{what}: written outside the window of C"
    X = Cw[:M, :N].double().cpu()
    near = pre.abs() <= p.bound * S                       # the ReLU's kink: either side is right there
    assert bool((X[near].abs() <= 2 * p.bound * S[near]).all())
    held(what, "bias + ReLU", torch.where(near, pre.relu(), X), pre.relu(), S, p)
    same_bits(runs[0], runs[1], what + " C")


# ----------------------------------------------------------------------------------------------------------
# b. TN tiles 10, 12
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.TN_CASES, ids=G.case_id)
def test_tn_case(ops, c):
    p = G.case_problem(c)
    M, N, K = c.M, c.N, c.K
    Ad, Bd = place(p.A, c.pad, 4 * c.pad), place(p.B, c.pad, 4 * c.pad)
    c0 = G.operand(M, N, "randn", 9)
    what = G.case_id(c)
    for acc in (False, True):
        runs = []
        for _ in range(2):
            Cw = poisoned(M + 3, N + G.TN_LDC_PAD)
            if acc:
                Cw[:M, :N] = c0.cuda()
            d = ops.gemm(G.TN, Ad, Bd, Cw[:M, :N], prec=1, tile=c.tile, splitk=1, alpha=G.TN_ALPHA, accumulate=acc)
            torch.cuda.synchronize()
            assert (d.tile, d.splitk) == (c.tile, 1)
            runs.append(Cw)
        Cw = runs[0]
        assert bool(is_poison(Cw[M:]).all()) and bool(is_poison(Cw[:, N:]).all()), f"{what}: written outside the window of C"
        ref = G.TN_ALPHA * p.ref + (c0.double() if acc else 0.0)
        S = abs(G.TN_ALPHA) * p.S + (c0.double().abs() if acc else 0.0)
        held(what, "accumulate" if acc else "alpha", Cw[:M, :N], ref, S, p)
        same_bits(runs[0], runs[1], what)


# ----------------------------------------------------------------------------------------------------------
# c. the AdamW epilogue of tiles 10, 12
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.ADAM_CASES, ids=G.case_id)
def test_adamw_epilogue(ops, c):
    """Two steps with parameter and moments as windows of poisoned [M + 3, N + 8] buffers, against
    loss_optim_oracle.adamw64 at the tolerances of test_gemm_bf16x3_weight_gradient_tiled_with_adamw_epilogue.  As in the fp32
    pin (test_gemm_f32_gpu.run_adam) the float64 update starts from the float32 gradient the same tile stores -- itself held
    to the product's bound here: the tolerances are those of the update's arithmetic."""
    K, M, N = c.K, c.M, c.N
    hp = G.ADAM
    p = G.problem(G.TN, M, N, K, "randn", 77 + K)
    Ad, Bd = place(p.A), place(p.B)
    gen = torch.Generator().manual_seed(5)
    p0, m0 = torch.randn(M, N, generator=gen) * 0.1, torch.randn(M, N, generator=gen) * 1e-3
    v0 = torch.rand(M, N, generator=gen) * 1e-4
    lr_t = torch.full((1,), hp["lr"], dtype=torch.float32, device="cuda")
    f32 = lambda x: float(np.float32(x))      # noqa: E731  (the hyper-parameters cross the C ABI as float32)
    what = G.case_id(c)

    def two_steps(compare):
        step_t = torch.zeros(1, dtype=torch.int64, device="cuda")
        wide = [poisoned(M + 3, N + G.TN_LDC_PAD) for _ in range(3)]
        for w, x in zip(wide, (p0, m0, v0)):
            w[:M, :N] = x.cuda()
        g = poisoned(M, N)
        for step in (1, 2):
            ops.tick(step_t, None)
            before = [w[:M, :N].cpu().numpy().astype(np.float64) for w in wide]
            d = ops.gemm(G.TN, Ad, Bd, wide[0][:M, :N], prec=1, tile=c.tile, alpha=hp["alpha"],
                         adam=dict(m=wide[1][:M, :N], v=wide[2][:M, :N], lr_t=lr_t, step_t=step_t, beta1=hp["beta1"],
                                   beta2=hp["beta2"], eps=hp["eps"], weight_decay=hp["weight_decay"], grad_scale=hp["grad_scale"]))
            assert (d.tile, d.splitk) == (c.tile, 1)
            if not compare:
                continue
            ops.gemm(G.TN, Ad, Bd, g, prec=1, tile=c.tile, splitk=1, alpha=hp["alpha"])
            torch.cuda.synchronize()
            if step == 1:
                held(what, "gradient", g, hp["alpha"] * p.ref, hp["alpha"] * p.S, p)
            ref = R.adamw64(before[0], g.cpu().numpy(), before[1], before[2], step, f32(hp["lr"]), f32(hp["weight_decay"]),
                            f32(hp["beta1"]), f32(hp["beta2"]), f32(hp["eps"]), grad_scale=hp["grad_scale"])
            for name, w, r in (("parameter", wide[0], ref[0]), ("exp_avg", wide[1], ref[1]), ("exp_avg_sq", wide[2], ref[2])):
                got = w[:M, :N].cpu().double()
                assert not bool(torch.isnan(got).any()), f"{what} step {step} {name}: not written"
                rtol, atol = G.ADAM_TOL[name]
                assert_close(got, torch.from_numpy(r), rtol, atol, f"{what} step {step} {name} vs float64")
        torch.cuda.synchronize()
        return wide
    first, second = two_steps(True), two_steps(False)
    for name, w, u in zip(("parameter", "exp_avg", "exp_avg_sq"), first, second):
        assert bool(is_poison(w[M:]).all()) and bool(is_poison(w[:, N:]).all()), f"{what}: written outside the {name} window"
        same_bits(w, u, f"{what} {name}")


# ----------------------------------------------------------------------------------------------------------
# d. the pair launch
# ----------------------------------------------------------------------------------------------------------
def pair_operands(c):
    p1, p2, _ = G.pair_problems(c)
    return p1, p2, (place(p1.A), place(p1.B), place(p2.A, c.pad2, 4), place(p2.B, c.pad2 + 4, 8))


@pytest.mark.parametrize("c", G.PAIR_CASES, ids=G.case_id)
def test_pair(ops, c):
    M, N = c.M, c.N
    p1, p2, (a1, b1, a2, b2) = pair_operands(c)
    _, ns1, kps1 = G.plan_nt(M, N, c.K1)
    ns2, kps2 = G.pair_split(c.K2, ns1, kps1)
    what = G.case_id(c)
    cd = torch.empty(M, N, device="cuda")
    runs = []
    for _ in range(2):
        ws1, ws2 = slab_ws(ops, ns1 * M * N), slab_ws(ops, ns2 * M * N)
        r = ops.gemm_bf3_nt_pair(a1, b1, cd, ws1, a2, b2, cd, ws2)
        torch.cuda.synchronize()
        assert r is not None, f"{what}: the wrapper refused the pair"
        d1, d2 = r
        assert (d1.tile, d1.splitk, d1.k_per_split) == (8, ns1, kps1) and (d2.tile, d2.splitk, d2.k_per_split) == (8, ns2, kps2)
        assert (d2.lda, d2.ldb) == (c.K2 + c.pad2, c.K2 + c.pad2 + 4)
        runs.append((ws1.buf, ws2.buf))
    for buf, ns, p, which in ((runs[0][0], ns1, p1, "first"), (runs[0][1], ns2, p2, "second")):
        assert bool(is_poison(buf[ns * M * N:]).all()), f"{what}: written past the {which} product's slabs"
        held(what, which + " slab sum", buf[:ns * M * N].view(ns, M, N).double().sum(0), p.ref, p.S, p)
    same_bits(runs[0][0], runs[1][0], what + " first")
    same_bits(runs[0][1], runs[1][1], what + " second")
    # the same two products launched separately with the same splits
    ws1, ws2 = slab_ws(ops, ns1 * M * N), slab_ws(ops, ns2 * M * N)
    e1 = ops.gemm(G.NT, a1, b1, cd, prec=1, defer_reduce=True, ws=ws1)
    e2 = ops.gemm(G.NT, a2, b2, cd, prec=1, tile=8, splitk=-ns1 % 8, defer_reduce=True, ws=ws2)
    torch.cuda.synchronize()
    assert (e1.tile, e1.splitk, e1.k_per_split) == (8, ns1, kps1) and (e2.tile, e2.splitk, e2.k_per_split) == (8, ns2, kps2)
    assert torch.equal(ws1.buf.view(torch.int32), runs[0][0].view(torch.int32)), f"{what}: first product, pair vs single launch"
    assert torch.equal(ws2.buf.view(torch.int32), runs[0][1].view(torch.int32)), f"{what}: second product, pair vs single launch"


def pair_descs(ops, a1, b1, a2, b2, cd, K2_kps):
    from r3d_amd import _lib
    lib = _lib.load()
    d1, d2 = _lib.GemmDesc(), _lib.GemmDesc()
    M, N, _ = ops._fill_desc(d1, G.NT, a1, b1, cd, prec=1)
    _, _, K2 = ops._fill_desc(d2, G.NT, a2, b2, cd, prec=1)
    assert lib.r3d_gemm_plan(C.byref(d1)) == 0 and d1.tile == 8
    d2.tile, d2.k_per_split, d2.splitk = 8, K2_kps, G.cdiv(K2, K2_kps)
    return lib, d1, d2


@pytest.mark.parametrize("row", G.PAIR_DIRECT, ids=lambda r: f"{r[2]}+{r[3]}")
def test_pair_direct(ops, row):
    """r3d_gemm_bf3_nt_pair itself, with splits the wrapper does not make"""
    M, N, K1, K2, kps2, what = row
    (p1, _, _, _), (p2, _, _, _) = G.pair_direct_problems(row)
    a1, b1, a2, b2 = place(p1.A), place(p1.B), place(p2.A, 4, 4), place(p2.B, 8, 8)
    cd = torch.empty(M, N, device="cuda")
    lib, d1, d2 = pair_descs(ops, a1, b1, a2, b2, cd, kps2)
    assert d1.splitk == G.plan_nt(M, N, K1)[1]
    bufs = poisoned(d1.splitk * M * N + 64), poisoned(d2.splitk * M * N + 64)
    d1.partial, d2.partial = bufs[0].data_ptr(), bufs[1].data_ptr()
    assert lib.r3d_gemm_bf3_nt_pair(C.byref(d1), C.byref(d2), ops._stream()) == 0
    torch.cuda.synchronize()
    for buf, d, p, which in ((bufs[0], d1, p1, "first"), (bufs[1], d2, p2, "second")):
        n = d.splitk * M * N
        assert bool(is_poison(buf[n:]).all()), f"{what}: written past the {which} product's slabs"
        held(f"pair-direct-{K1}+{K2}", which + " slab sum", buf[:n].view(d.splitk, M, N).double().sum(0), p.ref, p.S, p)


def test_pair_refusals(ops):
    """R3D_EINVAL and nothing launched: both slab buffers keep every bit"""
    from r3d_amd import _lib
    M, N, K1, K2 = 8, 40, 8200, 136
    a1, b1 = place(G.operand(M, K1, "randn", 1)), place(G.operand(N, K1, "randn", 2))
    a2, b2 = place(G.operand(M, K2, "randn", 3)), place(G.operand(N, K2, "randn", 4))
    cd = torch.empty(M, N, device="cuda")
    bufs = poisoned(64 * M * N), poisoned(64 * M * N)
    add = place(G.operand(8, K2, "randn", 5))

    def call(change):
        lib, d1, d2 = pair_descs(ops, a1, b1, a2, b2, cd, 64)
        d1.partial, d2.partial = bufs[0].data_ptr(), bufs[1].data_ptr()
        change(d1, d2)
        rc = lib.r3d_gemm_bf3_nt_pair(C.byref(d1), C.byref(d2), ops._stream())
        torch.cuda.synchronize()
        return rc

    def set_(which, **kw):
        def change(d1, d2):
            for k, v in kw.items():
                setattr((d1, d2)[which], k, v)
        return change
    refused = {"M mismatch": set_(1, M=M - 1), "N mismatch": set_(1, N=N - 1), "shared partial": set_(1, partial=bufs[0].data_ptr()),
               "first tile": set_(0, tile=9), "second tile": set_(1, tile=9), "first alpha": set_(0, alpha=0.5),
               "second alpha": set_(1, alpha=0.5), "second a_add": set_(1, a_add=add.data_ptr(), a_add_mod=8, a_add_ld=K2)}
    for name, change in refused.items():
        assert call(change) == _lib.EINVAL, name
        assert bool(is_poison(bufs[0]).all()) and bool(is_poison(bufs[1]).all()), f"{name}: something was launched"
    assert call(lambda d1, d2: None) == 0 and not bool(is_poison(bufs[0][:M * N]).any())      # (the unchanged pair is taken)


def test_pair_wrapper_returns_none(ops):
    M, N = 8, 40
    cd = torch.empty(M, N, device="cuda")

    def refused(K1, a2, b2, c2=cd):
        a1, b1 = torch.zeros(M, K1, device="cuda"), torch.zeros(N, K1, device="cuda")
        ws1, ws2 = ops.GemmWorkspace("cuda"), ops.GemmWorkspace("cuda")
        ws1.buf, ws2.buf = poisoned(256), poisoned(256)
        keep = ws1.buf, ws2.buf
        r = ops.gemm_bf3_nt_pair(a1, b1, cd, ws1, a2, b2, c2, ws2)
        torch.cuda.synchronize()
        assert r is None
        assert ws1.buf is keep[0] and ws2.buf is keep[1] and bool(is_poison(keep[0]).all()) and bool(is_poison(keep[1]).all())
    z = lambda r, k, pad=0, off=0: place(torch.zeros(r, k), pad, off)      # noqa: E731
    for K1, K2, why in G.PAIR_NONE:
        refused(K1, z(M, K2), z(N, K2))
    refused(8200, z(M, 136), torch.zeros(4 + N * 136, device="cuda")[2:2 + N * 136].view(N, 136))      # B 8 bytes off
    refused(8200, z(M, 136, 2), z(N, 136))                                  # a row stride off a multiple of 4
    refused(8200, z(M, 136), z(N + 1, 136), torch.empty(M, N + 1, device="cuda"))   # another N


# ----------------------------------------------------------------------------------------------------------
# exactness
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.EXACT_CASES, ids=G.case_id)
def test_exact(ops, c):
    A, B, want = G.exact_operands(c)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    Cd = poisoned(c.M, c.N)
    ws = ops.GemmWorkspace("cuda")
    if c.tile in G.NT_TILES:
        d = ops.gemm(G.NT, Ad, Bd, Cd, prec=1, tile=c.tile, splitk=c.splitk, ws=ws)
    elif c.tile == 7:
        d = ops.gemm(G.TN, Ad, Bd, Cd, prec=1, ws=ws)
    else:
        d = ops.gemm(G.TN, Ad, Bd, Cd, prec=1, tile=c.tile, splitk=1)
    torch.cuda.synchronize()
    assert d.tile == c.tile
    got = Cd.cpu().numpy().astype(np.float64)
    bad = got != want                                     # (-0 == +0; a NaN differs from everything)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        ulp = np.abs(got[bad] - want[bad]) / np.spacing(np.abs(want[bad]).astype(np.float32)).astype(np.float64)
        raise AssertionError(f"{G.case_id(c)}: {int(bad.sum())} of {bad.size} elements differ, by up to {float(np.nanmax(ulp)):.3g} ulp; "
                             f"first at {i}: got {got[i]!r} want {want[i]!r}")
