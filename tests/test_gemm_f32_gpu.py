"""gemm_f32_kernel, gemm_grouped_kernel and splitk_reduce_kernel (csrc/gemm_f32.hip) over tests/gemm_f32_cases.py: the
k-split-wave tiles 4 and 5, the epilogue of tiles 2..5, the XCD placement modes, the AdamW epilogue of the fp32 tiles and
the grouped launches the engine makes.  Every launch is compared with a float64 CPU evaluation of the same operation at
the tolerances tests/test_kernels_gpu.py uses for this kernel (products and bias_grad: rtol 1e-4, atol 1e-4 sqrt(K);
epilogues: 1e-4, 1e-4).  Outputs start as NaN in buffers wider than N: nothing inside may stay NaN (a tile that was
skipped), the columns past N must stay NaN (a tile that was misplaced), and a second launch must give the same bits (the
kernels have no atomics).  Needs an MI355X."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import gemm_f32_cases as G  # noqa: E402
from tests import loss_optim_oracle as R  # noqa: E402
from tests.helpers import assert_close  # noqa: E402

NAN = float("nan")
C_PAD = 5                 # C and pre_out live in [M, N + 5] buffers, bias_grad in an [M + 3] one
WORST = {}                # group -> (worst error / tolerance, max abs error there, what)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    yield o
    print("\n[gemm_f32] worst error as a fraction of the tolerance, per group")
    for g in sorted(WORST):
        ratio, err, what = WORST[g]
        print(f"[gemm_f32]   {g:<24s} {ratio:6.3f}  (abs err {err:.3e}: {what})")


@pytest.fixture(scope="module")
def ws(ops):
    return ops.GemmWorkspace("cuda")


def dev(t):
    return t.to("cuda")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def nan_wide(rows, cols, extra=C_PAD, init=None):
    t = torch.full((rows, cols + extra), NAN, device="cuda")
    if init is not None:
        t[:, :cols] = dev(init)
    return t


def check(group, got, ref, rtol, atol, what):
    """assert_close, after refusing NaN and noting the worst error / tolerance of the group"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    nnan = int(torch.isnan(got).sum())
    assert nnan == 0, f"{what}: {nnan}/{got.numel()} elements were never written"
    err = (got - ref).abs()
    ratio = err / (atol + rtol * ref.abs())
    i = int(ratio.argmax())
    if group not in WORST or float(ratio.reshape(-1)[i]) > WORST[group][0]:
        WORST[group] = (float(ratio.reshape(-1)[i]), float(err.reshape(-1)[i]), what)
    assert_close(got, ref, rtol, atol, what)


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: a second launch gave other bits"


def tail_is_nan(t, cols, what):
    assert bool(torch.isnan(t[..., cols:]).all()), f"{what}: written past column {cols}"


def operands(layout, M, N, K, pad, seed, scale_a=1.0):
    """(A, B) device views with leading dimension = columns + pad, and their float32 host values"""
    sa = (M, K) if layout in (G.NT, G.NN) else (K, M)
    sb = (N, K) if layout == G.NT else (K, N)
    A, B = rnd(sa[0], sa[1] + pad, seed=seed, scale=scale_a), rnd(sb[0], sb[1] + pad, seed=seed + 1)
    return dev(A)[:, :sa[1]], dev(B)[:, :sb[1]], A[:, :sa[1]], B[:, :sb[1]]


def product(layout, A, B):
    A, B = A.double(), B.double()
    return A @ B.t() if layout == G.NT else (A @ B if layout == G.NN else A.t() @ B)


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


class Epilogue:
    """Operands of a set of epilogue / prologue names (host float32 values and device views of wider buffers), the
    keywords ops.gemm takes for them, and the float64 evaluation in the order of test_gemm_epilogue_and_prologue."""

    def __init__(self, layout, M, N, K, names, seed, pad=0, c0=None):
        self.layout, self.M, self.N, self.K, self.names = layout, M, N, K, set(names)
        self.h, self.kw = {}, {}
        self.c0 = c0

        def mat(name, rows, cols, extra, sd):
            x = rnd(rows, cols + extra, seed=seed + sd)
            self.h[name] = x[:, :cols]
            return dev(x)[:, :cols]
        n = self.names
        if "a_add" in n:
            self.kw.update(a_add=mat("a_add", G.ADD_MOD, K, pad, 11), a_add_mod=G.ADD_MOD)
        if "a_row_xor" in n:
            self.kw.update(a_row_xor=1)
        if "b_add" in n:
            self.kw.update(b_add=mat("b_add", G.ADD_MOD, N, pad, 12), b_add_mod=G.ADD_MOD)
        if "bias" in n:
            self.h["bias"] = rnd(N, seed=seed + 13)
            self.kw.update(bias=dev(self.h["bias"]))
        if "drop" in n:
            m = (torch.rand(M, N + 3, generator=torch.Generator().manual_seed(seed + 14)) > 0.3).to(torch.uint8)
            self.h["drop"] = m[:, :N]
            self.kw.update(drop_mask=dev(m)[:, :N], drop_scale=1.25)
        if "aux" in n:
            self.kw.update(aux=mat("aux", M, N, 8, 15))
        if "res1" in n:
            self.kw.update(res1=mat("res1", M, N, 4, 16))
        if "res2" in n:
            self.kw.update(res2=mat("res2", M, N, 0, 17))
        if "alpha" in n:
            self.kw.update(alpha=0.5)
        if "c_row_xor" in n:
            self.kw.update(c_row_xor=1)
        if "act2" in n:
            self.kw.update(act=2)
        if "mul2" in n:
            self.kw.update(mul=2)

    def reference(self, A, B, act=None, mul=None):
        """(pre_out, C) in float64; act / mul override the names (the epilogue cases loop over them)"""
        h, n = self.h, self.names
        A, B = A.double(), B.double()
        rows = torch.arange(self.M)
        if "a_row_xor" in n:
            A = A[rows ^ 1]
        if "a_add" in n:
            A = A + h["a_add"].double()[rows % G.ADD_MOD]
        if "b_add" in n:
            B = B + h["b_add"].double()[torch.arange(self.K) % G.ADD_MOD]
        v = product(self.layout, A, B)
        if "c_row_xor" in n:
            v = v[rows ^ 1]                                  # row m of the product lands in row m ^ 1
        v = (0.5 if "alpha" in n else 1.0) * v
        if "bias" in n:
            v = v + h["bias"].double()
        pre = v.clone()
        act = (2 if "act2" in n else 0) if act is None else act
        mul = (2 if "mul2" in n else 0) if mul is None else mul
        if act == 1:
            v = v.relu()
        elif act == 2:
            v = F.gelu(v)
        if "drop" in n:
            v = v * 1.25 * h["drop"].double()
        if mul == 1:
            v = v * (h["aux"] > 0).double()
        elif mul == 2:
            v = v * gelu_grad(h["aux"].double())
        if "res1" in n:
            v = v + h["res1"].double()
        if "res2" in n:
            v = v + h["res2"].double()
        if self.c0 is not None:
            v = v + self.c0.double()
        return pre, v


def launched_as_planned(c, d):
    assert d.tile == c.tile and d.splitk == G.nsplits(c.K, c.splitk), (d.tile, d.splitk)


# ----------------------------------------------------------------------------------------------------------
# plain products: tiles 4 and 5, the grid modes
# ----------------------------------------------------------------------------------------------------------
def run_raw(ops, ws, c):
    M, N, K = c.M, c.N, c.K
    Ad, Bd, A, B = operands(c.layout, M, N, K, c.pad, seed=M + N + K + c.layout)
    out = []
    for _ in range(2):
        Cw = nan_wide(M, N)
        d = ops.gemm(c.layout, Ad, Bd, Cw[:, :N], tile=c.tile, splitk=c.splitk, ws=ws)
        torch.cuda.synchronize()
        out.append(Cw)
    launched_as_planned(c, d)
    what = G.case_id(c)
    mode = G.case_mode(c)[0]
    tail_is_nan(out[0], N, what)
    check(f"{c.tag} tile {c.tile} mode {mode}", out[0][:, :N], product(c.layout, A, B), 1e-4, 1e-4 * math.sqrt(K), what)
    same_bits(out[0], out[1], what)


def run_bias_grad(ops, ws, c):
    M, N, K = c.M, c.N, c.K
    Ad, Bd, A, B = operands(c.layout, M, N, K, c.pad, seed=M + N + K)
    ep = Epilogue(c.layout, M, N, K, c.epi, seed=K, pad=c.pad)
    out = []
    for _ in range(2):
        Cw, db = nan_wide(M, N), torch.full((M + 3,), NAN, device="cuda")
        d = ops.gemm(c.layout, Ad, Bd, Cw[:, :N], bias_grad=db[:M], tile=c.tile, ws=ws, **ep.kw)
        torch.cuda.synchronize()
        out.append((Cw, db))
    launched_as_planned(c, d)
    what = G.case_id(c)
    tail_is_nan(out[0][0], N, what)
    tail_is_nan(out[0][1], M, what + " bias_grad")
    check(f"db tile {c.tile} dW", out[0][0][:, :N], ep.reference(A, B)[1], 1e-4, 1e-4 * math.sqrt(K), what + " dW")
    check(f"db tile {c.tile} db", out[0][1][:M], A.double().sum(0), 1e-4, 1e-4 * math.sqrt(K), what + " bias_grad")
    same_bits(out[0][0], out[1][0], what)
    same_bits(out[0][1], out[1][1], what + " bias_grad")


# ----------------------------------------------------------------------------------------------------------
# epilogues
# ----------------------------------------------------------------------------------------------------------
def run_epi(ops, ws, c):
    M, N, K = c.M, c.N, c.K
    Ad, Bd, A, B = operands(c.layout, M, N, K, c.pad, seed=1 + M + c.tile)
    c0 = rnd(M, N, seed=9)
    ep = Epilogue(c.layout, M, N, K, G.EPI_FULL | c.epi, seed=100 + c.tile, pad=c.pad, c0=c0)
    plain = Epilogue(c.layout, M, N, K, (G.EPI_FULL | c.epi) - {"accumulate"}, seed=100 + c.tile, pad=c.pad)
    group = f"epi tile {c.tile} sk{c.splitk}"
    combos = [(act, mul, True) for act in (0, 1, 2) for mul in (0, 1, 2)] + [(2, 2, False)]
    for act, mul, acc in combos:
        e = ep if acc else plain
        what = f"{G.case_id(c)} act{act} mul{mul} acc{int(acc)}"
        out = []
        for _ in range(2):
            Cw, pre = nan_wide(M, N, init=c0 if acc else None), nan_wide(M, N, extra=7)
            d = ops.gemm(c.layout, Ad, Bd, Cw[:, :N], pre_out=pre[:, :N], act=act, mul=mul, accumulate=acc, tile=c.tile,
                         splitk=c.splitk, ws=ws, **e.kw)
            torch.cuda.synchronize()
            out.append((Cw, pre))
        launched_as_planned(c, d)
        ref_pre, ref_c = e.reference(A, B, act=act, mul=mul)
        tail_is_nan(out[0][0], N, what)
        tail_is_nan(out[0][1], N, what + " pre_out")
        check(group, out[0][1][:, :N], ref_pre, 1e-4, 1e-4, what + " pre_out")
        check(group, out[0][0][:, :N], ref_c, 1e-4, 1e-4, what)
        same_bits(out[0][0], out[1][0], what)
        same_bits(out[0][1], out[1][1], what + " pre_out")


def run_xor(ops, ws, c):
    M, N, K = c.M, c.N, c.K
    Ad, Bd, A, B = operands(c.layout, M, N, K, c.pad, seed=2 + M + c.tile)
    ep = Epilogue(c.layout, M, N, K, {"res1", "c_row_xor"}, seed=3)
    out = []
    for _ in range(2):
        Cw = nan_wide(M, N)
        d = ops.gemm(c.layout, Ad, Bd, Cw[:, :N], tile=c.tile, splitk=c.splitk, ws=ws, **ep.kw)
        torch.cuda.synchronize()
        out.append(Cw)
    launched_as_planned(c, d)
    what = G.case_id(c)
    tail_is_nan(out[0], N, what)
    check(f"xor tile {c.tile}", out[0][:, :N], ep.reference(A, B)[1], 1e-4, 1e-4, what)
    same_bits(out[0], out[1], what)


# ----------------------------------------------------------------------------------------------------------
# AdamW epilogue
# ----------------------------------------------------------------------------------------------------------
def run_adam(ops, ws, c):
    """Two steps of the product with the AdamW epilogue on parameter / moment blocks of wider buffers, against (1) the
    same tile's stored gradient followed by r3d_adamw_flat, at the margins of
    test_gemm_bf16x3_weight_gradient_tiled_with_adamw_epilogue, and (2) loss_optim_oracle.adamw64 at the margins
    test_loss_optim_gpu.py has for r3d_adamw_flat.  As there, the float64 update starts from the float32 gradient the
    kernel stored (here: the same tile's, itself compared with the float64 product at the product tolerance): the
    margins are those of the update's arithmetic, and an fp32 dot product does not reach them on elements that cancel."""
    M, N, K, L = c.M, c.N, c.K, c.layout
    hp = G.ADAM
    Ad, Bd, A, B = operands(L, M, N, K, 0, seed=K + M, scale_a=0.05)
    ld = N + G.ADAM_LDC_PAD
    p0, m0 = rnd(M, ld, seed=5, scale=0.1), rnd(M, ld, seed=6, scale=1e-3)
    v0 = torch.rand(M, ld, generator=torch.Generator().manual_seed(7)) * 1e-4
    lr_t = torch.full((1,), hp["lr"], dtype=torch.float32, device="cuda")
    f32 = lambda x: float(np.float32(x))      # noqa: E731  (the hyper-parameters cross the C ABI as float32)
    what = G.case_id(c)
    group = f"adam tile {c.tile}"

    def two_steps(compare):
        step_t = torch.zeros(1, dtype=torch.int64, device="cuda")
        wide = [dev(p0.clone()), dev(m0.clone()), dev(v0.clone())]
        flat = [t[:, :N].contiguous() for t in wide]
        g = torch.full((M, N), NAN, device="cuda")
        for step in (1, 2):
            ops.tick(step_t, None)
            before = [t[:, :N].cpu().numpy().astype(np.float64) for t in wide]
            kw = dict(tile=c.tile) if c.tile else {}
            d1 = ops.gemm(L, Ad, Bd, wide[0][:, :N], alpha=hp["alpha"], ws=ws, **kw,
                          adam=dict(m=wide[1][:, :N], v=wide[2][:, :N], lr_t=lr_t, step_t=step_t, beta1=hp["beta1"],
                                    beta2=hp["beta2"], eps=hp["eps"], weight_decay=hp["weight_decay"],
                                    grad_scale=hp["grad_scale"]))
            assert d1.tile in (2, 3) and d1.splitk == 1 and (not c.tile or d1.tile == c.tile), (d1.tile, d1.splitk)
            if not compare:
                continue
            g.fill_(NAN)
            ops.gemm(L, Ad, Bd, g, alpha=hp["alpha"], tile=d1.tile, splitk=1)
            ops.adamw_flat(flat[0].view(-1), g.view(-1), flat[1].view(-1), flat[2].view(-1), lr_t, step_t,
                           weight_decay=hp["weight_decay"], grad_scale=hp["grad_scale"])
            torch.cuda.synchronize()
            check(group + " gradient", g, hp["alpha"] * product(L, A, B), 1e-4, 1e-4 * math.sqrt(K), f"{what} stored gradient")
            for name, t, r, atol in (("exp_avg", wide[1], flat[1], 1e-9), ("exp_avg_sq", wide[2], flat[2], 1e-12),
                                     ("parameter", wide[0], flat[0], 1e-7)):
                check(group + " vs flat", t[:, :N], r, 1e-6, atol, f"{what} step {step} {name} vs stored gradient + adamw_flat")
            ref = R.adamw64(before[0], g.cpu().numpy(), before[1], before[2], step, f32(hp["lr"]), f32(hp["weight_decay"]),
                            f32(hp["beta1"]), f32(hp["beta2"]), f32(hp["eps"]), grad_scale=hp["grad_scale"])
            for name, t, r, atol in (("parameter", wide[0], ref[0], 1e-6), ("exp_avg", wide[1], ref[1], 1e-8),
                                     ("exp_avg_sq", wide[2], ref[2], 1e-10)):
                check(group + " vs float64", t[:, :N], torch.from_numpy(r), 1e-5, atol, f"{what} step {step} {name} vs float64")
        torch.cuda.synchronize()
        return wide
    first, second = two_steps(True), two_steps(False)
    for name, t, u, t0 in zip(("parameter", "exp_avg", "exp_avg_sq"), first, second, (p0, m0, v0)):
        assert torch.equal(t[:, N:].cpu(), t0[:, N:]), f"{what}: the padding columns of the {name} buffer were written"
        same_bits(t, u, f"{what} {name}")


RUN = dict(raw=run_raw, bias_grad=run_bias_grad, epi=run_epi, xor=run_xor, adam=run_adam)


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_case(ops, ws, c):
    RUN[c.kind](ops, ws, c)


def test_planned_weight_gradient_runs_on_tile_4(ops, ws):
    """The engine's call as it stands (no tile, no split asked for) at the shape of gemm_f32_cases.PLANNED_TILE4: the
    planner's tile 4 is kept, its K-slabs are dropped for bias_grad, and 2 x 32 tiles go through placement mode 2."""
    Kc, M, N = (G.PLANNED_TILE4[k] for k in ("Kc", "M", "N"))
    dY, X = rnd(Kc, M, seed=1), rnd(Kc, N, seed=2)
    dW, db = nan_wide(M, N), torch.full((M + 3,), NAN, device="cuda")
    d = ops.gemm(G.TN, dev(dY), dev(X), dW[:, :N], bias_grad=db[:M], ws=ws)
    torch.cuda.synchronize()
    assert (d.tile, d.splitk) == (4, 1) and G.grid_mode(4, M, N, 1) == (2, 2, 32)
    tail_is_nan(dW, N, "planned dW")
    tail_is_nan(db, M, "planned bias_grad")
    check("planned tile 4", dW[:, :N], dY.double().t() @ X.double(), 1e-4, 1e-4 * math.sqrt(Kc), "planned dW")
    check("planned tile 4", db[:M], dY.double().sum(0), 1e-4, 1e-4 * math.sqrt(Kc), "planned bias_grad")


# ----------------------------------------------------------------------------------------------------------
# grouped launches
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", G.GROUP_CASES, ids=G.group_id)
def test_group(ops, ws, g):
    """Every problem of the group against float64, and against the same problem launched on its own with the same tile
    (at the margins of test_gemm_grouped_matches_individual)."""
    probs = []
    for i, (M, N, K, name) in enumerate(g.problems):
        names = G.GROUP_EPI[name]
        Ad, Bd, A, B = operands(g.layout, M, N, K, 0, seed=100 + 2 * i)
        ep = Epilogue(g.layout, M, N, K, names, seed=300 + 20 * i)
        probs.append(dict(M=M, N=N, K=K, names=names, a=Ad, b=Bd, ref=ep.reference(A, B), kw=ep.kw))

    def fresh():
        """output buffers of one launch of every problem: [(C, pre_out or None)]"""
        return [(nan_wide(p["M"], p["N"]), nan_wide(p["M"], p["N"], extra=7) if "pre_out" in p["names"] else None) for p in probs]

    def kwargs(p, o):
        kw = dict(a=p["a"], b=p["b"], c=o[0][:, :p["N"]], **p["kw"])
        if o[1] is not None:
            kw["pre_out"] = o[1][:, :p["N"]]
        return kw
    outs = []
    for _ in range(2):
        o = fresh()
        ops.GemmGroup(g.layout, [kwargs(p, oo) for p, oo in zip(probs, o)], tile=g.tile).launch()
        torch.cuda.synchronize()
        outs.append(o)
    single = fresh()
    for p, oo in zip(probs, single):
        kw = kwargs(p, oo)
        ops.gemm(g.layout, kw.pop("a"), kw.pop("b"), kw.pop("c"), tile=g.tile, splitk=1, **kw)
    torch.cuda.synchronize()
    group = f"group {g.tag} tile {g.tile}"
    for i, (p, o, o2, s) in enumerate(zip(probs, outs[0], outs[1], single)):
        M, N, K = p["M"], p["N"], p["K"]
        what = f"{G.group_id(g)} problem {i} ({M}x{N}x{K} {sorted(p['names'])})"
        rtol, atol = (1e-4, 1e-4) if p["names"] else (1e-4, 1e-4 * math.sqrt(K))
        tail_is_nan(o[0], N, what)
        check(group, o[0][:, :N], p["ref"][1], rtol, atol, what)
        check(group + " vs single", o[0][:, :N], s[0][:, :N], 1e-4, 1e-3, what + " vs a launch of its own")
        same_bits(o[0], o2[0], what)
        if o[1] is not None:
            tail_is_nan(o[1], N, what + " pre_out")
            check(group, o[1][:, :N], p["ref"][0], rtol, atol, what + " pre_out")
            check(group + " vs single", o[1][:, :N], s[1][:, :N], 1e-4, 1e-3, what + " pre_out vs a launch of its own")
            same_bits(o[1], o2[1], what + " pre_out")
