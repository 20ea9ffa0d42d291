"""The build-defined THREE-modality fuser (r3d_amd/model/cmfuser3.py, csrc/fuser3.hip; BASELINE.json configs[4]) against the
build's own CPU restatement oracle.cm_fuser_m -- **parity unpinned**: the reference's CMFuser is two-token
(model/futr_safuser_tokenfusion.py:74-81), SURVEY.md 8(d) allows exactly this check.  What pins the restatement is that for
M = 2 it is the reference-pinned cm_fuser bit for bit (tests/test_oracle_golden.py).  Forward, selected indices (bit-exact as
sets), and every gradient -- three input streams and all 13 live parameters (Q / K now receive gradient) -- at B = 16,
hidden 1024 (configs[4]'s per-GPU shape) and at a small shape; tolerance 1e-3 of each tensor's scale (north star)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import futr_oracle as O, synth  # noqa: E402


def _close(a, b, what, rtol=1e-3):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    sc = max(float(b.abs().max()), 1e-6)
    err = float((a - b).abs().max())
    assert err <= rtol * sc, f"{what}: max abs err {err:.3e} vs scale {sc:.3e} (rel {err / sc:.2e})"


@pytest.mark.parametrize("B,S,H,heads,mode", [(2, 5, 64, 4, "train"), (16, 16, 1024, 8, "train"), (4, 8, 256, 8, "val")])
def test_three_modality_fuser_matches_the_cpu_restatement(B, S, H, heads, mode):
    from r3d_amd.model.cmfuser3 import CMFuser3
    fz = CMFuser3(H, depth=1, num_heads=heads).to("cuda").eval()          # eval(): embd_drop off; `mode` picks the selection
    names = [("fuser." + n, tuple(p.shape)) for n, p in fz.named_parameters()]
    vals = synth.fill_state(names)
    with torch.no_grad():
        for n, p in fz.named_parameters():
            p.copy_(torch.from_numpy(vals["fuser." + n]))
    pc = {n: torch.from_numpy(v).clone().requires_grad_(True) for n, v in vals.items()}
    xs = [torch.from_numpy(synth.symmetric(B * S * H, 0xF3000 + 17 * m).reshape(B, S, H)).clone() for m in range(3)]
    xs[0] = xs[0].relu()                                                    # (an embedding after its ReLU, as :183,197)
    xs[1] = xs[1].relu() * 0.7
    cot = torch.from_numpy(synth.symmetric(B * S * H, 0xF3900).reshape(B, S, H))
    # CPU restatement
    xc = [x.clone().requires_grad_(True) for x in xs]
    want, aux = O.cm_fuser_m(pc, xc, mode, heads)
    (want * cot).sum().backward()
    # HIP
    xg = [x.cuda().requires_grad_(True) for x in xs]
    got = fz({"rgb": xg[0], "depth": xg[1], "gaze": xg[2]}, mode)
    (got * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    _close(got.detach(), want.detach(), f"H{H}/{mode} fused")
    for m in range(3):
        assert np.array_equal(np.sort(fz.last_idx[m].cpu().numpy()), np.sort(aux["idx"][m].numpy())), f"selection of modality {m}"
        _close(xg[m].grad, xc[m].grad, f"H{H}/{mode} d input {m}")
    live = 0
    for n, p in fz.named_parameters():
        ref = pc["fuser." + n].grad
        if ref is None:
            assert p.grad is None, n
            continue
        live += 1
        _close(p.grad, ref, f"H{H}/{mode} grad {n}", rtol=2e-3)
    assert live == 13
    qk = fz.blocks[0].attn.qkv.weight.grad[:2 * H]
    assert float(qk.abs().max()) > 0.0, "with three tokens the softmax is real: Q / K must receive gradient"


# ------------------------------------------------------------------------------------------------------------------------
# The six entry points on their own, the model in training state, and admission -- against the float64 restatement
# tests/fuser3_oracle.py (pinned without a GPU by tests/test_fuser3_cpu.py) at the cases of tests/fuser3_cases.py.
# ------------------------------------------------------------------------------------------------------------------------
import functools  # noqa: E402

from tests import fuser3_cases as FC, fuser3_oracle as F3  # noqa: E402

DROP_SCALE = float(np.float32(1.0 / (1.0 - FC.DROP_P)))      # as the kernels receive it: a float32


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("N,C", FC.ROW_CASES)
def test_exchange3_kernels_are_exact(N, C, with_keep):
    """A select and one multiplication by drop_scale * keep; the adjoint one such multiplication per term and at most one
    addition: equal (==, a zero's sign is not compared) to the float64 oracle rounded to float32, under every mask kind."""
    from r3d_amd import ops
    xs, g, _ = FC.row_inputs(N, C)
    keep = FC.keep_mask(3 * N, C) if with_keep else None
    xg, gg = [x.cuda() for x in xs], g.cuda()
    kg = keep.cuda() if with_keep else None
    for kind in FC.MASK_KINDS:
        mask = FC.exchange_mask(kind, C)
        x0 = _nan(3 * N, C)
        ops.token_exchange3_fwd(xg[0], xg[1], xg[2], mask.cuda(), x0, drop_mask=kg, drop_scale=DROP_SCALE)
        want = F3.exchange3([x.double() for x in xs], mask.double(), keep, DROP_SCALE).float()
        bad = ~(x0.cpu() == want)
        assert not bool(bad.any()), f"exchange3_fwd {kind}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"
        d = [_nan(N, C) for _ in range(3)]
        ops.token_exchange3_bwd(gg, mask.cuda(), d[0], d[1], d[2], drop_mask=kg, drop_scale=DROP_SCALE)
        ref = F3.exchange3_adjoint(g.double(), mask.double(), keep, DROP_SCALE, term_dtype=torch.float32)
        for m in range(3):
            bad = ~(d[m].cpu() == ref[m].float())
            assert not bool(bad.any()), f"exchange3_bwd {kind} d x{m}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("N,C", FC.ROW_CASES)
def test_triple_mean_kernels(N, C):
    """forward: two additions, one multiplication by the rounded 1/3 and that constant's own rounding: 4 * 2^-24 *
    (|a| + |b| + |c|) / 3 per element; adjoint: 2 * 2^-24 * |d_out| / 3."""
    from r3d_amd import ops
    _, y, d = FC.row_inputs(N, C)
    out, dy = _nan(N, C), _nan(3 * N, C)
    ops.triple_mean_fwd(y.cuda(), out)
    ops.triple_mean_bwd(d.cuda(), dy)
    err = (out.cpu().double() - F3.triple_mean(y.double())).abs()
    lim = 4 * 2.0 ** -24 * y.double().abs().reshape(N, 3, C).sum(dim=1) / 3
    assert bool((err <= lim).all()), f"triple_mean_fwd: {int((~(err <= lim)).sum())} outside, worst {float((err / lim.clamp_min(1e-300)).max()):.2f} of the bound"
    err = (dy.cpu().double() - F3.triple_mean_adjoint(d.double())).abs()
    lim = 2 * 2.0 ** -24 * F3.triple_mean_adjoint(d.double().abs())
    assert bool((err <= lim).all()), f"triple_mean_bwd: {int((~(err <= lim)).sum())} outside, worst {float((err / lim.clamp_min(1e-300)).max()):.2f} of the bound"


@functools.lru_cache(maxsize=None)
def _attn_reference(N, C, heads, variant):
    qkv, d_out = FC.attn_inputs(N, C, heads, variant)
    probs, out = F3.attn3(qkv.double(), heads)
    return qkv, d_out, probs, out, F3.attn3_adjoint(qkv.double(), d_out.double(), heads)


@pytest.mark.parametrize("N,C,heads,variant", FC.ATTN_CASES)
def test_attn3_kernels(N, C, heads, variant):
    """probs (ABI order [N][heads][3][2]), out and the three thirds of d_qkv, each element against the float64 oracle within
    tol (|ref| + the largest |ref| of the same frame); tol from tests/fuser3_cases.py (measured on the CPU)."""
    from r3d_amd import ops
    qkv, d_out, r_probs, r_out, r_dqkv = _attn_reference(N, C, heads, variant)
    probs, out, d_qkv = _nan(N * heads * 6), _nan(3 * N, C), _nan(3 * N, 3 * C)
    ops.attn3_fwd(qkv.cuda(), probs, out, heads)
    ops.attn3_bwd(qkv.cuda(), d_out.cuda(), d_qkv, heads)
    got = FC.attn_ratios(probs.cpu().view(N, heads, 3, 2), out.cpu(), d_qkv.cpu(), r_probs, r_out, r_dqkv)
    tol = FC.attn_tol(variant)
    print(f"attn3 {(N, C, heads, variant)}: " + "  ".join(f"{k} {v:.2e} (tol {tol[k]:.2e})" for k, v in got.items()))
    for k, v in got.items():
        assert v <= tol[k], f"attn3 {k}: {v:.3e} > {tol[k]:.3e}"
    if variant == "q0":
        assert torch.equal(probs.cpu(), torch.full((N * heads * 6,), 0.5)), "q = 0: both logits are 0, every probability exactly 0.5"
    if variant == "sat":
        cond = FC.condition_ratios(d_qkv.cpu(), r_dqkv, *F3.attn3_grad_condition(qkv.double(), d_out.double(), heads))
        print("attn3 saturated, against the condition size: " + "  ".join(f"{k} {v:.2e}" for k, v in cond.items()))
        for k, v in cond.items():
            assert v <= FC.ATTN_TOL_CONDITION[k], f"attn3 saturated {k}: {v:.3e} > {FC.ATTN_TOL_CONDITION[k]:.3e}"


def _module(H, heads, training):
    from r3d_amd.model.cmfuser3 import CMFuser3
    fz = CMFuser3(H, depth=1, num_heads=heads).to("cuda")
    fz.train(training)
    with torch.no_grad():
        for n, v in FC.model_params(H).items():
            fz.get_parameter(n[len(FC.PARAM_PREFIX):]).copy_(v)
    return fz


def _keep_of_call(fz, rows, C, call):
    """The keep mask of the module's call number `call`, by the same ops.dropout_mask launch the module makes."""
    from r3d_amd import ops
    from r3d_amd.model.cmfuser3 import DROP_P
    assert DROP_P == FC.DROP_P
    drop = torch.empty(rows * C, dtype=torch.uint8, device="cuda")
    ops.dropout_mask(drop, DROP_P, fz.drop_seed, torch.full((1,), call, dtype=torch.int64, device="cuda"))
    return drop.view(rows, C).cpu()


def _run(fz, xs, cot, mode):
    xg = [x.cuda().requires_grad_(True) for x in xs]
    got = fz({"rgb": xg[0], "depth": xg[1], "gaze": xg[2]}, mode)
    (got * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    return got.detach(), xg


@pytest.mark.parametrize("B,S,H,heads,mode,training", FC.MODEL_CASES + [FC.BIG_TRAINING_CASE])
def test_model_matches_the_float64_oracle_in_either_state(B, S, H, heads, mode, training):
    """Fused output, selected sets, three input gradients and all 13 live parameter gradients against cm_fuser3 in float64,
    the keep mask regenerated with the module's own seed and call offset; tolerance: error against tensor scale, 8 x what
    float32 itself needs (tests/fuser3_cases.py), far inside the eval-state test's 1e-3 / 2e-3."""
    case = (B, S, H, heads, mode, training)
    fz = _module(H, heads, training)
    xs, cot = FC.model_inputs(B, S, H)
    keep = _keep_of_call(fz, 3 * B * S, H, 0) if training else None
    if training:
        dens = float(keep.float().mean())
        assert 0 < dens < 1 and (B * S * H < 4096 or abs(dens - (1 - FC.DROP_P)) < 0.03), dens
    want, aux, gx, gp = FC.model_reference(case, torch.float64, keep, DROP_SCALE)
    got, xg = _run(fz, xs, cot, mode)
    assert fz._drop_calls == (1 if training else 0)
    figs = {"fused": FC.scale_ratio(got, want)}
    for m in range(3):
        assert np.array_equal(np.sort(fz.last_idx[m].cpu().numpy()), aux["idx"][m].numpy()), f"selection of modality {m}"
        figs[f"d input {m}"] = FC.scale_ratio(xg[m].grad, gx[m])
    pfigs = {}
    for n, p in fz.named_parameters():
        if FC.PARAM_PREFIX + n in FC.LIVE:
            pfigs[n] = FC.scale_ratio(p.grad, gp[FC.PARAM_PREFIX + n])
        else:
            assert p.grad is None, n
    print(f"model {case}: " + "  ".join(f"{k} {v:.2e}" for k, v in {**figs, **pfigs}.items()))
    assert len(pfigs) == 13
    for k, v in figs.items():
        assert v <= FC.MODEL_TOL, f"{case} {k}: {v:.3e} > {FC.MODEL_TOL:.3e}"
    for k, v in pfigs.items():
        assert v <= FC.MODEL_TOL_PARAM, f"{case} grad {k}: {v:.3e} > {FC.MODEL_TOL_PARAM:.3e}"
    qk = fz.blocks[0].attn.qkv.weight.grad[:2 * H]
    assert float(qk[:H].abs().max()) > 0.0 and float(qk[H:].abs().max()) > 0.0, "Q and K must receive gradient"


def test_dropout_offset_advances_and_fresh_modules_repeat():
    B, S, H, heads, mode = 2, 5, 64, 4, "val"
    xs, cot = FC.model_inputs(B, S, H)
    a, b = _module(H, heads, True), _module(H, heads, True)
    keep0, keep1 = _keep_of_call(a, 3 * B * S, H, 0), _keep_of_call(a, 3 * B * S, H, 1)
    assert not torch.equal(keep0, keep1), "the second call's mask (offset 1) must differ from the first's"
    got_a, xa = _run(a, xs, cot, mode)
    got_b, xb = _run(b, xs, cot, mode)
    assert torch.equal(got_a, got_b), "two fresh modules, same inputs: same bits"
    for m in range(3):
        assert torch.equal(xa[m].grad, xb[m].grad), m
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad), n
    # the second forward of the same module is the oracle under the offset-1 mask -- and not under the first call's
    second, _ = _run(a, xs, cot, mode)
    assert a._drop_calls == 2
    case = (B, S, H, heads, mode, True)
    want1 = FC.model_reference(case, torch.float64, keep1, DROP_SCALE)[0]
    want0 = FC.model_reference(case, torch.float64, keep0, DROP_SCALE)[0]
    assert FC.scale_ratio(second, want1) <= FC.MODEL_TOL
    assert FC.scale_ratio(second, want0) > 100 * FC.MODEL_TOL and FC.scale_ratio(got_a, want0) <= FC.MODEL_TOL


@pytest.mark.parametrize("training", [False, True])
def test_strided_inputs_give_the_bits_of_their_contiguous_copies(training):
    """A [B, T, C] slice of a wider tensor, and a strided d_fused, as an engine may hand them over."""
    B, S, H, heads, mode = 2, 3, 130, 2, "val"
    xs, cot = FC.model_inputs(B, S, H)
    dense, strided = _module(H, heads, training), _module(H, heads, training)
    got_d, xd = _run(dense, xs, cot, mode)
    wide = [torch.cat([x, x.flip(-1)], dim=-1).cuda() for x in xs]
    xv = [w[:, :, :H].detach().requires_grad_(True) for w in wide]
    cv = torch.cat([cot, -cot], dim=-1).cuda()[:, :, :H]
    assert not xv[0].is_contiguous() and not cv.is_contiguous()
    got_s = strided({"rgb": xv[0], "depth": xv[1], "gaze": xv[2]}, mode)
    got_s.backward(cv)
    torch.cuda.synchronize()
    assert torch.equal(got_s.detach(), got_d)
    for m in range(3):
        assert torch.equal(xv[m].grad, xd[m].grad), m
    for (n, p), (_, q) in zip(dense.named_parameters(), strided.named_parameters()):
        assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad), n


# --- refusals: each raises before any launch (csrc/fuser3.hip: every R3D_REQUIRE returns ahead of hipLaunchKernelGGL; the
# wrappers' asserts and CMFuser3.forward's run ahead of the ABI call).  Outputs are NaN-filled and must stay so.
@pytest.mark.parametrize("C,heads", [(129, 1), (258, 2), (10, 3), (128, 3)])
def test_attn3_refuses_heads_it_cannot_hold(C, heads):
    from r3d_amd import ops
    from r3d_amd._lib import R3DHipError
    qkv = torch.zeros(3, 3 * C, device="cuda")
    probs, out, d_qkv = _nan(heads * 6), _nan(3, C), _nan(3, 3 * C)
    with pytest.raises(R3DHipError):
        ops.attn3_fwd(qkv, probs, out, heads)
    with pytest.raises(R3DHipError):
        ops.attn3_bwd(qkv, torch.zeros(3, C, device="cuda"), d_qkv, heads)
    torch.cuda.synchronize()
    assert bool(torch.isnan(probs).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(d_qkv).all())


def test_model_refuses_other_modality_counts_and_host_tensors():
    fz = _module(64, 4, False)
    x = torch.zeros(1, 2, 64, device="cuda")
    for keys in (("rgb", "depth"), ("rgb", "depth", "gaze", "audio")):
        with pytest.raises(AssertionError, match="exactly three"):
            fz({k: x for k in keys}, "val")
    with pytest.raises(AssertionError, match="device tensors"):
        fz({k: x.cpu() for k in ("rgb", "depth", "gaze")}, "val")
    with pytest.raises(AssertionError):
        fz({k: torch.zeros(1, 2, 32, device="cuda") for k in ("rgb", "depth", "gaze")}, "val")
    assert fz._drop_calls == 0 and fz.last_idx is None


def test_wrappers_refuse_malformed_operands():
    from r3d_amd import ops
    N, C, heads = 2, 8, 2
    f = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda")      # noqa: E731
    xa, mask, x0, drop = f(N, C), f(3, C), _nan(3 * N, C), torch.ones(3 * N, C, dtype=torch.uint8, device="cuda")
    d = [_nan(N, C) for _ in range(3)]
    qkv, probs, out, d_qkv = f(3 * N, 3 * C), _nan(N * heads * 6), _nan(3 * N, C), _nan(3 * N, 3 * C)
    bad = [
        # float32 on every tensor
        lambda: ops.token_exchange3_fwd(xa.double(), xa, xa, mask, x0),
        lambda: ops.token_exchange3_fwd(xa, xa, xa.half(), mask, x0),
        lambda: ops.token_exchange3_fwd(xa, xa, xa, mask.double(), x0),
        lambda: ops.token_exchange3_fwd(xa, xa, xa, mask, x0.double()),
        lambda: ops.token_exchange3_bwd(x0.double(), mask, *d),
        lambda: ops.token_exchange3_bwd(x0, mask, d[0], d[1].double(), d[2]),
        lambda: ops.attn3_fwd(qkv.double(), probs, out, heads),
        lambda: ops.attn3_fwd(qkv, probs.double(), out, heads),
        lambda: ops.attn3_fwd(qkv, probs, out.double(), heads),
        lambda: ops.attn3_bwd(qkv, out.double(), d_qkv, heads),
        lambda: ops.attn3_bwd(qkv, out, d_qkv.double(), heads),
        lambda: ops.triple_mean_fwd(x0.double(), d[0]),
        lambda: ops.triple_mean_fwd(x0, d[0].double()),
        lambda: ops.triple_mean_bwd(d[0].double(), x0),
        lambda: ops.triple_mean_bwd(d[0], x0.double()),
        # the backward's mask: (3, C), contiguous
        lambda: ops.token_exchange3_bwd(x0, f(2, C), *d),
        lambda: ops.token_exchange3_bwd(x0, f(3, C + 1), *d),
        lambda: ops.token_exchange3_bwd(x0, f(3, 2 * C)[:, ::2], *d),
        # drop_mask: uint8, (3N, C)
        lambda: ops.token_exchange3_fwd(xa, xa, xa, mask, x0, drop_mask=drop.float()),
        lambda: ops.token_exchange3_fwd(xa, xa, xa, mask, x0, drop_mask=drop[:N]),
        lambda: ops.token_exchange3_fwd(xa, xa, xa, mask, x0, drop_mask=drop.view(-1)),
        lambda: ops.token_exchange3_bwd(x0, mask, *d, drop_mask=drop.bool()),
        lambda: ops.token_exchange3_bwd(x0, mask, *d, drop_mask=drop.view(N, 3 * C)),
        # probs: float32 (above) and contiguous
        lambda: ops.attn3_fwd(qkv, _nan(2 * N * heads * 6)[::2], out, heads),
        lambda: ops.attn3_fwd(qkv, _nan(N * heads * 6 - 1), out, heads),
        # rows % 3 and C3 % 3: no remainder is dropped
        lambda: ops.attn3_fwd(f(3 * N + 1, 3 * C), probs, _nan(3 * N + 1, C), heads),
        lambda: ops.attn3_fwd(f(3 * N, 3 * C + 1), probs, out, heads),
        lambda: ops.attn3_bwd(f(3 * N + 2, 3 * C), f(3 * N + 2, C), _nan(3 * N + 2, 3 * C), heads),
        lambda: ops.attn3_bwd(f(3 * N, 3 * C + 2), out, _nan(3 * N, 3 * C + 2), heads),
        # strides
        lambda: ops.attn3_fwd(f(3 * N, 6 * C)[:, :3 * C], probs, out, heads),
        lambda: ops.triple_mean_fwd(f(3 * N, 2 * C)[:, :C], d[0]),
        lambda: ops.triple_mean_bwd(f(N, 2 * C)[:, :C], x0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(AssertionError):
            call()
            pytest.fail(f"malformed call {i} was accepted")
    torch.cuda.synchronize()
    for t in [x0, probs, out, d_qkv] + d:
        assert bool(torch.isnan(t).all()), "a refused call must not have launched"
