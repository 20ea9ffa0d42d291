"""The split-key cross-attention core (csrc/attention_splitk.hip) against the float64 reference of the tiled test, operands
laid out as the token-fusion engine has them: q a [B*Lq, H] buffer, k and v the column halves of one [B*Lk, 2H] buffer, the
gradients slices of NaN-filled wider buffers whose outside must stay untouched.  Shapes on both sides of every 64-key tile
and chunk boundary, 1 / 8 / 16 queries, head widths that are no multiple of the MFMA k-step (tests/splitk_cases.py); a first
chunk wholly masked, a single valid key in the last chunk; key labels against the key-padding mask and a second run, bit for
bit; parity with the S x S core, interchange with the tiled core, the wholly masked clip, refusal.  Needs an MI355X.

Tolerances (max abs error / max abs of the reference, tests/test_engine_gpu.close_rel): 1e-4 for o, lse and delta, 1e-3 for
dq, dk, dv, per tensor -- those of tests/test_tiled_attention_gpu.py for this operation."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import splitk_cases as SC  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402
from tests.test_query_kernels_gpu import rnd, strided, outside_untouched  # noqa: E402
from tests.test_tiled_attention_gpu import reference, keep_mask  # noqa: E402

PAD, B = SC.PAD, SC.B
assert (PAD, B) == (99, 3)              # (reference and keep_mask are written for the tiled test's own B and PAD)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def problem(Lk, Lq, dh, heads, drop, mask, C):
    """Inputs on the host and the float64 reference, computed once per shape and left unchanged."""
    H = heads * dh
    q, kv, d_o = rnd(B * Lq, H, seed=Lk + 3 * Lq + dh), rnd(B * Lk, 2 * H, seed=Lk + 1), rnd(B * Lq, H, seed=Lk + 2)
    lab = SC.labels(Lk, mask, C)
    keep, dsc = keep_mask(heads, Lq, Lk, drop)
    ref = reference(q, kv[:, :H], kv[:, H:], d_o, lab, keep, dsc, heads, dh, Lq, Lk)
    return q, kv, d_o, lab, keep, dsc, ref


def run_splitk(ops, q, k, v, d_o, heads, dh, Lq, Lk, dq, dk, dv, *, key_labels=None, kpm=None, keep=None, dsc=1.0, bwd=True):
    H = heads * dh
    o = torch.empty(B * Lq, H, device="cuda")
    lse = torch.empty(B, heads, Lq, device="cuda")
    delta = torch.empty(B, heads, Lq, device="cuda")
    ws = torch.full((max(ops.mha_splitk_ws_floats(B, heads, Lq, Lk, dh, False),
                         ops.mha_splitk_ws_floats(B, heads, Lq, Lk, dh, True)),), float("nan"), device="cuda")
    kw = dict(key_labels=key_labels, kpm=kpm, pad_idx=PAD, drop_mask=keep, drop_scale=dsc)
    ops.mha_splitk_fwd(q, k, v, o, lse, ws, B, heads, Lq, Lk, dh, **kw)
    if bwd:
        ops.mha_splitk_bwd(q, k, v, o, lse, d_o, delta, dq, dk, dv, ws, B, heads, Lq, Lk, dh, **kw)
    return o, lse, delta


def grad_buffers(Lq, Lk, H):
    """dq a slice of [B*Lq, H + 9], dk | dv the halves of a [B*Lk, 2H] slice of [B*Lk, 2H + 7], all NaN outside."""
    dq, dqb = strided(torch.zeros(B * Lq, H), H + 9, 5)
    dkv, dkvb = strided(torch.zeros(B * Lk, 2 * H), 2 * H + 7, 3)
    return dq, dqb, dkv, dkvb


@pytest.mark.parametrize("row", SC.ROWS, ids=SC.row_id)
def test_splitk_against_fp64(ops, row):
    lk, Lq, dh, heads, drop, mask = row
    Lk = SC.resolve(lk, dh, ops.mha_splitk_chunk)
    C = ops.mha_splitk_chunk(Lk, dh)
    assert C > 0 and C % 64 == 0
    H = heads * dh
    q, kv, d_o, lab, keep, dsc, (o64, lse64, gq, gk, gv) = problem(Lk, Lq, dh, heads, drop, mask, C)
    if drop:
        assert Lk % 4, "the keep-mask's row stride must be no multiple of 4 bytes"
    qd, kvd, dod, labd = q.cuda(), kv.cuda(), d_o.cuda(), lab.cuda()
    kd = keep.cuda() if drop else None
    dq, dqb, dkv, dkvb = grad_buffers(Lq, Lk, H)
    o, lse, delta = run_splitk(ops, qd, kvd[:, :H], kvd[:, H:], dod, heads, dh, Lq, Lk, dq, dkv[:, :H], dkv[:, H:],
                               key_labels=labd, keep=kd, dsc=dsc)
    # key-label masking is the key-padding mask of the same keys, bit for bit (forward and backward)
    dq_k, _, dkv_k, _ = grad_buffers(Lq, Lk, H)
    o_k, lse_k, delta_k = run_splitk(ops, qd, kvd[:, :H], kvd[:, H:], dod, heads, dh, Lq, Lk, dq_k, dkv_k[:, :H], dkv_k[:, H:],
                                     kpm=(lab == PAD).to(torch.uint8).cuda(), keep=kd, dsc=dsc)
    # a second run of the pair on the same inputs: bit-equal
    dq2, _, dkv2, _ = grad_buffers(Lq, Lk, H)
    o2, lse2, delta2 = run_splitk(ops, qd, kvd[:, :H], kvd[:, H:], dod, heads, dh, Lq, Lk, dq2, dkv2[:, :H], dkv2[:, H:],
                                  key_labels=labd, keep=kd, dsc=dsc)
    torch.cuda.synchronize()
    tag = SC.row_id(row) + f" (Lk {Lk}, chunk {C})"
    d64 = (o64 * d_o.double()).reshape(B, Lq, heads, dh).sum(-1).transpose(1, 2)
    flat = lambda *ts: torch.cat([t.double().cpu().reshape(-1) for t in ts])         # noqa: E731
    for name, got, want, rtol in (("o", o, o64, 1e-4), ("lse", lse, lse64, 1e-4), ("delta", delta, d64, 1e-4),
                                  ("dq", dq, gq, 1e-3), ("dk", dkv[:, :H], gk, 1e-3), ("dv", dkv[:, H:], gv, 1e-3),
                                  ("dq|dk|dv", flat(dq, dkv[:, :H], dkv[:, H:]), flat(gq, gk, gv), 1e-3)):
        a, b = got.double().cpu(), want.double()
        print(f"[splitk] {tag} {name}: err {float((a - b).abs().max()):.2e}, scale {float(b.abs().max()):.2e}")
        # with a single key (Lk 1) the exact dq and dk are 0 in every clip -- delta = rowsum(dO o O) and dO . v round
        # differently -- and only dv gives the gradients a scale: those two are held to the gradients' joint scale alone,
        # as tests/test_tiled_attention_gpu.py holds its [N, 3H] gradient buffer
        if float(b.abs().max()) > 0:
            close_rel(got, want, f"{tag} {name}", rtol=rtol)
    assert outside_untouched(dqb, 5, H) and outside_untouched(dkvb, 3, 2 * H), tag
    for a, b in ((o_k, o), (lse_k, lse), (delta_k, delta), (dq_k, dq), (dkv_k, dkv)):
        assert torch.equal(a, b), tag
    for a, b in ((o2, o), (lse2, lse), (delta2, delta), (dq2, dq), (dkv2, dkv)):
        assert torch.equal(a, b), tag
    if mask == "three" and not drop:        # clip 0 attends to key 0 alone: every output row of a head is that key's value row
        v0 = kv[:, H:].reshape(B, Lk, H)[0, 0]
        assert torch.equal(o.cpu().reshape(B, Lq, H)[0], v0.expand(Lq, H)), tag


def _small(Lq, Lk, dh, heads=8, drop=True):
    H = heads * dh
    q, kv, d_o = rnd(B * Lq, H, seed=Lk + dh).cuda(), rnd(B * Lk, 2 * H, seed=5).cuda(), rnd(B * Lq, H, seed=4).cuda()
    lab = SC.labels(Lk, "three", 0).cuda()
    keep, dsc = keep_mask(heads, Lq, Lk, drop)
    return H, q, kv, d_o, lab, keep.cuda() if drop else None, dsc


@pytest.mark.parametrize("Lq,Lk,dh", [(8, 64, 16), (8, 300, 16)])
def test_splitk_agrees_with_the_core_where_both_run(ops, Lq, Lk, dh):
    heads = 8
    H, q, kv, d_o, lab, keep, dsc = _small(Lq, Lk, dh)
    probs, oc = torch.empty(B, heads, Lq, Lk, device="cuda"), torch.empty(B * Lq, H, device="cuda")
    gqc, gkvc = torch.empty(B * Lq, H, device="cuda"), torch.empty(B * Lk, 2 * H, device="cuda")
    ops.mha_core_fwd(q, kv[:, :H], kv[:, H:], probs, oc, B, heads, Lq, Lk, dh, key_labels=lab, pad_idx=PAD, drop_mask=keep,
                     drop_scale=dsc)
    ops.mha_core_bwd(q, kv[:, :H], kv[:, H:], probs, d_o, gqc, gkvc[:, :H], gkvc[:, H:], B, heads, Lq, Lk, dh, drop_mask=keep,
                     drop_scale=dsc)
    gq, gkv = torch.empty_like(gqc), torch.empty_like(gkvc)
    o, lse, _ = run_splitk(ops, q, kv[:, :H], kv[:, H:], d_o, heads, dh, Lq, Lk, gq, gkv[:, :H], gkv[:, H:], key_labels=lab,
                           keep=keep, dsc=dsc)
    torch.cuda.synchronize()
    close_rel(o, oc, "o against the core", rtol=1e-4)
    for name, got, want in (("dq", gq, gqc), ("dk", gkv[:, :H], gkvc[:, :H]), ("dv", gkv[:, H:], gkvc[:, H:])):
        close_rel(got, want, f"{name} against the core", rtol=1e-3)


def test_splitk_and_tiled_are_interchangeable(ops):
    """(Lq, Lk, dh) = (8, 300, 16): the split-key forward feeds the tiled backward and the reverse; o, lse and every gradient
    within the kernel tolerances of the float64 reference."""
    Lq, Lk, dh, heads = 8, 300, 16, 8
    H, q, kv, d_o, lab, keep, dsc = _small(Lq, Lk, dh)
    o64, lse64, gq64, gk64, gv64 = reference(q.cpu(), kv[:, :H].cpu(), kv[:, H:].cpu(), d_o.cpu(), lab.cpu(), keep.cpu(), dsc,
                                             heads, dh, Lq, Lk)
    kw = dict(key_labels=lab, pad_idx=PAD, drop_mask=keep, drop_scale=dsc)
    k, v = kv[:, :H], kv[:, H:]
    new = lambda *s: torch.full(s, float("nan"), device="cuda")         # noqa: E731
    ws = new(max(ops.mha_splitk_ws_floats(B, heads, Lq, Lk, dh, t) for t in (False, True)))
    for fwd in ("splitk", "tiled"):
        o, lse, delta, gq, gkv = new(B * Lq, H), new(B, heads, Lq), new(B, heads, Lq), new(B * Lq, H), new(B * Lk, 2 * H)
        if fwd == "splitk":
            ops.mha_splitk_fwd(q, k, v, o, lse, ws, B, heads, Lq, Lk, dh, **kw)
            ops.mha_tiled_bwd(q, k, v, o, lse, d_o, delta, gq, gkv[:, :H], gkv[:, H:], B, heads, Lq, Lk, dh, **kw)
        else:
            ops.mha_tiled_fwd(q, k, v, o, lse, B, heads, Lq, Lk, dh, **kw)
            ops.mha_splitk_bwd(q, k, v, o, lse, d_o, delta, gq, gkv[:, :H], gkv[:, H:], ws, B, heads, Lq, Lk, dh, **kw)
        torch.cuda.synchronize()
        tag = f"{fwd} forward, the other backward"
        close_rel(o, o64, f"{tag}: o", rtol=1e-4)
        close_rel(lse, lse64, f"{tag}: lse", rtol=1e-4)
        for name, got, want in (("dq", gq, gq64), ("dk", gkv[:, :H], gk64), ("dv", gkv[:, H:], gv64)):
            close_rel(got, want, f"{tag}: {name}", rtol=1e-3)


def test_a_wholly_masked_clip_gives_the_cores_nan_rows(ops):
    """Clip 1 of three has every key masked: its rows of o are NaN exactly where the S x S core's are, the other clips' rows
    are finite and agree with the core's."""
    Lq, Lk, dh, heads = 8, 300, 16, 8
    H, q, kv, d_o, lab, _, _ = _small(Lq, Lk, dh, drop=False)
    lab[1, :] = PAD
    probs, oc = torch.empty(B, heads, Lq, Lk, device="cuda"), torch.empty(B * Lq, H, device="cuda")
    ops.mha_core_fwd(q, kv[:, :H], kv[:, H:], probs, oc, B, heads, Lq, Lk, dh, key_labels=lab, pad_idx=PAD)
    o, lse, _ = run_splitk(ops, q, kv[:, :H], kv[:, H:], d_o, heads, dh, Lq, Lk, None, None, None, key_labels=lab, bwd=False)
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(o), torch.isnan(oc))
    assert bool(torch.isnan(o.view(B, Lq, H)[1]).all()) and not bool(torch.isnan(o.view(B, Lq, H)[[0, 2]]).any())
    close_rel(o.view(B, Lq, H)[[0, 2]], oc.view(B, Lq, H)[[0, 2]], "the other clips", rtol=1e-4)


@pytest.mark.parametrize("Lq,dh,heads", [(17, 16, 8), (8, 129, 1)])
def test_refused_shape_raises_and_writes_nothing(ops, Lq, dh, heads):
    from r3d_amd._lib import R3DHipError
    Lk, H = 70, heads * dh
    q, kv, d_o = rnd(B * Lq, H, seed=1).cuda(), rnd(B * Lk, 2 * H, seed=2).cuda(), rnd(B * Lq, H, seed=3).cuda()
    o, lse, delta = torch.zeros(B * Lq, H, device="cuda"), torch.zeros(B, heads, Lq, device="cuda"), torch.zeros(B, heads, Lq, device="cuda")
    gq, gkv, ws = torch.zeros(B * Lq, H, device="cuda"), torch.zeros(B * Lk, 2 * H, device="cuda"), torch.zeros(1 << 16, device="cuda")
    assert not ops.mha_splitk_supported(Lq, Lk, dh, False) and not ops.mha_splitk_supported(Lq, Lk, dh, True)
    assert ops.mha_splitk_ws_floats(B, heads, Lq, Lk, dh, True) == 0
    with pytest.raises(R3DHipError):
        ops.mha_splitk_fwd(q, kv[:, :H], kv[:, H:], o, lse, ws, B, heads, Lq, Lk, dh)
    with pytest.raises(R3DHipError):
        ops.mha_splitk_bwd(q, kv[:, :H], kv[:, H:], o, lse, d_o, delta, gq, gkv[:, :H], gkv[:, H:], ws, B, heads, Lq, Lk, dh)
    torch.cuda.synchronize()
    for t in (o, lse, delta, gq, gkv, ws):
        assert not bool(t.any())
