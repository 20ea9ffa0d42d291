"""The tiled attention core (csrc/attention_tiled.hip) against float64 torch, operands laid out as the query models'
engine lays them out (q / k / v column slices of one [N, 3H] buffer): shapes on both sides of every 64-row tile boundary,
head widths that are no multiple of the MFMA k-step, key tiles that are masked entirely (the first one included), a single
valid key, dropout masks whose row stride is no multiple of 4 bytes; rectangular Lq != Lk into slices of wider buffers;
parity with the S x S core where both run; bitwise reproducibility; refusal.  Needs an MI355X.

Tolerances (max abs error / max abs of the reference, tests/test_engine_gpu.close_rel): 1e-4 for o and lse, 1e-3 for
dq / dk / dv -- the figures tests/test_query_kernels_gpu.test_mha_core_at_lq_equals_lk uses for this operation, on the
[N, 3H] gradient buffer as a whole where q, k and v share one (as that test does), per tensor in the rectangular case."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_engine_gpu import close_rel  # noqa: E402
from tests.test_query_kernels_gpu import rnd, strided, outside_untouched  # noqa: E402

PAD = 99
B = 3


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


def labels(Lk):
    """clip 0: only key 0 valid; clip 1: keys [0, 64) all masked and the later ones valid where Lk > 64, else every third
    key masked; clip 2: a masked tail covering the whole last 64-key tile (never every key)."""
    lab = torch.zeros(B, Lk, dtype=torch.int64)
    lab[0, 1:] = PAD
    if Lk > 64:
        lab[1, :64] = PAD
    else:
        lab[1, 2::3] = PAD
    last_tile = (Lk - 1) // 64 * 64
    if Lk > 1:
        lab[2, (last_tile if last_tile else Lk // 2):] = PAD          # (one tile only: its second half)
    assert bool((lab != PAD).any(dim=1).all())
    return lab


def reference(q, k, v, d_o, lab, keep, dsc, heads, dh, Lq, Lk):
    """fp64: o [B*Lq, H], lse [B, heads, Lq], dq, dk, dv."""
    H = heads * dh
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    qh = qr.reshape(B, Lq, heads, dh).transpose(1, 2)
    kh = kr.reshape(B, Lk, heads, dh).transpose(1, 2)
    vh = vr.reshape(B, Lk, heads, dh).transpose(1, 2)
    s = ((qh @ kh.transpose(-2, -1)) / math.sqrt(dh)).masked_fill((lab == PAD)[:, None, None, :], float("-inf"))
    att = s.softmax(-1)
    if keep is not None:
        att = att * keep.double() * dsc
    o = (att @ vh).transpose(1, 2).reshape(B * Lq, H)
    o.backward(d_o.double())
    return o.detach(), torch.logsumexp(s, -1).detach(), qr.grad, kr.grad, vr.grad


def keep_mask(heads, Lq, Lk, drop):
    if not drop:
        return None, 1.0
    g = torch.Generator().manual_seed(5)
    return (torch.rand(B, heads, Lq, Lk, generator=g) > 0.1).to(torch.uint8), 1 / 0.9


def run_tiled(ops, q, k, v, d_o, heads, dh, Lq, Lk, dq, dk, dv, *, key_labels=None, kpm=None, keep=None, dsc=1.0):
    H = heads * dh
    o = torch.empty(B * Lq, H, device="cuda")
    lse = torch.empty(B, heads, Lq, device="cuda")
    delta = torch.empty(B, heads, Lq, device="cuda")
    kw = dict(key_labels=key_labels, kpm=kpm, pad_idx=PAD, drop_mask=keep, drop_scale=dsc)
    ops.mha_tiled_fwd(q, k, v, o, lse, B, heads, Lq, Lk, dh, **kw)
    ops.mha_tiled_bwd(q, k, v, o, lse, d_o, delta, dq, dk, dv, B, heads, Lq, Lk, dh, **kw)
    return o, lse, delta


SQUARE = [(1, 16, 8, False), (63, 16, 8, True), (64, 16, 8, False), (65, 16, 8, True), (129, 8, 4, True), (130, 5, 8, False),
          (41, 25, 8, True), (17, 64, 8, False), (70, 65, 2, True), (9, 128, 2, True), (200, 128, 1, False),
          (1142, 16, 8, False)]


@pytest.mark.parametrize("S,dh,heads,drop", SQUARE)
def test_tiled_self_attention_against_fp64(ops, S, dh, heads, drop):
    H = heads * dh
    qkv = rnd(B * S, 3 * H, seed=S * 7 + dh)
    d_o = rnd(B * S, H, seed=3)
    lab = labels(S)
    keep, dsc = keep_mask(heads, S, S, drop)
    o64, lse64, gq, gk, gv = reference(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], d_o, lab, keep, dsc, heads, dh, S, S)
    qd, dod, labd = qkv.cuda(), d_o.cuda(), lab.cuda()
    kd = keep.cuda() if drop else None
    sl = lambda t: (t[:, :H], t[:, H:2 * H], t[:, 2 * H:])      # noqa: E731
    dqkv = torch.full((B * S, 3 * H), float("nan"), device="cuda")
    o, lse, delta = run_tiled(ops, *sl(qd), dod, heads, dh, S, S, *sl(dqkv), key_labels=labd, keep=kd, dsc=dsc)
    # key-label masking is the key-padding mask of the same keys, bit for bit
    o_k = torch.empty_like(o)
    lse_k = torch.empty_like(lse)
    ops.mha_tiled_fwd(*sl(qd), o_k, lse_k, B, heads, S, S, dh, kpm=(lab == PAD).to(torch.uint8).cuda(), drop_mask=kd,
                      drop_scale=dsc)
    # a second run of the pair on the same inputs: bit-equal
    dqkv2 = torch.full((B * S, 3 * H), float("nan"), device="cuda")
    o2, lse2, delta2 = run_tiled(ops, *sl(qd), dod, heads, dh, S, S, *sl(dqkv2), key_labels=labd, keep=kd, dsc=dsc)
    torch.cuda.synchronize()
    tag = f"S={S} dh={dh}"
    close_rel(o, o64, f"{tag} o", rtol=1e-4)
    close_rel(lse, lse64, f"{tag} lse", rtol=1e-4)
    close_rel(delta, (o64 * d_o.double()).reshape(B, S, heads, dh).sum(-1).transpose(1, 2), f"{tag} delta", rtol=1e-4)
    # the [N, 3H] gradient buffer against its reference, as test_mha_core_at_lq_equals_lk compares it (with one valid key the
    # exact dq and dk are 0: delta = rowsum(dO o O) and dO . v round differently, and only dv gives the buffer a scale)
    close_rel(dqkv, torch.cat([gq, gk, gv], 1), f"{tag} dq|dk|dv", rtol=1e-3)
    assert torch.equal(o_k, o) and torch.equal(lse_k, lse)
    assert torch.equal(o2, o) and torch.equal(lse2, lse) and torch.equal(delta2, delta) and torch.equal(dqkv2, dqkv)
    # clip 0 attends to key 0 alone: every output row of a head is that key's value row (times the keep factor)
    if not drop:
        v0 = qkv[:, 2 * H:].reshape(B, S, H)[0, 0]
        assert torch.equal(o.cpu().reshape(B, S, H)[0], v0.expand(S, H))


def test_tiled_rectangular_into_slices_of_wider_buffers(ops):
    """Lq = 70, Lk = 133: k / v are slices of an [N_k, 2H] buffer, the gradients land in slices of NaN-filled wider buffers
    whose other columns stay NaN."""
    Lq, Lk, dh, heads = 70, 133, 16, 8
    H = heads * dh
    q, kv, d_o = rnd(B * Lq, H, seed=11), rnd(B * Lk, 2 * H, seed=12), rnd(B * Lq, H, seed=13)
    lab = labels(Lk)
    keep, dsc = keep_mask(heads, Lq, Lk, True)
    o64, lse64, gq, gk, gv = reference(q, kv[:, :H], kv[:, H:], d_o, lab, keep, dsc, heads, dh, Lq, Lk)
    qd, _ = strided(q, H + 12, 4)
    kvd = kv.cuda()
    dod, _ = strided(d_o, H + 4, 4)
    zq, zk = torch.zeros(B * Lq, H), torch.zeros(B * Lk, H)
    (dq, dqb), (dk, dkb), (dv, dvb) = strided(zq, H + 9, 5), strided(zk, 2 * H + 7, 3), strided(zk, H + 16, 16)
    o, lse, _ = run_tiled(ops, qd, kvd[:, :H], kvd[:, H:], dod, heads, dh, Lq, Lk, dq, dk, dv, key_labels=lab.cuda(),
                          keep=keep.cuda(), dsc=dsc)
    torch.cuda.synchronize()
    close_rel(o, o64, "rect o", rtol=1e-4)
    close_rel(lse, lse64, "rect lse", rtol=1e-4)
    for name, got, want in (("dq", dq, gq), ("dk", dk, gk), ("dv", dv, gv)):
        close_rel(got, want, f"rect {name}", rtol=1e-3)
    assert outside_untouched(dqb, 5, H) and outside_untouched(dkb, 3, H) and outside_untouched(dvb, 16, H)


@pytest.mark.parametrize("S,dh,heads", [(64, 16, 8), (8, 128, 2)])
def test_tiled_agrees_with_the_core_where_both_run(ops, S, dh, heads):
    """Both are fp32 evaluations of the same sums: 1e-5 of scale."""
    H = heads * dh
    qkv, d_o, lab = rnd(B * S, 3 * H, seed=S + dh).cuda(), rnd(B * S, H, seed=4).cuda(), labels(S).cuda()
    keep, dsc = keep_mask(heads, S, S, True)
    keep = keep.cuda()
    sl = lambda t: (t[:, :H], t[:, H:2 * H], t[:, 2 * H:])      # noqa: E731
    probs, oc, gc = torch.empty(B, heads, S, S, device="cuda"), torch.empty(B * S, H, device="cuda"), torch.empty(B * S, 3 * H, device="cuda")
    ops.mha_core_fwd(*sl(qkv), probs, oc, B, heads, S, S, dh, key_labels=lab, pad_idx=PAD, drop_mask=keep, drop_scale=dsc)
    ops.mha_core_bwd(*sl(qkv), probs, d_o, *sl(gc), B, heads, S, S, dh, drop_mask=keep, drop_scale=dsc)
    gt = torch.empty_like(gc)
    ot, _, _ = run_tiled(ops, *sl(qkv), d_o, heads, dh, S, S, *sl(gt), key_labels=lab, keep=keep, dsc=dsc)
    torch.cuda.synchronize()
    close_rel(ot, oc, "o against the core", rtol=1e-5)
    for i, name in enumerate(("dq", "dk", "dv")):
        close_rel(gt[:, i * H:(i + 1) * H], gc[:, i * H:(i + 1) * H], f"{name} against the core", rtol=1e-5)


def test_refused_head_width_raises_and_writes_nothing(ops):
    from r3d_amd._lib import R3DHipError
    S, dh, heads = 8, 129, 1
    H = heads * dh
    qkv, d_o = rnd(B * S, 3 * H, seed=1).cuda(), rnd(B * S, H, seed=2).cuda()
    sl = lambda t: (t[:, :H], t[:, H:2 * H], t[:, 2 * H:])      # noqa: E731
    o, lse, delta = torch.zeros(B * S, H, device="cuda"), torch.zeros(B, heads, S, device="cuda"), torch.zeros(B, heads, S, device="cuda")
    g = torch.zeros(B * S, 3 * H, device="cuda")
    assert not ops.mha_tiled_supported(S, S, dh, False)
    with pytest.raises(R3DHipError):
        ops.mha_tiled_fwd(*sl(qkv), o, lse, B, heads, S, S, dh)
    with pytest.raises(R3DHipError):
        ops.mha_tiled_bwd(*sl(qkv), o, lse, d_o, delta, *sl(g), B, heads, S, S, dh)
    torch.cuda.synchronize()
    for t in (o, lse, delta, g):
        assert not bool(t.any())
