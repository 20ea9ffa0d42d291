"""The kernels only the query models (r3d_amd/engine_unsup.py) reach, at the shapes those models give them, against float64
torch (fp32 torch bit for bit where the kernel is one rounding per element): the adaptive average pooling of csrc/posenc.hip
and its adjoint, the positional encoding with its dropout / ReLU gate, the label-index gather and its adjoint (out-of-range
indices included), and the attention core at Lq = Lk = S with key-label masking.  Needs an MI355X."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.helpers import assert_close  # noqa: E402
from tests import query_cases as QC  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


def strided(t, ld, c0, fill=float("nan")):
    """t [rows, H] as the column slice [:, c0:c0 + H] of a [rows, ld] device buffer filled with `fill` elsewhere; returns
    (slice, buffer)."""
    rows, H = t.shape
    buf = torch.full((rows, ld), fill, dtype=t.dtype)
    buf[:, c0:c0 + H] = t
    buf = buf.cuda()
    return buf[:, c0:c0 + H], buf


def outside_untouched(buf, c0, H, fill_value=None):
    keep = torch.ones(buf.shape[1], dtype=torch.bool)
    keep[c0:c0 + H] = False
    rest = buf.cpu()[:, keep]
    return bool(torch.isnan(rest).all()) if fill_value is None else bool((rest == fill_value).all())


# ----------------------------------------------------------------------------------------------------------
# adaptive average pooling of the S decoder outputs to Q rows (futr_unsupervised_depth.py:134) and its adjoint
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 3, 8, 13])
@pytest.mark.parametrize("S", [1, 2, 5, 7, 8, 9, 13, 64, 65, 1000])
def test_avgpool_rows_matches_adaptive_avg_pool1d(ops, S, Q):
    B, H = 3, 72                                  # (H not a multiple of 64; rows are slices of wider buffers)
    x = rnd(B * S, H, seed=S * 31 + Q)
    dy = rnd(B * Q, H, seed=S * 37 + Q + 1)
    xr = x.double().requires_grad_(True)
    ref = F.adaptive_avg_pool1d(xr.view(B, S, H).permute(0, 2, 1), Q).permute(0, 2, 1).reshape(B * Q, H)
    ref.backward(dy.double())
    xd, _ = strided(x, H + 13, 5)
    yd, ybuf = strided(torch.zeros(B * Q, H), H + 9, 3)
    ops.avgpool_rows_fwd(xd, yd, B, S, Q)
    dyd, _ = strided(dy, H + 5, 2)
    dxd, dxbuf = strided(torch.zeros(B * S, H), H + 11, 7)
    ops.avgpool_rows_bwd(dyd, dxd, B, S, Q)
    torch.cuda.synchronize()
    assert_close(yd.cpu(), ref.detach(), 1e-5, 1e-6, f"avgpool fwd S={S} Q={Q}")
    assert_close(dxd.cpu(), xr.grad, 1e-5, 1e-6, f"avgpool bwd S={S} Q={Q}")
    assert outside_untouched(ybuf, 3, H) and outside_untouched(dxbuf, 7, H)
    if S == Q:                                    # identity, both ways (a window of one row: x / 1)
        assert torch.equal(yd.cpu(), x) and torch.equal(dxd.cpu(), dy)


# ----------------------------------------------------------------------------------------------------------
# positional encoding + dropout (position.py:29-35) and its backward with the ReLU gate: one rounding per element
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,H", [(3, 7, 40), (2, 65, 264), (1, 1, 8), (4, 16, 1032)])
@pytest.mark.parametrize("drop", [False, True])
def test_posenc_fwd_is_bit_exact(ops, B, S, H, drop):
    rows = B * S
    x = rnd(rows, H, seed=1)
    table = rnd(S + 3, H, seed=2)                 # (more rows than S: only the first S are read)
    g = torch.Generator().manual_seed(3)
    keep = (torch.rand(rows, H, generator=g) > 0.1).to(torch.uint8)
    dsc = 1.0 / 0.9
    v = x + table[torch.arange(rows) % S]
    want = torch.where(keep.bool(), v * torch.tensor(dsc, dtype=torch.float32), torch.zeros(())) if drop else v
    xd, _ = strided(x, H + 6, 1)
    td, _ = strided(table, H + 17, 4)
    yd, ybuf = strided(torch.zeros(rows, H), H + 3, 2)
    ops.posenc_fwd(xd, td, S, yd, drop_mask=keep.cuda() if drop else None, drop_scale=dsc)
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), want), float((yd.cpu() - want).abs().max())
    assert outside_untouched(ybuf, 2, H)


@pytest.mark.parametrize("drop,gate", [(False, False), (True, False), (False, True), (True, True)])
def test_posenc_bwd_is_bit_exact(ops, drop, gate):
    rows, H = 3 * 37, 264
    dy = rnd(rows, H, seed=4)
    gt = torch.relu(rnd(rows, H, seed=5))         # the post-ReLU embedding: exact zeros where the gate is shut
    gt[0, :5] = -1.0                              # (a negative gate value shuts it as well)
    g = torch.Generator().manual_seed(6)
    keep = (torch.rand(rows, H, generator=g) > 0.1).to(torch.uint8)
    dsc = 1.0 / 0.9
    want = torch.where(keep.bool(), dy * torch.tensor(dsc, dtype=torch.float32), torch.zeros(())) if drop else dy.clone()
    if gate:
        want = torch.where(gt > 0, want, torch.zeros(()))
    dyd, _ = strided(dy, H + 8, 3)
    gd, _ = strided(gt, H + 5, 1)
    dxd, dxbuf = strided(torch.zeros(rows, H), H + 4, 0)
    ops.posenc_bwd(dyd, dxd, drop_mask=keep.cuda() if drop else None, drop_scale=dsc, gate=gd if gate else None)
    torch.cuda.synchronize()
    assert torch.equal(dxd.cpu(), want), float((dxd.cpu() - want).abs().max())
    assert outside_untouched(dxbuf, 0, H)


# ----------------------------------------------------------------------------------------------------------
# label-index gather (futr_proposed.py:103-106) and its adjoint
# ----------------------------------------------------------------------------------------------------------
N_EMBED, N_USED = 50, 30                          # rows N_USED.. of the embedding are never looked up


@pytest.mark.parametrize("H", [40, 264, 1032])
def test_embed_gather_matches_embedding(ops, H):
    B, S = 5, 61                                  # 305 rows (> 256)
    rows = B * S
    w = rnd(N_EMBED, H, seed=7)
    g = torch.Generator().manual_seed(8)
    idx = torch.randint(0, N_USED, (rows,), generator=g, dtype=torch.int64)     # repeated indices
    table = rnd(S + 2, H, seed=9)
    d_out = rnd(rows, H, seed=10)
    wr = w.double().requires_grad_(True)
    F.embedding(idx, wr).backward(d_out.double())
    want = F.embedding(idx, w) + table[torch.arange(rows) % S]                 # one fp32 add per element
    td, _ = strided(table, H + 7, 3)
    od, obuf = strided(torch.zeros(rows, H), H + 5, 2)
    ops.embed_gather_fwd(w.cuda(), idx.cuda(), td, S, od)
    dd, _ = strided(d_out, H + 3, 1)
    dw = torch.full((N_EMBED, H), float("nan"), device="cuda")                  # every row must be written
    ops.embed_gather_bwd(dd, idx.cuda(), dw)
    torch.cuda.synchronize()
    assert torch.equal(od.cpu(), want) and outside_untouched(obuf, 2, H)
    dwc = dw.cpu()
    assert_close(dwc, wr.grad, 1e-5, 1e-6, f"embed_gather bwd H={H}")
    assert torch.equal(dwc[N_USED:], torch.zeros(N_EMBED - N_USED, H)), "rows never looked up get exactly 0"


@pytest.mark.parametrize("H", [40, 264])
def test_embed_gather_bwd_is_the_adjoint_of_the_clamped_fwd(ops, H):
    """<fwd(W), dy> = <W, bwd(dy)> in float64 for indices outside [0, n_embed): the forward clamps them (row 0 for
    negative indices, row n_embed - 1 past the end), so the backward must route their gradient to the same rows."""
    rows = 300
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(0, N_EMBED, (rows,), generator=g, dtype=torch.int64)
    idx[::7] = -1
    idx[3::11] = N_EMBED
    idx[5::13] = N_EMBED + 7
    w = rnd(N_EMBED, H, seed=12)
    dy = rnd(rows, H, seed=13)
    table = torch.zeros(1, H)                     # (the table's term is affine: left out, the gather is linear in W)
    out = torch.empty(rows, H, device="cuda")
    ops.embed_gather_fwd(w.cuda(), idx.cuda(), table.cuda(), 1, out)
    dw = torch.empty(N_EMBED, H, device="cuda")
    ops.embed_gather_bwd(dy.cuda(), idx.cuda(), dw)
    torch.cuda.synchronize()
    clamped = idx.clamp(0, N_EMBED - 1)
    assert torch.equal(out.cpu(), F.embedding(clamped, w))
    wr = w.double().requires_grad_(True)
    F.embedding(clamped, wr).backward(dy.double())
    assert_close(dw.cpu(), wr.grad, 1e-5, 1e-6, "embed_gather bwd vs the clamped lookup's adjoint")
    lhs = float((out.cpu().double() * dy.double()).sum())
    rhs = float((w.double() * dw.cpu().double()).sum())
    mag = float((out.cpu().double() * dy.double()).abs().sum())
    assert abs(lhs - rhs) <= 1e-6 * mag, (lhs, rhs, mag)


# ----------------------------------------------------------------------------------------------------------
# the attention core at Lq = Lk = S (both decoder attentions of the query models), operands as the engine lays them out
# ----------------------------------------------------------------------------------------------------------
PAD = 99


def _labels(B, S):
    """clip 0: one valid key (key 0); clip 1: every third key masked (never all); clips >= 2: nothing masked."""
    lab = torch.zeros(B, S, dtype=torch.int64)
    lab[0, 1:] = PAD
    if B > 1:
        lab[1, 2::3] = PAD
    return lab


@pytest.mark.parametrize("S,dh,heads,drop", [(1, 16, 8, False), (5, 4, 8, False), (9, 16, 8, False), (64, 16, 8, True),
                                             (65, 8, 4, False), (112, 8, 8, True), (8, 128, 2, True), (4, 256, 2, False)])
def test_mha_core_at_lq_equals_lk(ops, S, dh, heads, drop):
    B, H = 3, heads * dh
    qkv = rnd(B * S, 3 * H, seed=S * 7 + dh)              # self-attention's layout: q, k and v are slices of one [N, 3H] row
    lab = _labels(B, S)
    kpm = lab == PAD
    g = torch.Generator().manual_seed(5)
    keep = (torch.rand(B, heads, S, S, generator=g) > 0.1).to(torch.uint8) if drop else None
    dsc = 1 / 0.9 if drop else 1.0
    d_o = rnd(B * S, H, seed=3)
    qr = qkv.double().requires_grad_(True)
    qh = qr[:, :H].reshape(B, S, heads, dh).transpose(1, 2)
    kh = qr[:, H:2 * H].reshape(B, S, heads, dh).transpose(1, 2)
    vh = qr[:, 2 * H:].reshape(B, S, heads, dh).transpose(1, 2)
    att = ((qh @ kh.transpose(-2, -1)) / math.sqrt(dh)).masked_fill(kpm[:, None, None, :], float("-inf")).softmax(-1)
    attd = att * keep.double() * dsc if drop else att
    o = (attd @ vh).transpose(1, 2).reshape(B * S, H)
    o.backward(d_o.double())
    qd = qkv.cuda()
    probs = torch.empty(B, heads, S, S, device="cuda")
    od = torch.empty(B * S, H, device="cuda")
    kd = keep.cuda() if drop else None
    labd = lab.cuda()
    ops.mha_core_fwd(qd[:, :H], qd[:, H:2 * H], qd[:, 2 * H:], probs, od, B, heads, S, S, dh, key_labels=labd, pad_idx=PAD,
                     drop_mask=kd, drop_scale=dsc)
    dqkv = torch.empty(B * S, 3 * H, device="cuda")
    ops.mha_core_bwd(qd[:, :H], qd[:, H:2 * H], qd[:, 2 * H:], probs, d_o.cuda(), dqkv[:, :H], dqkv[:, H:2 * H],
                     dqkv[:, 2 * H:], B, heads, S, S, dh, drop_mask=kd, drop_scale=dsc)
    # key-label masking is the key-padding mask of the same keys, bit for bit
    probs_k = torch.empty_like(probs)
    od_k = torch.empty_like(od)
    ops.mha_core_fwd(qd[:, :H], qd[:, H:2 * H], qd[:, 2 * H:], probs_k, od_k, B, heads, S, S, dh,
                     kpm=kpm.to(torch.uint8).cuda(), drop_mask=kd, drop_scale=dsc)
    torch.cuda.synchronize()
    assert_close(probs.cpu(), att.detach(), 1e-4, 1e-6, "probs")
    assert bool((probs.cpu()[0, :, :, 1:] == 0).all()), "clip 0: every key but one masked"
    assert_close(od.cpu(), o.detach(), 1e-4, 1e-5, "attn out")
    assert_close(dqkv.cpu(), qr.grad, 1e-3, 1e-5, "dq, dk, dv")
    assert torch.equal(probs_k, probs) and torch.equal(od_k, od)


@pytest.mark.parametrize("H,heads,dh,last", QC.QUERY_BOUNDS)
def test_mha_core_refuses_one_past_the_training_bound_on_the_host(ops, H, heads, dh, last):
    """mha_core_supported agrees with the table at S = last and last + 1, and the backward at last + 1 returns an error from
    its host-side check (nothing is launched: mha_check runs before any launch)."""
    from r3d_amd._lib import R3DHipError
    if last:
        assert ops.mha_core_supported(last, last, dh, True) and ops.mha_core_supported(last, last, dh, False)
    S = last + 1
    assert not ops.mha_core_supported(S, S, dh, True)
    B, h = 1, 1
    q = torch.zeros(B * S, dh, device="cuda")
    probs = torch.zeros(B, h, S, S, device="cuda")
    g = [torch.zeros(B * S, dh, device="cuda") for _ in range(3)]
    with pytest.raises(R3DHipError, match="r3d_mha_core_bwd"):
        ops.mha_core_bwd(q, q, q, probs, q, g[0], g[1], g[2], B, h, S, S, dh)
    torch.cuda.synchronize()
    assert all(bool((t == 0).all()) for t in g), "the refused call wrote its outputs"
