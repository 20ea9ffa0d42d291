"""The row-wise kernels and the attention core at widths off the 64-column grid, against float64 torch restatements
(backward through autograd).  A row kernel's lane l owns columns l + 64 e, clamped to H - 1: at H % 64 != 0 a slot e is
only partly inside the row, so every sum must skip the clamped columns column by column (a mask on the slot passes every
multiple-of-64 width).  Widths cover each template bracket (<= 128, <= 512, <= 1024, <= 2048) with partly filled last
slots; the embedding seam also runs every slab-count stride of its vec4, wide and scalar branches."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.test_engine_gpu import close_rel  # noqa: E402

W = [24, 40, 72, 120, 128, 136, 200, 264, 504, 512, 520, 776, 1000, 1024]
W_WIDE = W + [1032, 1536, 2048]             # kernels whose widest instance is EPL 32 (layernorm, decoder tail)
EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def keep_mask(*shape, seed=0, p=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) > p).to(torch.uint8)


def chan_masks(H, seed):
    g = torch.Generator().manual_seed(seed)
    mr, md = torch.zeros(H), torch.zeros(H)
    mr[torch.randperm(H, generator=g)[:H // 4]] = 1
    md[torch.randperm(H, generator=g)[:H // 4]] = 1
    return mr, md


def ln64(x, g, b):
    return F.layer_norm(x, (x.shape[-1],), g, b, EPS)


def d(t):
    return None if t is None else t.cuda()


def dd(t):
    return t.double().requires_grad_(True)


# ----------------------------------------------------------------------------------------------------------
# embedding seam (embed.hip)
# ----------------------------------------------------------------------------------------------------------
SLABS = [(0, 1, False), (1, 3, True), (5, 4, True), (16, 15, False), (17, 16, True), (5, 17, True), (1, 61, True),
         (16, 64, False), (17, 65, True)]
EMBED_CASES = ([(H, 5, 61, True, False) for H in W] +
               [(H, nr, nd, drop, False) for H in (40, 120, 136, 200, 520, 776, 1000) for nr, nd, drop in SLABS] +
               [(H, nr, nd, True, True) for H in (120, 200, 776) for nr, nd in ((5, 61), (0, 17))])


def _slabs(ns, N, H, seed, misalign):
    """[ns, N, H] split-K slabs (a view one float past a 16-byte boundary when misalign: the scalar branch)."""
    x = rnd(ns * N * H, seed=seed, scale=0.5)
    buf = torch.zeros(ns * N * H + (1 if misalign else 0), device="cuda")
    v = buf[1:] if misalign else buf
    v.copy_(x.cuda())
    return v.view(ns, N, H), x.view(ns, N, H)


@pytest.mark.parametrize("H,ns_r,ns_d,drop,misalign", EMBED_CASES)
def test_embed_fuse_fwd_bwd(ops, H, ns_r, ns_d, drop, misalign):
    N = 16
    dsc = 1 / 0.9
    rg_d, rg = _slabs(max(ns_r, 1), N, H, 1, misalign)
    if ns_r == 0:
        rg_d, rg = rg_d[0], rg[0].relu()                    # a finished embedding (post ReLU)
        rg_d.copy_(rg.cuda())
    dp_d, dp = _slabs(ns_d, N, H, 2, misalign)
    br, bd_ = 0.1 * rnd(H, seed=3), 0.1 * rnd(H, seed=4)
    lg, lb = 1 + 0.2 * rnd(H, seed=5), 0.1 * rnd(H, seed=6)
    g1, b1 = 1 + 0.2 * rnd(H, seed=7), 0.1 * rnd(H, seed=8)
    mr, md = chan_masks(H, 9)
    keep = keep_mask(2 * N, H, seed=10) if drop else None
    kf = keep.double() * dsc if drop else torch.ones(2 * N, H, dtype=torch.float64)
    # float64 restatement
    r_pre = (rg.double().sum(0) + br.double()) if ns_r > 0 else rg.double()
    r = r_pre.relu() if ns_r > 0 else r_pre
    r = r.detach().requires_grad_(True)
    dpre = (dp.double().sum(0) + bd_.double()).detach().requires_grad_(True)
    lgd, lbd, g1d, b1d = dd(lg), dd(lb), dd(g1), dd(b1)
    dln = ln64(dpre, lgd, lbd)
    dep = dln.relu()
    ex_r = torch.where(mr.bool(), dep, r)
    ex_d = torch.where(md.bool(), r, dep)
    x0 = torch.stack([ex_r, ex_d], 1).reshape(2 * N, H) * kf
    h1 = ln64(x0, g1d, b1d)
    m1 = x0.mean(-1)
    r1 = 1 / torch.sqrt(x0.var(-1, unbiased=False) + EPS)
    # kernel
    f = lambda *s: torch.empty(*s, device="cuda")          # noqa: E731
    rgb_out = rg_d if ns_r == 0 else f(N, H)
    dep_pre, mean_d, rstd_d, dep_out, x0_k, h1_k, m1_k, r1_k = f(N, H), f(N), f(N), f(N, H), f(2 * N, H), f(2 * N, H), f(2 * N), f(2 * N)
    ops.embed_fuse_fwd(rg_d, ns_r, d(br), dp_d, ns_d, d(bd_), d(lg), d(lb), d(mr), d(md), d(keep), dsc,
                       d(g1), d(b1), rgb_out, dep_pre, mean_d, rstd_d, dep_out, x0_k, h1_k, m1_k, r1_k)
    torch.cuda.synchronize()
    tag = f"H{H} ns_r{ns_r} ns_d{ns_d} drop{int(drop)} mis{int(misalign)}"
    close_rel(rgb_out, r.detach(), f"{tag}: rgb", rtol=1e-5)
    close_rel(dep_pre, dpre.detach(), f"{tag}: dep_pre", rtol=1e-5)
    close_rel(mean_d, dpre.detach().mean(-1), f"{tag}: mean_d", rtol=1e-4)
    close_rel(rstd_d, 1 / torch.sqrt(dpre.detach().var(-1, unbiased=False) + EPS), f"{tag}: rstd_d", rtol=1e-4)
    close_rel(dep_out, dep.detach(), f"{tag}: dep", rtol=1e-4)
    close_rel(x0_k, x0.detach(), f"{tag}: x0", rtol=1e-4)
    close_rel(m1_k, m1.detach(), f"{tag}: m1", rtol=1e-4)
    close_rel(r1_k, r1.detach(), f"{tag}: r1", rtol=1e-4)
    close_rel(h1_k, h1.detach(), f"{tag}: h1", rtol=1e-4)
    # backward: d_h1 plus the two residual gradients added to norm1's input gradient (before embd_drop)
    dh1, a1, a2 = rnd(2 * N, H, seed=11), rnd(2 * N, H, seed=12), rnd(2 * N, H, seed=13)
    ((h1 * dh1.double()).sum() + (x0 * (a1 + a2).double()).sum()).backward()
    d_rgb_pre, d_dep_pre = f(N, H), f(N, H)
    ws_n1, ws_dep = f(N, 2, H), f(N, 2, H)
    ops.embed_fuse_bwd(d(dh1), x0_k, m1_k, r1_k, d(g1), d(a1), d(a2), d(keep), dsc, d(mr), d(md), rgb_out, dep_pre, mean_d,
                       rstd_d, d(lg), d(lb), d_rgb_pre, d_dep_pre, ws_n1, ws_dep)
    torch.cuda.synchronize()
    close_rel(d_rgb_pre, r.grad * (r.detach() > 0).double(), f"{tag}: d_rgb_pre", rtol=1e-3)
    close_rel(d_dep_pre, dpre.grad, f"{tag}: d_dep_pre", rtol=1e-3)
    close_rel(ws_n1.sum(0)[0], g1d.grad, f"{tag}: norm1 dgamma", rtol=1e-3)
    close_rel(ws_n1.sum(0)[1], b1d.grad, f"{tag}: norm1 dbeta", rtol=1e-3)
    close_rel(ws_dep.sum(0)[0], lgd.grad, f"{tag}: depth LN dgamma", rtol=1e-3)
    close_rel(ws_dep.sum(0)[1], lbd.grad, f"{tag}: depth LN dbeta", rtol=1e-3)


# ----------------------------------------------------------------------------------------------------------
# plain SA-Fuser seam (plainfuse.hip): the embedding seam with the modality token added instead of the exchange
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,ns_r,ns_d,drop,misalign", EMBED_CASES)
def test_plain_fuse_fwd_bwd(ops, H, ns_r, ns_d, drop, misalign):
    N = 16
    dsc = 1 / 0.9
    rg_d, rg = _slabs(max(ns_r, 1), N, H, 1, misalign)
    if ns_r == 0:
        rg_d, rg = rg_d[0], rg[0].relu()                    # a finished embedding (post ReLU)
        rg_d.copy_(rg.cuda())
    dp_d, dp = _slabs(ns_d, N, H, 2, misalign)
    br, bd_ = 0.1 * rnd(H, seed=3), 0.1 * rnd(H, seed=4)
    lg, lb = 1 + 0.2 * rnd(H, seed=5), 0.1 * rnd(H, seed=6)
    g1, b1 = 1 + 0.2 * rnd(H, seed=7), 0.1 * rnd(H, seed=8)
    tok = 0.3 * rnd(H, seed=9)
    keep = keep_mask(2 * N, H, seed=10) if drop else None
    kf = keep.double() * dsc if drop else torch.ones(2 * N, H, dtype=torch.float64)
    # float64 restatement: x0 = embd_drop([rgb; dep] + tok), rows 2n (rgb token) and 2n + 1 (depth token)
    r_pre = (rg.double().sum(0) + br.double()) if ns_r > 0 else rg.double()
    r = r_pre.relu() if ns_r > 0 else r_pre
    r = r.detach().requires_grad_(True)
    dpre = (dp.double().sum(0) + bd_.double()).detach().requires_grad_(True)
    lgd, lbd, g1d, b1d, tokd = dd(lg), dd(lb), dd(g1), dd(b1), dd(tok)
    dln = ln64(dpre, lgd, lbd)
    dep = dln.relu()
    t_r, t_d = r + tokd, dep + tokd
    x0 = torch.stack([t_r, t_d], 1).reshape(2 * N, H) * kf
    h1 = ln64(x0, g1d, b1d)
    m1 = x0.mean(-1)
    r1 = 1 / torch.sqrt(x0.var(-1, unbiased=False) + EPS)
    # kernel
    f = lambda *s: torch.empty(*s, device="cuda")          # noqa: E731
    rgb_out = rg_d if ns_r == 0 else f(N, H)
    dep_pre, mean_d, rstd_d, dep_out, x0_k, h1_k, m1_k, r1_k = f(N, H), f(N), f(N), f(N, H), f(2 * N, H), f(2 * N, H), f(2 * N), f(2 * N)
    ops.plain_fuse_fwd(rg_d, ns_r, d(br), dp_d, ns_d, d(bd_), d(lg), d(lb), d(tok), d(keep), dsc, d(g1), d(b1), rgb_out,
                       dep_pre, mean_d, rstd_d, dep_out, x0_k, h1_k, m1_k, r1_k)
    torch.cuda.synchronize()
    tag = f"plain H{H} ns_r{ns_r} ns_d{ns_d} drop{int(drop)} mis{int(misalign)}"
    close_rel(rgb_out, r.detach(), f"{tag}: rgb", rtol=1e-5)
    close_rel(dep_pre, dpre.detach(), f"{tag}: dep_pre", rtol=1e-5)
    close_rel(mean_d, dpre.detach().mean(-1), f"{tag}: mean_d", rtol=1e-4)
    close_rel(rstd_d, 1 / torch.sqrt(dpre.detach().var(-1, unbiased=False) + EPS), f"{tag}: rstd_d", rtol=1e-4)
    close_rel(dep_out, dep.detach(), f"{tag}: dep", rtol=1e-4)
    close_rel(x0_k, x0.detach(), f"{tag}: x0", rtol=1e-4)
    close_rel(m1_k, m1.detach(), f"{tag}: m1", rtol=1e-4)
    close_rel(r1_k, r1.detach(), f"{tag}: r1", rtol=1e-4)
    close_rel(h1_k, h1.detach(), f"{tag}: h1", rtol=1e-4)
    # backward: d_h1 plus the residual gradient added to norm1's input gradient (before embd_drop), given and None
    dh1, a1 = rnd(2 * N, H, seed=11), rnd(2 * N, H, seed=12)
    for add in (a1, None):
        obj = (h1 * dh1.double()).sum() + ((x0 * add.double()).sum() if add is not None else 0.0)
        wrt = (r, dpre, g1d, b1d, lgd, lbd, tokd, t_r, t_d)
        gr, gdp, gg1, gb1, glg, glb, gtok, gtr, gtd = torch.autograd.grad(obj, wrt, retain_graph=True)
        d_rgb_pre, d_dep_pre, t_tok = f(N, H), f(N, H), f(N, H)
        ws_n1, ws_dep = f(N, 2, H), f(N, 2, H)
        ops.plain_fuse_bwd(d(dh1), x0_k, m1_k, r1_k, d(g1), d(add), d(keep), dsc, rgb_out, dep_pre, mean_d, rstd_d, d(lg),
                           d(lb), d_rgb_pre, d_dep_pre, ws_n1, ws_dep, t_tok)
        # the t_tok-only mode (after the hidden-128 fuser chain): the same partials, bit for bit
        t_only = torch.full((N, H), float("nan"), device="cuda")
        ops.plain_fuse_bwd(d(dh1), x0_k, m1_k, r1_k, d(g1), d(add), d(keep), dsc, None, None, None, None, None, None, None,
                           None, None, None, t_only)
        torch.cuda.synchronize()
        tg = f"{tag} add1{int(add is not None)}"
        close_rel(d_rgb_pre, gr * (r.detach() > 0).double(), f"{tg}: d_rgb_pre", rtol=1e-3)
        close_rel(d_dep_pre, gdp, f"{tg}: d_dep_pre", rtol=1e-3)
        close_rel(ws_n1.sum(0)[0], gg1, f"{tg}: norm1 dgamma", rtol=1e-3)
        close_rel(ws_n1.sum(0)[1], gb1, f"{tg}: norm1 dbeta", rtol=1e-3)
        close_rel(ws_dep.sum(0)[0], glg, f"{tg}: depth LN dgamma", rtol=1e-3)
        close_rel(ws_dep.sum(0)[1], glb, f"{tg}: depth LN dbeta", rtol=1e-3)
        close_rel(t_tok, gtr + gtd, f"{tg}: t_tok (per frame)", rtol=1e-3)
        close_rel(t_tok.double().sum(0), gtok, f"{tg}: d modality_token (column sum of t_tok)", rtol=1e-3)
        assert torch.equal(t_only, t_tok), f"{tg}: t_tok-only mode differs from the full mode"


def test_plain_fuse_refuses_a_row_past_its_seam_before_any_launch(ops, monkeypatch):
    N, H = 4, 1032
    f = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731

    def launched(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops._lib, "load", launched)
    v, rows, rows2 = f(H), f(N, H), f(2 * N, H)
    with pytest.raises(ValueError, match="plain fuser"):
        ops.plain_fuse_fwd(rows, 0, v, rows, 1, v, v, v, v, None, 1.0, v, v, f(N, H), f(N, H), f(N), f(N), f(N, H), f(2 * N, H),
                           f(2 * N, H), f(2 * N), f(2 * N))
    with pytest.raises(ValueError, match="plain fuser"):
        ops.plain_fuse_bwd(rows2, rows2, f(2 * N), f(2 * N), v, None, None, 1.0, rows, rows, f(N), f(N), v, v, f(N, H),
                           f(N, H), f(N, 2, H), f(N, 2, H), f(N, H))
    with pytest.raises(ValueError, match="plain fuser"):
        ops.plain_fuse_bwd(rows2, rows2, f(2 * N), f(2 * N), v, None, None, 1.0, None, None, None, None, None, None, None,
                           None, None, None, f(N, H))


# ----------------------------------------------------------------------------------------------------------
# decoder tail (tail.hip): norm3 -> decoder.norm -> heads, and its adjoint
# ----------------------------------------------------------------------------------------------------------
TAIL_SHAPES = [(1, 1), (6, 3), (7, 61), (18, 1000), (24, 3), (25, 61), (123, 1000)]        # (n_head, rows)


@pytest.mark.parametrize("H", W_WIDE)
@pytest.mark.parametrize("n_head,rows", TAIL_SHAPES)
def test_decoder_tail_fwd_bwd(ops, H, n_head, rows):
    ld = n_head + 3                                        # ld_out > n_head
    x = rnd(rows, H, seed=1)
    g3, b3, gF, bF = 1 + 0.2 * rnd(H, seed=2), 0.1 * rnd(H, seed=3), 1 + 0.2 * rnd(H, seed=4), 0.1 * rnd(H, seed=5)
    wh, bh = rnd(n_head, H, seed=6, scale=H ** -0.5), 0.1 * rnd(n_head, seed=7)
    keep = keep_mask(rows, H, seed=8)
    dsc = 1 / 0.9
    xd, g3d, b3d, gFd, bFd = dd(x), dd(g3), dd(b3), dd(gF), dd(bF)
    t3 = ln64(xd, g3d, b3d)
    tF = ln64(t3, gFd, bFd)
    out = tF @ wh.double().t() + bh.double()
    dout = rnd(rows, n_head, seed=9)
    out.backward(dout.double())
    f = lambda *s: torch.empty(*s, device="cuda")          # noqa: E731
    t3k, m3, r3, tFk, mF, rF = f(rows, H), f(rows), f(rows), f(rows, H), f(rows), f(rows)
    outk = torch.full((rows, ld), 7.0, device="cuda")
    ops.decoder_tail_fwd(d(x), d(g3), d(b3), d(gF), d(bF), d(wh), d(bh), t3k, m3, r3, tFk, mF, rF, outk)
    torch.cuda.synchronize()
    tag = f"H{H} n_head{n_head} rows{rows}"
    close_rel(t3k, t3.detach(), f"{tag}: t3", rtol=1e-4)
    close_rel(tFk, tF.detach(), f"{tag}: tgtF", rtol=1e-4)
    close_rel(outk[:, :n_head], out.detach(), f"{tag}: out", rtol=1e-4)
    assert bool((outk[:, n_head:] == 7.0).all()), f"{tag}: wrote past n_head"
    close_rel(m3, x.double().mean(-1), f"{tag}: m3", rtol=1e-4)
    close_rel(rF, 1 / torch.sqrt(t3.detach().var(-1, unbiased=False) + EPS), f"{tag}: rF", rtol=1e-4)
    dld = torch.zeros(rows, ld)
    dld[:, :n_head] = dout
    dld[:, n_head:] = 1e3                                  # columns past n_head must not be read
    dx, dx2 = f(rows, H), f(rows, H)
    dgF, dbF, dg3, db3 = f(H), f(H), f(H), f(H)
    nws = max(ops.layernorm_bwd_ws_floats(rows, H), 4)
    wsF, ws3 = f(nws), f(nws)
    ops.decoder_tail_bwd(d(dld), d(wh), t3k, mF, rF, d(gF), d(x), m3, r3, d(g3), d(keep), dsc, dx, dx2, dgF, dbF, dg3, db3,
                         wsF, ws3)
    rpb = max(4, (-(-rows // 256) + 3) // 4 * 4)
    if -(-rows // rpb) > 1:                                # partial (dgamma, dbeta) per block: finalize as the engine does
        ops.layernorm_bwd_finalize(wsF, rows, H, dgF, dbF)
        ops.layernorm_bwd_finalize(ws3, rows, H, dg3, db3)
    torch.cuda.synchronize()
    close_rel(dx, xd.grad, f"{tag}: dx", rtol=1e-3)
    close_rel(dx2, xd.grad * keep.double() * dsc, f"{tag}: dx2", rtol=1e-3)
    for got, ref, nm in ((dgF, gFd.grad, "dgF"), (dbF, bFd.grad, "dbF"), (dg3, g3d.grad, "dg3"), (db3, b3d.grad, "db3")):
        close_rel(got, ref, f"{tag}: {nm}", rtol=1e-3)


# ----------------------------------------------------------------------------------------------------------
# LayerNorm (rowops.hip) off the grid: the bounds of tests/test_kernels_gpu.py::test_layernorm_fwd_bwd
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", W_WIDE)
@pytest.mark.parametrize("rows", [3, 70])
@pytest.mark.parametrize("relu", [False, True])
def test_layernorm_off_grid(ops, rows, H, relu):
    from tests.test_kernels_gpu import test_layernorm_fwd_bwd
    test_layernorm_fwd_bwd(ops, rows, H, relu)


# ----------------------------------------------------------------------------------------------------------
# token exchange at hidden > 1024 (the un-seamed route)
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1032, 1536, 2048, 136, 520])
def test_token_exchange_wide(ops, H):
    N = 13
    rgb, dep = rnd(N, H, seed=1).relu(), rnd(N, H, seed=2).relu()
    mr, md = chan_masks(H, 3)
    keep = keep_mask(2 * N, H, seed=4)
    x0 = torch.empty(2 * N, H, device="cuda")
    ops.token_exchange_fwd(d(rgb), d(dep), d(mr), d(md), x0, drop_mask=d(keep), drop_scale=1 / 0.9)
    r, dp = dd(rgb), dd(dep)
    st = torch.stack([torch.where(mr.bool(), dp, r), torch.where(md.bool(), r, dp)], 1).reshape(2 * N, H) * keep.double() / 0.9
    dx0 = rnd(2 * N, H, seed=5)
    st.backward(dx0.double())
    drp, ddp = torch.empty(N, H, device="cuda"), torch.empty(N, H, device="cuda")
    ops.token_exchange_bwd(d(dx0), d(rgb), d(mr), d(md), drp, ddp, drop_mask=d(keep), drop_scale=1 / 0.9)
    torch.cuda.synchronize()
    close_rel(x0, st.detach(), f"H{H}: x0", rtol=1e-6)
    close_rel(drp, r.grad * (rgb > 0).double(), f"H{H}: d_rgb_pre", rtol=1e-6)
    close_rel(ddp, dp.grad, f"H{H}: d_dep", rtol=1e-6)


# ----------------------------------------------------------------------------------------------------------
# attention core: general path at odd head widths and long key counts, and the largest admitted Lk
# ----------------------------------------------------------------------------------------------------------
def _mha(ops, B, heads, Lq, Lk, dh, seed, drop=True):
    H = heads * dh
    q, kv = rnd(B * Lq, H, seed=seed), rnd(B * Lk, 2 * H, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    kpm = (torch.rand(B, Lk, generator=g) < 0.3).to(torch.uint8)
    kpm[:, 0] = 0                                          # at least one key per clip
    if Lk > 1:
        kpm[0, Lk // 2:] = 1                               # one clip padded past its middle
    keep = keep_mask(B, heads, Lq, Lk, seed=seed + 3) if drop else None
    dsc = 1 / 0.9 if drop else 1.0
    d_o = rnd(B * Lq, H, seed=seed + 4)
    qr, kvr = dd(q), dd(kv)
    qh = qr.view(B, Lq, heads, dh).transpose(1, 2)
    kh = kvr[:, :H].reshape(B, Lk, heads, dh).transpose(1, 2)
    vh = kvr[:, H:].reshape(B, Lk, heads, dh).transpose(1, 2)
    att = ((qh @ kh.transpose(-2, -1)) / math.sqrt(dh)).masked_fill(kpm.bool()[:, None, None, :], float("-inf")).softmax(-1)
    attd = att * keep.double() * dsc if drop else att
    o = (attd @ vh).transpose(1, 2).reshape(B * Lq, H)
    o.backward(d_o.double())
    qd, kvd = d(q), d(kv)
    probs, od = torch.empty(B, heads, Lq, Lk, device="cuda"), torch.empty(B * Lq, H, device="cuda")
    ops.mha_core_fwd(qd, kvd[:, :H], kvd[:, H:], probs, od, B, heads, Lq, Lk, dh, kpm=d(kpm), drop_mask=d(keep), drop_scale=dsc)
    dq, dkv = torch.empty(B * Lq, H, device="cuda"), torch.empty(B * Lk, 2 * H, device="cuda")
    ops.mha_core_bwd(qd, kvd[:, :H], kvd[:, H:], probs, d(d_o), dq, dkv[:, :H], dkv[:, H:], B, heads, Lq, Lk, dh,
                     drop_mask=d(keep), drop_scale=dsc)
    torch.cuda.synchronize()
    tag = f"B{B} heads{heads} Lk{Lk} dh{dh}"
    close_rel(probs, att.detach(), f"{tag}: probs", rtol=1e-4)
    close_rel(od, o.detach(), f"{tag}: out", rtol=1e-4)
    close_rel(dq, qr.grad, f"{tag}: dq", rtol=1e-3)
    close_rel(dkv, kvr.grad, f"{tag}: dkv", rtol=1e-3)


@pytest.mark.parametrize("dh", [5, 12, 17, 25, 65, 86])
@pytest.mark.parametrize("Lk", [1, 63, 64, 65, 257, 1000])
def test_mha_core_general_path(ops, dh, Lk):
    _mha(ops, 2, 3, 8, Lk, dh, seed=dh * 7 + Lk)


@pytest.mark.parametrize("dh", [16, 64, 128])
def test_mha_core_at_the_largest_admitted_key_count(ops, dh):
    from r3d_amd import engine as E
    Lk = E.max_clip_len(8 * dh, 8, 8, 10 ** 5, True)
    assert ops.mha_core_supported(8, Lk, dh, True) and not ops.mha_core_supported(8, Lk + 1, dh, True)
    _mha(ops, 2, 2, 8, Lk, dh, seed=dh)


@pytest.mark.parametrize("dh", [16, 64, 128])
def test_mha_core_forward_at_the_largest_forward_only_key_count(ops, dh):
    """A forward alone (validation) needs less LDS than the backward: its own bound is larger."""
    from r3d_amd import engine as E
    Lk = E.max_clip_len(8 * dh, 8, 8, 10 ** 5, False)
    assert Lk > E.max_clip_len(8 * dh, 8, 8, 10 ** 5, True)
    assert ops.mha_core_supported(8, Lk, dh, False) and not ops.mha_core_supported(8, Lk + 1, dh, False)
    B, heads, Lq = 2, 2, 8
    H = heads * dh
    q, kv = rnd(B * Lq, H, seed=dh), rnd(B * Lk, 2 * H, seed=dh + 1)
    kpm = torch.zeros(B, Lk, dtype=torch.uint8)
    kpm[1, Lk // 3:] = 1
    qh = q.double().view(B, Lq, heads, dh).transpose(1, 2)
    kh = kv[:, :H].double().reshape(B, Lk, heads, dh).transpose(1, 2)
    vh = kv[:, H:].double().reshape(B, Lk, heads, dh).transpose(1, 2)
    att = ((qh @ kh.transpose(-2, -1)) / math.sqrt(dh)).masked_fill(kpm.bool()[:, None, None, :], float("-inf")).softmax(-1)
    o = (att @ vh).transpose(1, 2).reshape(B * Lq, H)
    kvd = d(kv)
    probs, od = torch.empty(B, heads, Lq, Lk, device="cuda"), torch.empty(B * Lq, H, device="cuda")
    ops.mha_core_fwd(d(q), kvd[:, :H], kvd[:, H:], probs, od, B, heads, Lq, Lk, dh, kpm=d(kpm))
    torch.cuda.synchronize()
    close_rel(probs, att, f"fwd-only Lk{Lk} dh{dh}: probs", rtol=1e-4)
    close_rel(od, o, f"fwd-only Lk{Lk} dh{dh}: out", rtol=1e-4)


# ----------------------------------------------------------------------------------------------------------
# BN-blend seam (bnfuse.hip): statistics, blend + norm1, its adjoint, the BatchNorm input gradients
# ----------------------------------------------------------------------------------------------------------
def _alpha(C, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + 0.45 * torch.rand(C, generator=g)).float()


@pytest.mark.parametrize("C", W)
@pytest.mark.parametrize("training", [True, False])
def test_bn_seam_fwd_bwd(ops, C, training):
    N, eps, mom, dsc = 24, 1e-5, 0.1, 1 / 0.9
    rgb, dep = rnd(N, C, seed=1).relu(), rnd(N, C, seed=2, scale=0.7) + 0.3
    g_r, b_r, g_d, b_d = 1 + 0.3 * rnd(C, seed=3), 0.1 * rnd(C, seed=4), 1 + 0.3 * rnd(C, seed=5), 0.1 * rnd(C, seed=6)
    al, g1, b1 = _alpha(C, 7), 1 + 0.2 * rnd(C, seed=8), 0.1 * rnd(C, seed=9)
    rm = [0.1 * rnd(C, seed=10), 0.1 * rnd(C, seed=11)]
    rv = [1 + 0.2 * rnd(C, seed=12).abs(), 1 + 0.2 * rnd(C, seed=13).abs()]
    mods = []
    for t, gam in enumerate((g_r, g_d)):
        m = torch.nn.BatchNorm1d(C, momentum=mom).cuda()
        with torch.no_grad():
            m.weight.copy_(gam.cuda())
            m.running_mean.copy_(rm[t].cuda())
            m.running_var.copy_(rv[t].cuda())
        mods.append(m)
    mr, md = chan_masks(C, 14)
    keep = keep_mask(2 * N, C, seed=15)
    # float64 restatement (futr_safuser_batchnormalization.py: BatchNorm1d, alpha blend on the selected channels)
    r, dp = dd(rgb), dd(dep)
    g_rd, b_rd, g_dd, b_dd, ald, g1d, b1d = dd(g_r), dd(b_r), dd(g_d), dd(b_d), dd(al), dd(g1), dd(b1)

    def bn(x, t, g, b):
        if training:
            mu, var = x.mean(0), x.var(0, unbiased=False)
        else:
            mu, var = rm[t].double(), rv[t].double()
        return (x - mu) / torch.sqrt(var + eps) * g + b, mu, var
    rb, mu_r, var_r = bn(r, 0, g_rd, b_rd)
    db, mu_d, var_d = bn(dp, 1, g_dd, b_dd)
    ex_r = torch.where(mr.bool(), ald * rb + (1 - ald) * db, rb)
    ex_d = torch.where(md.bool(), ald * db + (1 - ald) * rb, db)
    x0 = torch.stack([ex_r, ex_d], 1).reshape(2 * N, C) * keep.double() * dsc
    h1 = ln64(x0, g1d, b1d)
    dh1, a1 = rnd(2 * N, C, seed=16), rnd(2 * N, C, seed=17)
    ((h1 * dh1.double()).sum() + (x0 * a1.double()).sum()).backward()
    # kernels
    f = lambda *s: torch.empty(*s, device="cuda")          # noqa: E731
    mean, rstd, absg = f(2, C), f(2, C), f(2, C)
    rgb_d, dep_d = d(rgb), d(dep)
    ops.bn_stats(rgb_d, dep_d, mods[0], mods[1], mean, rstd, absg, training, mom)
    x0k, h1k, m1k, r1k = f(2 * N, C), f(2 * N, C), f(2 * N), f(2 * N)
    ops.bn_blend_fwd(rgb_d, dep_d, mean, rstd, d(g_r), d(b_r), d(g_d), d(b_d), d(al), d(mr), d(md), d(keep), dsc, d(g1), d(b1),
                     x0k, h1k, m1k, r1k)
    terms = [f(N, C) for _ in range(5)]
    ws_n1 = f(N, 2, C)
    ops.bn_blend_bwd(d(dh1), x0k, m1k, r1k, d(g1), d(a1), d(keep), dsc, rgb_d, dep_d, mean, rstd, d(g_r), d(b_r), d(g_d),
                     d(b_d), d(al), d(mr), d(md), *terms, ws_n1)
    t_drb, t_drbx, t_ddb, t_ddbx, t_dal = terms
    sums = [t.sum(0) for t in terms]
    d_rgb_pre, d_dep = f(N, C), f(N, C)
    ops.bn_bwd_apply(rgb_d, dep_d, mean, rstd, d(g_r), d(g_d), t_drb, t_ddb, sums[1], sums[0], sums[3], sums[2], d_rgb_pre, d_dep,
                     training)
    torch.cuda.synchronize()
    tag = f"C{C} training{int(training)}"
    close_rel(mean, torch.stack([mu_r, mu_d]).detach(), f"{tag}: mean", rtol=1e-5)
    close_rel(rstd, 1 / torch.sqrt(torch.stack([var_r, var_d]).detach() + eps), f"{tag}: rstd", rtol=1e-4)
    assert torch.equal(absg.cpu(), torch.stack([g_r, g_d]).abs()), tag
    for t, (mu, x) in enumerate(((mu_r, rgb), (mu_d, dep))):
        want_m = (1 - mom) * rm[t].double() + mom * mu.detach() if training else rm[t].double()
        want_v = ((1 - mom) * rv[t].double() + mom * x.double().var(0, unbiased=True)) if training else rv[t].double()
        close_rel(mods[t].running_mean, want_m, f"{tag}: running_mean {t}", rtol=1e-5)
        close_rel(mods[t].running_var, want_v, f"{tag}: running_var {t}", rtol=1e-5)
        assert int(mods[t].num_batches_tracked) == (1 if training else 0), tag
    close_rel(x0k, x0.detach(), f"{tag}: x0", rtol=1e-4)
    close_rel(m1k, x0.detach().mean(-1), f"{tag}: m1", rtol=1e-4)
    close_rel(r1k, 1 / torch.sqrt(x0.detach().var(-1, unbiased=False) + EPS), f"{tag}: r1", rtol=1e-4)
    close_rel(h1k, h1.detach(), f"{tag}: h1", rtol=1e-4)
    for got, ref, nm in ((sums[0], b_rd.grad, "d beta_rgb"), (sums[1], g_rd.grad, "d gamma_rgb"), (sums[2], b_dd.grad, "d beta_dep"),
                         (sums[3], g_dd.grad, "d gamma_dep"), (sums[4], ald.grad, "d alpha"),
                         (ws_n1.sum(0)[0], g1d.grad, "norm1 dgamma"), (ws_n1.sum(0)[1], b1d.grad, "norm1 dbeta")):
        close_rel(got, ref, f"{tag}: {nm}", rtol=1e-3)
    close_rel(d_rgb_pre, r.grad * (rgb > 0).double(), f"{tag}: d_rgb_pre", rtol=1e-3)
    close_rel(d_dep, dp.grad, f"{tag}: d_dep", rtol=1e-3)


# ----------------------------------------------------------------------------------------------------------
# activation-magnitude seam (varyfuse.hip): scaled exchange + norm1, and its adjoint
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", W)
@pytest.mark.parametrize("with_ws", [True, False])
def test_scaled_exchange_fwd_bwd(ops, C, with_ws):
    N, dsc = 20, 1 / 0.9
    rgb, dep = rnd(N, C, seed=1).relu(), rnd(N, C, seed=2).relu()
    al, g1, b1 = _alpha(C, 3), 1 + 0.2 * rnd(C, seed=4), 0.1 * rnd(C, seed=5)
    mr, md = chan_masks(C, 6)
    keep = keep_mask(2 * N, C, seed=7)
    r, dp, ald, g1d, b1d = dd(rgb), dd(dep), dd(al), dd(g1), dd(b1)
    ex_r = torch.where(mr.bool(), ald * dp, r)
    ex_d = torch.where(md.bool(), ald * r, dp)
    x0 = torch.stack([ex_r, ex_d], 1).reshape(2 * N, C) * keep.double() * dsc
    h1 = ln64(x0, g1d, b1d)
    dh1, a1 = rnd(2 * N, C, seed=8), rnd(2 * N, C, seed=9)
    ((h1 * dh1.double()).sum() + (x0 * a1.double()).sum()).backward()
    f = lambda *s: torch.empty(*s, device="cuda")          # noqa: E731
    x0k, h1k, m1k, r1k = f(2 * N, C), f(2 * N, C), f(2 * N), f(2 * N)
    rgb_d, dep_d = d(rgb), d(dep)
    ops.scaled_exchange_fwd(rgb_d, dep_d, d(mr), d(md), d(al), d(keep), dsc, d(g1), d(b1), x0k, h1k, m1k, r1k)
    d_rgb_pre, d_dep, t_dal = f(N, C), f(N, C), f(N, C)
    ws_n1 = f(N, 2, C) if with_ws else None
    ops.scaled_exchange_bwd(d(dh1), x0k, m1k, r1k, d(g1), d(a1), d(keep), dsc, rgb_d, dep_d, d(mr), d(md), d(al), d_rgb_pre,
                            d_dep, t_dal, ws_n1)
    torch.cuda.synchronize()
    tag = f"C{C} ws{int(with_ws)}"
    close_rel(x0k, x0.detach(), f"{tag}: x0", rtol=1e-5)
    close_rel(m1k, x0.detach().mean(-1), f"{tag}: m1", rtol=1e-4)
    close_rel(r1k, 1 / torch.sqrt(x0.detach().var(-1, unbiased=False) + EPS), f"{tag}: r1", rtol=1e-4)
    close_rel(h1k, h1.detach(), f"{tag}: h1", rtol=1e-4)
    close_rel(d_rgb_pre, r.grad * (rgb > 0).double(), f"{tag}: d_rgb_pre", rtol=1e-3)
    close_rel(d_dep, dp.grad, f"{tag}: d_dep", rtol=1e-3)
    close_rel(t_dal.sum(0), ald.grad, f"{tag}: d alpha", rtol=1e-3)
    if with_ws:
        close_rel(ws_n1.sum(0)[0], g1d.grad, f"{tag}: norm1 dgamma", rtol=1e-3)
        close_rel(ws_n1.sum(0)[1], b1d.grad, f"{tag}: norm1 dbeta", rtol=1e-3)


# ----------------------------------------------------------------------------------------------------------
# the training step's tail forward + 3 losses + tail backward as ONE launch (losses.hip): up to hidden 512, including the
# dynamic-LDS widths 129-512, against float64 and against the three launches it replaces
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [h for h in W if h <= 512])
@pytest.mark.parametrize("B,S,K", [(2, 16, 17), (3, 7, 23), (16, 5, 17)])
def test_decoder_tail_losses_one_launch(ops, H, B, S, K):
    from oracle import futr_oracle as O, synth
    Q, pad = 8, K + 1
    rows, N, nh = B * Q, B * S, K + 1
    assert ops.tail_losses_supported(H, nh, Q, rows)
    _, _, lab, dur, tgt = [torch.from_numpy(x) for x in synth.make_batch(B, S, K, pad, 5, depth_hw=(4, 4))]
    x = rnd(rows, H, seed=1)
    g3, b3, gF, bF = 1 + 0.2 * rnd(H, seed=2), 0.1 * rnd(H, seed=3), 1 + 0.2 * rnd(H, seed=4), 0.1 * rnd(H, seed=5)
    wh, bh = rnd(nh, H, seed=6, scale=H ** -0.5), 0.1 * rnd(nh, seed=7)
    seg = rnd(N, K, seed=8)
    keep = keep_mask(rows, H, seed=9)
    dsc = 1 / 0.9
    # float64: the tail, the reference's loss composition, autograd
    xd, g3d, b3d, gFd, bFd, segd = dd(x), dd(g3), dd(b3), dd(gF), dd(bF), dd(seg)
    out = ln64(ln64(xd, g3d, b3d), gFd, bFd) @ wh.double().t() + bh.double()
    res = O.losses(dict(seg=segd.view(B, S, K), action=out[:, :K].reshape(B, Q, K), duration=out[:, K].reshape(B, Q)),
                   lab, dur.double(), tgt, pad)
    res["loss"].backward()
    want_loss = torch.stack([res[k].detach() for k in ("loss_seg", "loss_action", "loss_dur", "loss")])
    want_counts = [int(res[k]) for k in ("seg_correct", "seg_total", "act_correct", "act_total")]
    f = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731
    nws = max(ops.layernorm_bwd_ws_floats(rows, H), 4)
    labd, tgtd, durd = d(lab), d(tgt), d(dur)

    def run(one):
        o = dict(t3=f(rows, H), m3=f(rows), r3=f(rows), tgtF=f(rows, H), mF=f(rows), rF=f(rows), out=f(rows, nh),
                 d_seg=f(N, K), d_out=f(rows, nh), loss=f(4), counts=torch.zeros(4, dtype=torch.int64, device="cuda"),
                 dx=f(rows, H), dx2=f(rows, H), wsF=f(nws), ws3=f(nws), dgF=f(H), dbF=f(H), dg3=f(H), db3=f(H))
        ws = f(ops.losses_ws_floats(B, S, Q))
        tail = dict(x=d(x), g3=d(g3), b3=d(b3), gF=d(gF), bF=d(bF), w_head=d(wh), b_head=d(bh), t3=o["t3"], m3=o["m3"],
                    r3=o["r3"], tgtF=o["tgtF"], mF=o["mF"], rF=o["rF"], out=o["out"])
        if one:
            ops.decoder_tail_losses(**tail, seg=d(seg), past_label=labd, target=tgtd, target_dur=durd, B=B, S=S, Q=Q, K=K,
                                    pad_idx=pad, exclude_idx=47, dur_den=None, grad_scale=1.0, d_seg=o["d_seg"],
                                    d_out=o["d_out"], loss_out=o["loss"], counts=o["counts"], tick_a=None, tick_b=None,
                                    drop=d(keep), drop_scale=dsc, dx=o["dx"], dx2=o["dx2"], wsF=o["wsF"], ws3=o["ws3"], ws=ws)
            ops.layernorm_bwd_finalize(o["wsF"], rows, H, o["dgF"], o["dbF"])
            ops.layernorm_bwd_finalize(o["ws3"], rows, H, o["dg3"], o["db3"])
        else:
            ops.decoder_tail_fwd(*tail.values())
            ops.losses_fwd_bwd(d(seg), o["out"][:, :K], o["out"][:, K:], nh, labd, tgtd, durd, B, S, Q, K, pad, 47, o["loss"],
                               o["counts"], d_seg=o["d_seg"], d_act=o["d_out"][:, :K], d_dur=o["d_out"][:, K:], ld_ddur=nh,
                               ws=ws)
            ops.decoder_tail_bwd(o["d_out"], d(wh), o["t3"], o["mF"], o["rF"], d(gF), d(x), o["m3"], o["r3"], d(g3), d(keep),
                                 dsc, o["dx"], o["dx2"], o["dgF"], o["dbF"], o["dg3"], o["db3"], o["wsF"], o["ws3"])
            rpb = max(4, (-(-rows // 256) + 3) // 4 * 4)
            if -(-rows // rpb) > 1:
                ops.layernorm_bwd_finalize(o["wsF"], rows, H, o["dgF"], o["dbF"])
                ops.layernorm_bwd_finalize(o["ws3"], rows, H, o["dg3"], o["db3"])
        torch.cuda.synchronize()
        return o
    one, three = run(True), run(False)
    tag = f"H{H} B{B} S{S} K{K}"
    for o, route in ((one, "one launch"), (three, "three launches")):
        t = f"{tag} {route}"
        close_rel(o["out"], out.detach(), f"{t}: out", rtol=1e-4)
        assert torch.allclose(o["loss"].cpu().double(), want_loss, rtol=1e-4, atol=1e-6), (t, o["loss"].cpu(), want_loss)
        assert o["counts"].cpu().tolist() == want_counts, t
        close_rel(o["d_seg"], segd.grad, f"{t}: d_seg", rtol=1e-3)
        close_rel(o["dx"], xd.grad, f"{t}: dx", rtol=1e-3)
        close_rel(o["dx2"], xd.grad * keep.double() * dsc, f"{t}: dx2", rtol=1e-3)
        for nm, ref in (("dgF", gFd.grad), ("dbF", bFd.grad), ("dg3", g3d.grad), ("db3", b3d.grad)):
            close_rel(o[nm], ref, f"{t}: {nm}", rtol=1e-3)
    for k in ("out", "loss", "d_seg", "d_out", "dx", "dx2", "dgF", "dbF", "dg3", "db3"):
        close_rel(one[k], three[k].double(), f"{tag}: one launch vs three, {k}", rtol=1e-5)
    assert torch.equal(one["counts"], three["counts"]), tag


# ----------------------------------------------------------------------------------------------------------
# the four seams' optional operands (seam_rows.h): absent = present and neutral
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [40, 136, 520])              # a partly filled last slot in each of the EPL 2 / 8 / 16 brackets
def test_seam_absent_operand_equals_a_neutral_one(ops, H):
    """A residual gradient (add1, add2) left out must give what an all-zero one gives, and a keep mask left out what an
    all-ones mask with drop_scale 1 gives, output for output (torch.equal: -0.0 == 0.0 is intended), for the four backward
    seams and the forward seams that take the mask."""
    N = 3
    f = lambda *s: torch.full(s, float("nan"), device="cuda")          # noqa: E731
    rgb, dep = d(rnd(N, H, seed=1).relu()), d(rnd(N, H, seed=2).relu())
    dpre = d(rnd(N, H, seed=3))
    lg, lb, g1, b1 = d(1 + 0.2 * rnd(H, seed=4)), d(0.1 * rnd(H, seed=5)), d(1 + 0.2 * rnd(H, seed=6)), d(0.1 * rnd(H, seed=7))
    mr, md = (d(m) for m in chan_masks(H, 8))
    tok, al = d(0.3 * rnd(H, seed=9)), d(_alpha(H, 10))
    dh1 = d(rnd(2 * N, H, seed=11))
    zeros, ones = torch.zeros(2 * N, H, device="cuda"), torch.ones(2 * N, H, dtype=torch.uint8, device="cuda")
    mean, rstd = d(0.1 * rnd(2, H, seed=12)), d(1 + 0.2 * rnd(2, H, seed=13).abs())
    bn = [d(1 + 0.3 * rnd(H, seed=14)), d(0.1 * rnd(H, seed=15)), d(1 + 0.3 * rnd(H, seed=16)), d(0.1 * rnd(H, seed=17))]

    def same(name, call, n_out, variants):
        """call(outs, *operands) for each operand tuple of `variants`; every output must equal the first tuple's."""
        got = []
        for v in variants:
            outs = [f(*s) for s in n_out]
            call(outs, *v)
            torch.cuda.synchronize()
            got.append(outs)
        for v, outs in zip(variants[1:], got[1:]):
            for i, (a, b) in enumerate(zip(got[0], outs)):
                assert not torch.isnan(a).any(), f"H{H} {name}: output {i} not fully written"
                assert torch.equal(a, b), f"H{H} {name}: output {i} differs with {[None if t is None else 'given' for t in v]}"
        return got[0]

    rows, fr, pf = (2 * N, H), (N, H), (N,)
    fwd_out = [fr, fr, pf, pf, fr, rows, rows, (2 * N,), (2 * N,)]          # rgb_out dep_pre mean_d rstd_d dep_out x0 h1 m1 r1
    drops = [(None, 1.0), (ones, 1.0)]
    e_f = same("embed_fuse_fwd", lambda o, dm, sc: ops.embed_fuse_fwd(rgb, 0, None, dpre.view(1, N, H), 1, None, lg, lb, mr, md,
                                                                       dm, sc, g1, b1, *o), fwd_out, drops)
    p_f = same("plain_fuse_fwd", lambda o, dm, sc: ops.plain_fuse_fwd(rgb, 0, None, dpre.view(1, N, H), 1, None, lg, lb, tok,
                                                                       dm, sc, g1, b1, *o), fwd_out, drops)
    row_out = [rows, rows, (2 * N,), (2 * N,)]                              # x0 h1 m1 r1
    v_f = same("scaled_exchange_fwd", lambda o, dm, sc: ops.scaled_exchange_fwd(rgb, dep, mr, md, al, dm, sc, g1, b1, *o),
               row_out, drops)
    b_f = same("bn_blend_fwd", lambda o, dm, sc: ops.bn_blend_fwd(rgb, dep, mean, rstd, *bn, al, mr, md, dm, sc, g1, b1, *o),
               row_out, drops)
    adds = [(None, None, 1.0), (zeros, None, 1.0), (None, ones, 1.0), (zeros, ones, 1.0)]
    _, dp_k, mean_d, rstd_d, _, x0, _, m1, r1 = e_f
    same("embed_fuse_bwd", lambda o, a1, a2, dm, sc: ops.embed_fuse_bwd(dh1, x0, m1, r1, g1, a1, a2, dm, sc, mr, md, rgb, dp_k,
                                                                         mean_d, rstd_d, lg, lb, *o),
         [fr, fr, (N, 2, H), (N, 2, H)],
         [(None, None, None, 1.0), (zeros, None, None, 1.0), (None, zeros, None, 1.0), (zeros, zeros, None, 1.0),
          (None, None, ones, 1.0), (zeros, zeros, ones, 1.0)])
    _, dp_k, mean_d, rstd_d, _, x0, _, m1, r1 = p_f
    same("plain_fuse_bwd", lambda o, a1, dm, sc: ops.plain_fuse_bwd(dh1, x0, m1, r1, g1, a1, dm, sc, rgb, dp_k, mean_d, rstd_d,
                                                                     lg, lb, *o),
         [fr, fr, (N, 2, H), (N, 2, H), fr], adds)
    x0, _, m1, r1 = v_f
    same("scaled_exchange_bwd", lambda o, a1, dm, sc: ops.scaled_exchange_bwd(dh1, x0, m1, r1, g1, a1, dm, sc, rgb, dep, mr, md,
                                                                               al, *o),
         [fr, fr, fr, (N, 2, H)], adds)
    x0, _, m1, r1 = b_f
    same("bn_blend_bwd", lambda o, a1, dm, sc: ops.bn_blend_bwd(dh1, x0, m1, r1, g1, a1, dm, sc, rgb, dep, mean, rstd, *bn, al,
                                                                 mr, md, *o),
         [fr] * 5 + [(N, 2, H)], adds)
