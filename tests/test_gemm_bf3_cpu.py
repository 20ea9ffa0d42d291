"""Sanity of tests/gemm_bf3_cases.py: every edge tests/test_gemm_bf3_gpu.py claims to pin is present in the table (computed
from it with the mirrors of the kernels' index arithmetic), every row is one gemm_validate / gemm_bf3_*_ok admits, every
bound meets the condition that keeps it from hiding what its row is for, the exactness inputs are exact under a numpy
emulation of the split and of the six-term accumulation, the planner mirror agrees with r3d_gemm_plan, and the planner's
prec == 1 rules hold on both sides of each boundary.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_bf3_cases as G

ALL_CASES = G.NT_CASES + G.TN_CASES + G.ADAM_CASES + G.PAIR_CASES + G.EXACT_CASES


def test_case_ids_are_unique():
    ids = [G.case_id(c) for c in ALL_CASES]
    assert len(ids) == len(set(ids))
    assert all(w[0] in ids for w in G.WIDENED), "a WIDENED entry names no case"


# ----------------------------------------------------------------------------------------------------------
# the edges
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", G.NT_TILES)
def test_nt_edges_are_present(tile):
    rows = [c for c in G.NT_CASES if c.tile == tile]
    slabs = {c: G.nt_slab_steps(tile, c.K, G.nt_split(tile, c.K, c.splitk)[1]) for c in rows}
    steps = {s[1] for v in slabs.values() for s in v}
    assert {1, 2, 4} <= steps and any(s > 1 and s % 2 for s in steps), steps
    # a last slab of a single octet (which is also its only k-step), one exactly full, the smallest K the kernel admits
    assert any(v[-1][0] == 8 for v in slabs.values())
    assert any(v[-1][0] == v[0][0] for v in slabs.values())
    assert any(v[-1][0] != v[0][0] and v[-1][2] == 1 and v[-1][1] > 1 for v in slabs.values()), "no one-octet last k-step"
    kmin = min(c.K for c in rows)
    assert kmin == (72 if tile == 8 else 64)
    assert not G.nt_ok(tile, 1, 1, kmin - 8, kmin - 8, kmin - 8, *G.nt_split(tile, kmin - 8, 2)), "a smaller K is admitted"
    assert any(len(v) > 2 for v in slabs.values()), "never more than two slabs"
    assert {c.M for c in rows} >= {1, 63, 64, 65, 130} and {c.N for c in rows} >= {1, 40, 64, 65, 129, 257}
    bm = G.BM[tile]
    assert any(c.M % bm == 0 and c.N % bm == 0 for c in rows), "no whole tile"
    assert any(c.M % bm and c.N % bm and G.cdiv(c.M, bm) > 1 and G.cdiv(c.N, bm) > 1 for c in rows), "no ragged 2-D tile grid"
    assert any(G.cdiv(c.M, bm) > 1 for c in rows) and any(G.cdiv(c.N, bm) > 1 for c in rows)
    assert {c.pad for c in rows} == {0, 4} and {c.off for c in rows} >= {0, 12}
    assert all(c.off % 4 == 0 for c in rows)
    assert any(c.pad == 4 and c.off for c in rows)
    assert sum(c.dist == "wide" for c in rows) == 1
    # workgroups past the last slab exist in every row (the `split >= NG` return), as the grid is padded to groups of 8
    assert all(G.nt_grid(tile, c.M, c.N, len(slabs[c]))[2] > 0 for c in rows)


@pytest.mark.parametrize("tile", G.TN_TILES)
def test_tn_edges_are_present(tile):
    rows = [c for c in G.TN_CASES if c.tile == tile]
    assert {c.K for c in rows} == {16, 24, 32, 40, 64, 96, 100}
    assert {c.M for c in rows} == {4, 64, 128, 132} and {c.N for c in rows} == {4, 128, 132, 1028}
    steps = {G.tn_steps(c.K) for c in rows}
    assert (1, 32) in steps and (1, 16) in steps and (2, 8) in steps and (4, 4) in steps
    assert any(nk > 1 and nk % 2 and last == 32 for nk, last in steps) and any(nk % 2 == 0 and last == 32 for nk, last in steps)
    assert {c.pad for c in rows} == {0, 4}
    nine = [c for c in rows if G.tn_grid(c.M, c.N)[1] == 9]
    assert nine and all(G.tn_grid(c.M, c.N)[3] == 7 * G.cdiv(c.M, 128) for c in nine), "the `tn >= NG` return is not reached"
    assert any(G.tn_grid(c.M, c.N)[0] == 2 and G.tn_grid(c.M, c.N)[1] == 2 for c in rows)
    assert any(c.M == 128 and c.N == 128 and c.K % 32 == 0 for c in rows), "the unchecked producer path never runs"
    assert sum(c.dist == "wide" for c in rows) == 1
    adam = [c for c in G.ADAM_CASES if c.tile == tile]
    assert {(c.K, c.M, c.N) for c in adam} == {(40, 132, 132), (64, 128, 256), (16, 4, 1028)}


def test_pair_edges_are_present():
    assert {(c.M, c.N) for c in G.PAIR_CASES} == {(8, 40), (70, 100), (130, 132)}
    assert {c.K2 for c in G.PAIR_CASES} == {72, 136, 1792} and all(c.K1 == 8200 and c.pad2 % 4 == 0 and c.pad2 for c in G.PAIR_CASES)
    for c in G.PAIR_CASES:
        tile, ns1, kps1 = G.plan_nt(c.M, c.N, c.K1)
        assert tile == 8 and ns1 % 8, "no spare slot"
        ns2, kps2 = G.pair_split(c.K2, ns1, kps1)
        assert ns2 >= 2 and ns2 <= -ns1 % 8 and kps2 <= kps1 and kps2 % 64 == 0
        # the second product's slabs sit behind the first's in its last group: nothing of it reaches a further group
        assert G.nt_grid(8, c.M, c.N, ns1, ns2)[1] == G.nt_grid(8, c.M, c.N, ns1)[1]
        assert G.nt_ok(8, c.M, c.N, c.K2, c.K2 + c.pad2, c.K2 + c.pad2, ns2, kps2)
    (M, N, K1, K2, kps2, _), (M_, N_, K1_, K2_, kps2_, _) = G.PAIR_DIRECT
    ns1, ns2 = G.plan_nt(M, N, K1)[1], G.cdiv(K2, kps2)
    assert ns2 > -ns1 % 8 and G.nt_grid(8, M, N, ns1, ns2)[1] > G.nt_grid(8, M, N, ns1)[1]
    assert G.plan_nt(M_, N_, K1_)[0] == 8 and G.plan_nt(M_, N_, K1_)[1] % 8 == 0
    for K1, K2, why in G.PAIR_NONE:
        assert G.plan_nt(8, 40, K1)[0] == 8 and G.pair_split(K2, *G.plan_nt(8, 40, K1)[1:]) == why
    assert {K2 % 8 != 0 for _, K2, why in G.PAIR_NONE if why == "k2"} == {True, False}
    assert {why for _, _, why in G.PAIR_NONE} == {"no spare slot", "kps2 > kps1", "k2"}


def test_exact_edges_are_present():
    for t in (7, 8, 9, 10, 11, 12):
        have = {(c.kind, c.side) for c in G.EXACT_CASES if c.tile == t}
        assert have == {(k, s) for k in ("select", "short", "single") for s in ("A", "B")}
    for c in G.EXACT_CASES:
        if c.tile in G.NT_TILES:
            assert 128 <= c.K <= 264 and c.N == c.K
        else:
            assert c.K == c.M == 128 and (c.tile != 7 or c.N == 2048)


# ----------------------------------------------------------------------------------------------------------
# admission
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.NT_CASES + G.TN_CASES + G.ADAM_CASES + G.EXACT_CASES, ids=G.case_id)
def test_row_is_admitted(c):
    kind = type(c).__name__
    if kind == "NtCase" or (kind == "ExactCase" and c.tile in G.NT_TILES):
        pad = c.pad if kind == "NtCase" else 0
        assert G.nt_ok(c.tile, c.M, c.N, c.K, c.K + pad, c.K + pad, *G.nt_split(c.tile, c.K, c.splitk))
    elif kind == "ExactCase" and c.tile == 7:
        assert G.panel_ok(c.M, c.N, c.K, c.N, c.N)
    else:
        pad = c.pad if kind == "TnCase" else 0
        assert G.tn_ok(c.M, c.N, c.K, c.M + pad, c.N + pad)
        if kind == "AdamCase":
            assert (c.N + G.TN_LDC_PAD) % 4 == 0 and G.ADAM["alpha"] != 0


# ----------------------------------------------------------------------------------------------------------
# the bounds
# ----------------------------------------------------------------------------------------------------------
def _bound_condition(p, K, dist, tail, what):
    assert p.bound == G.MARGIN * p.e32 + G.SLACK
    if tail:
        assert dist == "pos", f"{what}: a K-tail case needs positive operands"
        prod_min = float(p.A.min()) * float(p.B.min())
        assert p.A.min() >= 0.5 and p.B.min() >= 0.5 and p.A.max() < 1 and p.B.max() < 1
        assert 8 * prod_min / float(p.S.max()) >= 2.0 / K, f"{what}: an octet weighs less than 2 / K"
        assert p.bound < 1.0 / K, (what, p.bound, p.e32)
    else:
        assert dist in ("randn", "wide"), what
        assert bool((p.A < 0).any()) and bool((p.A > 0).any()) and bool((p.B < 0).any()) and bool((p.B > 0).any())
        assert p.bound <= 2.0 ** -16, (what, p.bound, p.e32)
    if dist == "wide":
        lo, hi = float(p.A.abs().min()), float(p.A.abs().max())
        assert hi / max(lo, 1e-300) > 2.0 ** 36, f"{what}: the exponents are not spread"


@pytest.mark.parametrize("c", G.NT_CASES + G.TN_CASES, ids=G.case_id)
def test_bound_cannot_hide_what_the_row_is_for(c):
    _bound_condition(G.case_problem(c), c.K, c.dist, G.is_tail(c), G.case_id(c))


@pytest.mark.parametrize("c", G.PAIR_CASES, ids=G.case_id)
def test_pair_bounds(c):
    p1, p2, d2 = G.pair_problems(c)
    tile, ns1, kps1 = G.plan_nt(c.M, c.N, c.K1)
    ns2, kps2 = G.pair_split(c.K2, ns1, kps1)
    _bound_condition(p1, c.K1, "pos", c.K1 != ns1 * kps1, G.case_id(c) + " first")
    _bound_condition(p2, c.K2, d2, c.K2 != ns2 * kps2, G.case_id(c) + " second")
    assert c.K1 != ns1 * kps1


@pytest.mark.parametrize("row", G.PAIR_DIRECT, ids=lambda r: f"{r[2]}+{r[3]}")
def test_pair_direct_bounds(row):
    M, N, K1, K2, kps2, _ = row
    _, ns1, kps1 = G.plan_nt(M, N, K1)
    for p, K, dist, tail in G.pair_direct_problems(row):
        _bound_condition(p, K, dist, tail, f"pair-direct-{K1}+{K2}")
    assert G.nt_ok(8, M, N, K2, K2 + 4, K2 + 8, G.cdiv(K2, kps2), kps2) and kps2 <= kps1


def test_slack_is_the_derived_one():
    """|m| < 2^-7 |x| and |l| < 2^-15 |x| under the truncation split: the three dropped products"""
    from fractions import Fraction as Fr
    m, l = Fr(1, 2 ** 7) - Fr(1, 2 ** 23), Fr(1, 2 ** 15) - Fr(1, 2 ** 23)
    assert 2 * m * l + l * l == Fr(1, 2 ** 21) - Fr(1, 2 ** 30) - Fr(1, 2 ** 36) + Fr(3, 2 ** 46) < Fr(1, 2 ** 21)
    assert G.SLACK == 2.0 ** -21
    x = G.exact_values("select", 64, 64, 1)
    h, m, l = (np.abs(v.astype(np.float64)) for v in G.split3(x))
    ax = np.abs(x.astype(np.float64))
    assert (m < 2.0 ** -7 * ax).all() and (l < 2.0 ** -15 * ax).all() and (h <= ax).all()


# ----------------------------------------------------------------------------------------------------------
# exactness inputs
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.EXACT_CASES, ids=G.case_id)
def test_exact_input_is_exact(c):
    A, B, want = G.exact_operands(c)
    if c.tile not in G.NT_TILES:
        A, B = A.T, B.T                                              # [M, K], [N, K]
    for x in (A, B):
        h, m, l = G.split3(x)
        assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
        assert not (l.view(np.uint32) & 0xFFFF).any(), "the last term is not a bf16 value"
        assert np.isfinite(x).all()
    dense, sel = (A, B) if c.side == "A" else (B, A)
    assert ((sel != 0).sum(1) == 1).all() and (dense != 0).all()
    h, m, l = G.split3(dense)
    if c.kind == "select":
        assert (h != 0).all() and (m != 0).any() and (l != 0).any() and set(np.unique(sel)) == {0.0, 1.0}
        mant = dense.view(np.uint32) & 0x7FFFFF
        assert (mant == 0x7FFFFF).any() and (mant == 0).any() and ((mant & 0xFFFF) == 0).any()
        e = ((dense.view(np.uint32) >> 23) & 0xFF).astype(int) - 127
        assert e.min() == -40 and e.max() == 40
    elif c.kind == "short":
        assert (h != 0).all() and (m != 0).all() and not l.any()
        hs, ms, ls = G.split3(sel[sel != 0])
        assert (hs != 0).all() and (ms != 0).all() and not ls.any()
    else:
        assert not m.any() and not l.any() and not G.split3(sel)[1].any()
    # every output element: its one nonzero pair through the six-term fp32 accumulation
    k_of = (sel != 0).argmax(1)                                      # [other]
    a = dense[:, k_of]                                               # [dense rows, other]
    b = sel[np.arange(sel.shape[0]), k_of][None, :]
    got, small = G.six_terms(a, b)
    exact = a.astype(np.float64) * b.astype(np.float64)
    assert np.array_equal(got.astype(np.float64), exact), "the six-term sum rounds"
    assert small >= 2.0 ** -126, f"a subnormal intermediate ({small:g})"
    w = exact if c.side == "A" else exact.T
    assert np.array_equal(w, want) and np.array_equal(want.astype(np.float32).astype(np.float64), want)


# ----------------------------------------------------------------------------------------------------------
# the planner
# ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from r3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _plan(lib, layout, M, N, K):
    from r3d_amd import _lib
    d = _lib.GemmDesc()
    d.layout, d.M, d.N, d.K, d.prec, d.alpha = layout, M, N, K, 1, 1.0
    d.lda, d.ldb, d.ldc = (K, K, N) if layout == G.NT else (M, N, N)
    d.A = d.B = d.C = 4096                           # (never dereferenced: the planner looks at the alignment only)
    assert lib.r3d_gemm_plan(C.byref(d)) == 0
    return int(d.tile), int(d.splitk), int(d.k_per_split)


def test_plan_mirror_agrees_with_the_planner(lib):
    shapes = [(c.M, c.N, c.K1) for c in G.PAIR_CASES] + [(8, 40, K1) for K1, _, _ in G.PAIR_NONE]
    shapes += [(M, N, K1) for M, N, K1, _, _, _ in G.PAIR_DIRECT]
    shapes += [(128, 128, 50176), (512, 512, 50176), (100, 96, 8200), (256, 1024, 16384), (256, 256, 2048), (256, 257, 8192),
               (2048, 2048, 2048), (1536, 1536, 8192)]
    for M, N, K in shapes:
        want = G.plan_nt(M, N, K)
        assert want is not None and _plan(lib, G.NT, M, N, K) == want, (M, N, K)
    for M, N, K in [(8, 40, 8184), (256, 255, 2048), (8, 40, 8196), (512, 512, 2040)]:
        assert G.plan_nt(M, N, K) is None and _plan(lib, G.NT, M, N, K)[0] <= 5, (M, N, K)
    # the planner's `ns >= 2` guard cannot fail for an admitted K (a slab is at most 64 * cdiv(cdiv(K, 2), 64) < K from
    # K = 2048 on), so the split count never falls below 2: where 256 / tiles does (129 tiles and more), it is raised to 2
    for M, N in ((1536, 1536), (2048, 2048)):
        assert 256 // min(G.cdiv(M, 128) * G.cdiv(N, 128), 256) < 2 and G.plan_nt(M, N, 8192)[:2] == (9, 2)


def _t(rows, cols, ld=None, off=0):
    """an uninitialised host tensor [rows, cols] of leading dimension ld, `off` floats into its allocation"""
    ld = cols if ld is None else ld
    return torch.empty(off + rows * ld, dtype=torch.float32)[off:].view(rows, ld)[:, :cols]


def test_planner_nt_boundaries(lib):
    from r3d_amd import ops

    def tile(M, N, K, a=None, c=None, **kw):
        a = _t(M, K) if a is None else a
        return ops.gemm_planned_tile(G.NT, a, _t(N, K), _t(M, N), prec=1, **kw)
    assert tile(8, 40, 8192) == 8 and tile(8, 40, 8184) <= 5
    assert tile(256, 256, 2048) == 8 and tile(256, 255, 2048) <= 5 and tile(256, 256, 2040) <= 5
    assert tile(256, 256, 8192) == 8 and tile(256, 257, 8192) == 9          # sixteen and twenty 64 x 64 tiles
    assert tile(192, 320, 8192) == 8 and tile(256, 320, 8192) == 9          # fifteen and twenty
    assert tile(64, 1024, 8192) == 8 and tile(64, 1088, 8192) == 9          # the rule's own edge: sixteen and seventeen
    assert tile(1408, 1408, 8192) == 9                                       # 121 tiles of 128: 256 / tiles = 2
    assert tile(2048, 2048, 8192) == 9                                       # 256 tiles: a split count of 1, raised to 2
    # back to an fp32 tile
    assert tile(8, 40, 8196) <= 5                                            # K % 8
    assert tile(8, 40, 8192, a=_t(8, 8192, ld=8194)) <= 5                    # lda % 4
    assert tile(8, 40, 8192, a=_t(8, 8192, ld=8196)) == 8                    # (a padded lda alone is fine)
    assert tile(8, 40, 8192, a=_t(8, 8192, off=1)) <= 5                      # A off a 16-byte boundary
    assert tile(8, 40, 8192, a=_t(8, 8192, off=4)) == 8
    assert tile(8, 40, 8192, alpha=0.5) <= 5
    assert tile(8, 40, 8192, a_add=_t(8, 8192), a_add_mod=8) <= 5
    assert ops.gemm_planned_tile(G.NT, _t(8, 8192), _t(40, 8192), _t(8, 40), prec=0) <= 5


def test_planner_tn_boundaries(lib):
    from r3d_amd import ops

    def tile(K, M, N, c=None, **kw):
        return ops.gemm_planned_tile(G.TN, _t(K, M), _t(K, N), _t(M, N) if c is None else c, prec=1, **kw)
    assert tile(256, 128, 2048) == 12 and tile(256, 128, 2044) <= 5
    assert tile(64, 512, 2048) == 12 and tile(60, 512, 2048) <= 5
    assert tile(64, 256, 2048) == 12 and tile(65, 252, 2048) <= 5            # M * K = 16384 / 16380
    assert tile(125, 132, 2048) == 12 and tile(124, 132, 2048) <= 5          # M * K = 16500 / 16368, K and M % 4 unchanged
    assert tile(127, 129, 2048) <= 5                                         # M * K = 16383 (and M % 4 != 0)
    assert tile(64, 260, 2048) == 12 and tile(64, 258, 2048) <= 5            # M % 4
    # the panel kernel: tile 7 needs float4 rows of C, tile 6 does not
    assert tile(128, 128, 2048) == 7
    assert tile(128, 128, 2048, c=_t(128, 2048, ld=2050)) == 6 and tile(128, 128, 2048, c=_t(128, 2048, ld=2052)) == 7
    assert tile(128, 128, 2048, c=_t(128, 2048, off=1)) == 6 and tile(128, 128, 2048, c=_t(128, 2048, off=4)) == 7
    assert ops.gemm_planned_tile(G.TN, _t(128, 128), _t(128, 2048), _t(128, 2048), prec=0) == 6
    # ... and just past its 128 x 128 limit
    assert tile(129, 128, 2048) == 12 and tile(128, 132, 2048) == 12
    assert tile(128, 129, 2048) <= 5                                         # M % 4: neither bf16x3 kernel takes it
    assert tile(129, 64, 2048) <= 5                                          # M * K = 8256: too few rows for tile 12
