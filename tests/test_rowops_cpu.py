"""tests/rowops_cases.py without a GPU: that the tables are the ones stated and cover every option on and off at every
site and every pair of options somewhere; that the ReLU kink condition masks under 1% of a case; that every fixed bound
leaves float32 itself a factor 8 (8 e32 <= bound per case and tensor; prints e32); that the closed-form backward the
kernel implements is autograd through the forward restatement; that the three statements of the backward's block count
agree; and that the C entry points refuse what they must before any launch."""
import itertools

import pytest
import torch

from tests import rowops_cases as RC
from tests import rowops_oracle as RO


@pytest.fixture(scope="module")
def lib():
    from r3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
def test_tables_are_the_stated_ones():
    assert RC.WIDTHS == [1, 2, 63, 64, 65, 128, 129, 136, 512, 513, 1024, 1025, 2048] and RC.WIDTH_ROWS == 5
    assert RC.ROWS == [1, 3, 4, 5, 1024, 1025, 2049, 4100] and RC.ROW_WIDTHS == [8, 72]
    assert RC.SPLITK_NSPLIT == [1, 5, 8, 9, 16, 17] and RC.SPLITK_H == [128, 264] and len(RC.SPLITK_VARIANTS) == 8
    assert RC.MULTI_ROWS == (8, 1030, 64, 2) and RC.MULTI_H == [128, 264] and len(RC.multi_cases()) == 8
    assert RC.FIN_PAIRS == [1, 2, 4, 12, 13, 15, 16, 17, 31, 32, 33, 1030]
    assert {H for _, H in RC.fin_jobs()} >= {8, 1032}
    assert RC.SUM_ROWS == [1, 64, 65, 129, 2048, 2049, 4100] and RC.COLSUM_COLS == [1, 63, 64, 65, 513]
    assert RC.ROWMOD_MODS == [1, 5, 4200] and RC.ROWMOD_COLS == [17, 257]
    assert (RC.MARGIN, RC.SUM_FLOOR, RC.KINK, RC.KINK_CAP, RC.FWD_TOL, RC.DX_TOL) == (8.0, 2e-6, 1e-5, 0.01, (1e-4, 1e-5), (1e-3, 1e-4))
    # the row counts reach what they are there for: one block, 256 blocks of 4 rows, rows_per_block 8, 12 and 20, ragged
    rpb = lambda r: max(4, ((r + 255) // 256 + 3) // 4 * 4)         # noqa: E731
    assert [rpb(r) for r in (1024, 1025, 2049, 4100)] == [4, 8, 12, 20] and RC.blocks_as_rowsum(1024) == 256
    assert all(r % rpb(r) for r in (1025, 2049)) and RC.blocks_as_rowsum(4) == 1 and RC.blocks_as_rowsum(5) == 2


def test_layernorm_cases_cover_every_option_and_every_pair():
    S = RC.sites()
    assert len(RC.LN_CASES) == 3 * (len(RC.WIDTHS) + len(RC.ROWS)) and len(set(RC.LN_IDS)) == len(RC.LN_IDS)
    flags = [(c[4], c[1], c[2], RC.flags_of(c[3])) for c in RC.LN_CASES]
    for i, (rows, H) in enumerate(S):
        mine = [f for s, r, h, f in flags if s == i]
        assert all(h == H and r in (rows, RC.even(rows)) for s, r, h, _ in flags if s == i)
        assert len(mine) == 3
        for n in RC.FLAGS:
            assert any(n in f for f in mine) and any(n not in f for f in mine), (rows, H, n)
        assert any(c[3]["dx2"] is None for c in RC.LN_CASES if c[4] == i) and {c[3]["layout"] for c in RC.LN_CASES if c[4] == i} == \
            {"dense", "aligned", "misaligned"}
    for n in RC.FLAGS:                             # (implied by the above; stated because the issue states it)
        assert any(n in f for _, r, h, f in flags if h > 128) and any(n in f for _, r, h, f in flags if r > 1024), n
    for a, b in itertools.combinations(RC.FLAGS, 2):
        if frozenset((a, b)) not in RC.EXCLUSIVE:
            assert any(a in f and b in f for *_, f in flags), (a, b)
    for _, r, _, o, _ in RC.LN_CASES:
        assert not o["pair_in"] or r % 2 == 0
    assert {c[3]["off"] for c in RC.LN_CASES if c[3]["layout"] == "misaligned"} == {"x", "dy", "dx"}


def test_rowsum_groups_cover_the_stated_mix():
    jobs = [j for g in RC.RS_GROUPS for j in g]
    assert [len(g) for g in RC.RS_GROUPS] == [1, 2, 3, 4, 5, 6]
    assert {j[2] for j in jobs} == set(RC.RS_MODS) == {1, 5, 8, 37} and {j[1] for j in jobs} == set(RC.RS_COLS) == {1, 17, 64, 136, 272, 513}
    assert {j[0] for j in jobs} == {1, 7, "16m", "16m+3", 4100}
    assert {j[4] for j in jobs} == set(RC.RS_HOWS)
    assert any(RC.rs_rows(j[0], j[2]) < j[2] for j in jobs)                              # mod > rows: empty residue classes
    assert all({bool(j[3]) for j in g} == {False, True} for g in RC.RS_GROUPS[1:])        # src2 present and absent in one group
    assert all(len({j[2] for j in g}) > 1 and len({j[1] for j in g}) > 1 for g in RC.RS_GROUPS[1:])
    for rows, cols, mod, src2, how in jobs:
        lay = RC.rs_layout(cols, how)
        assert all(ld > cols for ld, _ in lay.values())
        assert RC.rs_takes_vector_path(cols, src2, how) == (how == "vec"), (cols, how)
        if how != "vec" and how != "cols":           # each of the other ways alone: the columns would allow the vector path
            assert cols % 4 == 0 and (src2 or "2" not in how)
    # a misaligned src2 ALONE (src1, dst and every ld as the vector path wants them)
    assert any(how == "off_src2" and src2 for _, _, _, src2, how in jobs) and any(how == "odd_ld2" and src2 for _, _, _, src2, how in jobs)


def test_broadcast_cases_cover_the_stated_mix():
    B = RC.BCAST_CASES
    assert {(r, c) for r, c, *_ in B} == {(24, 40), (1030, 260)} and 1030 * 260 > RC.BCAST_GRID_ELEMENTS > 24 * 40
    for size in ((24, 40), (1030, 260)):
        mine = [b for b in B if b[:2] == size]
        assert any(m == r for r, _, m, *_ in mine) and any(m == 8 for _, _, m, *_ in mine)
        assert any(not b[3] for b in mine) and any(b[4] for b in mine) and any(b[5] for b in mine) and any(not b[5] for b in mine)
    assert not any(b[4] and not b[3] for b in B)


# ---------------------------------------------------------------------------------------------------------------------
# the kink cap and 8 e32 <= bound
# ---------------------------------------------------------------------------------------------------------------------
def _condition(tag, p, names):
    bad = []
    for n in names:
        f64, f32 = p["ref"][n], p["ref32"][n]
        assert f64.dtype == torch.float64 and f32.dtype == torch.float32 and bool(torch.isfinite(f64).all()), (tag, n)
        err = (f32.double() - f64).abs()
        e32 = float(err.max())
        if n in RC.LN_SUM_TENSORS:
            bound, _ = RC.sum_bound(f32, f64)
            ratio = RC.MARGIN * e32 / bound if bound else 0.0
        else:
            tol = RC.ln_tol(n)
            ratio = RC.elem_ok(err, f64, tol, RC.MARGIN)
            bound = tol[1] + tol[0] * float(f64.abs().max())
        print(f"[rowops] {tag} {n}: e32 {e32:.2e} bound {bound:.2e} ratio {ratio:.3f}")
        if not ratio <= 1.0:
            bad.append((n, e32, bound))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("cid", RC.LN_IDS)
def test_layernorm_case_meets_the_condition_and_the_kink_cap(cid):
    p = RC.ln_problem(cid)
    _condition(f"ln {cid}", p, list(p["ref"]))
    print(f"[rowops] ln {cid}: kink share {p['kink_share']:.2e}")
    assert p["kink_share"] < RC.KINK_CAP and (p["o"]["relu"] or p["kink_share"] == 0.0)
    if p["o"]["relu"]:                              # the condition did its work: no gradient arrives at a unit near the kink
        v = RO.ln_fwd(p["t"]["x"], p["t"]["gamma"], p["t"]["beta"], torch.float64)["v"]
        k = v.abs() <= RC.KINK * float(v.abs().max())
        d = p["t"]["dy"] if p["t"]["dy2"] is None else p["t"]["dy"].abs() + p["t"]["dy2"].abs()
        if p["o"]["pair_in"]:
            d = d.repeat_interleave(2, dim=0)
        assert not bool(d[k].any())


@pytest.mark.parametrize("j,H", [(j, H) for H in RC.MULTI_H for j in range(4)])
def test_multi_job_meets_the_condition_and_the_kink_cap(j, H):
    p = RC.multi_job(j, H)
    _condition(f"multi job{j} H{H}", p, list(p["ref"]))
    assert p["kink_share"] < RC.KINK_CAP
    assert [bool(RC.multi_job(k, H)["o"]["pair_in"]) for k in range(4)].count(True) == 1
    assert [bool(RC.multi_job(k, H)["o"]["relu"]) for k in range(4)].count(True) == 1


@pytest.mark.parametrize("nsplit", RC.SPLITK_NSPLIT)
@pytest.mark.parametrize("H", RC.SPLITK_H)
def test_splitk_case_meets_the_condition(nsplit, H):
    for i, (bias, pre, pair) in enumerate(RC.SPLITK_VARIANTS):
        p = RC.splitk_problem(nsplit, H, bias, bool(i & 1) != pair, pair)
        _condition(f"splitk ns{nsplit} H{H} bias{int(bias)} pair{int(pair)}", p, list(p["ref"]))


def test_sums_report_e32():
    """the sum bounds hold 8 e32 by construction; what is asserted is that the float32 restatement is a float32 sum (its
    error is not 0 at 4100 rows, and stays under 1e-5 of scale) -- and the figures are printed"""
    for tag, probs in (("colsum", [RC.colsum_problem(r, c) for r in RC.SUM_ROWS for c in RC.COLSUM_COLS]),
                       ("rowmod_sum", [RC.rowmod_problem(r, c, m) for r in RC.SUM_ROWS for c in RC.ROWMOD_COLS for m in RC.ROWMOD_MODS]),
                       ("rowsum_group", [RC.rs_problem(g, k) for g in range(len(RC.RS_GROUPS)) for k in range(len(RC.RS_GROUPS[g]))]),
                       ("finalize", [dict(ref=torch.stack(list(p["ref"].values())), ref32=torch.stack(list(p["ref32"].values())))
                                     for p in (RC.fin_problem(n, H) for n, H in RC.fin_jobs())])):
        es = []
        for p in probs:
            bound, e32 = RC.sum_bound(p["ref32"], p["ref"])
            assert p["ref32"].dtype == torch.float32 and RC.MARGIN * e32 <= bound
            assert e32 <= 1e-5 * max(float(p["ref"].abs().max()), 1.0)
            es.append(e32)
        print(f"[rowops] {tag}: e32 {min(es):.2e} .. {max(es):.2e} over {len(es)} cases")
        assert max(es) > 0.0


def test_empty_residue_classes_are_exact_zeros():
    p = RC.rowmod_problem(65, 17, 4200)
    assert float(p["ref"][65:].abs().max()) == 0.0 and bool((p["ref"][:65] == p["x"].double()).all())
    assert torch.equal(p["ref_acc"][65:], p["out0"].double()[65:])


@pytest.mark.parametrize("cid", RC.LN_IDS[::5] + [c[0] for c in RC.LN_CASES if c[3]["pair_in"] and c[3]["relu"]][:3])
def test_closed_form_backward_is_autograd_through_the_forward(cid):
    p = RC.ln_problem(cid)
    t = p["t"]
    a = RO.ln_bwd_closed(t["dy"], t["x"], t["gamma"], t["beta"], torch.float64, **p["kw"])
    for n in ("dx", "dx2", "dgamma", "dbeta"):
        want = p["ref"][n] if n in p["ref"] else p["ref"]["dx"]
        scale = max(float(want.abs().max()), 1.0)
        assert float((a[n] - want).abs().max()) <= 1e-12 * scale, (cid, n)


def test_forward_restatement_is_torch_layer_norm():
    import torch.nn.functional as F
    p = RC.ln_problem(RC.LN_IDS[20])
    t = p["t"]
    f = RO.ln_fwd(t["x"], t["gamma"], t["beta"], torch.float64)
    want = F.layer_norm(t["x"].double(), (p["H"],), t["gamma"].double(), t["beta"].double(), RO.EPS)
    assert float((f["y"] - want).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the block-count rule, stated three times
# ---------------------------------------------------------------------------------------------------------------------
def test_backward_block_count_has_one_value(lib):
    from r3d_amd import ops
    for H in (8, 2048):
        for rows in range(1, 6001):
            blocks = RC.blocks_as_rowsum(rows)
            got = ops.layernorm_bwd_ws_floats(rows, H)
            assert got == (blocks * 2 * H if blocks > 1 else 0), (rows, H)
            assert RC.blocks_finalize_kernel(rows) == blocks, rows
    assert RC.blocks_finalize_kernel(-13) == 13


def test_colsum_chunk_count(lib):
    for cols in (1, 513):
        for rows in range(1, 6001):
            ch = min(32, -(-rows // 64))
            assert lib.r3d_colsum_ws_floats(rows, cols) == (ch * cols if ch > 1 else 0), (rows, cols)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: R3D_EINVAL before any launch (the arguments are checked on the host; no pointer is followed)
# ---------------------------------------------------------------------------------------------------------------------
P = 0x1000                       # stands for a device address; every call below must return before using it


def _fwd(lib, *, ldx=16, ldy=16, rows=4, H=16, nsplit=0, pair=None):
    return lib.r3d_layernorm_fwd(P, ldx, nsplit, None, None, P, P, P, ldy, P, P, pair, rows, H, 0, None)


def _bwd(lib, *, lddy=16, ldx=16, lddx=16, dy2=None, lddy2=0, rows=4, H=16, pair_in=0, dgamma=P, dbeta=P):
    return lib.r3d_layernorm_bwd(P, lddy, pair_in, dy2, lddy2, P, ldx, P, P, P, P, 0, None, 0, None, 0, P, lddx, None, 0, None, 0,
                                 1.0, dgamma, dbeta, P, rows, H, 0, None)


def test_entry_points_refuse_before_launching(lib):
    from r3d_amd import _lib
    E = _lib.EINVAL
    assert E != 0
    for H in (0, 2049):
        assert _fwd(lib, H=H, ldx=4096, ldy=4096) == E and _bwd(lib, H=H, lddy=4096, ldx=4096, lddx=4096) == E
        assert lib.r3d_layernorm_bwd_finalize(P, 8, H, P, P, None) == E
        assert lib.r3d_layernorm_bwd_finalize_batched(P, 1, H, None) == E
    assert _fwd(lib, ldx=15) == E and _fwd(lib, ldy=15) == E                                   # ld < H
    assert _bwd(lib, lddy=15) == E and _bwd(lib, ldx=15) == E and _bwd(lib, lddx=15) == E and _bwd(lib, dy2=P, lddy2=15) == E
    assert _fwd(lib, rows=5, pair=P) == E and _bwd(lib, rows=5, pair_in=1) == E               # odd rows with pairing
    assert _bwd(lib, dgamma=None) == E and _bwd(lib, dbeta=None) == E                         # only one of dgamma / dbeta
    assert _fwd(lib, rows=0) == E and _bwd(lib, rows=0) == E
    # multi-job launches: the job structs are host memory
    def fwd_jobs(widths):
        arr = (_lib.LnFwdJob * max(len(widths), 1))()
        for a, H in zip(arr, widths):
            a.x, a.ldx, a.gamma, a.beta, a.y, a.ldy, a.mean, a.rstd, a.rows, a.H = P, H, P, P, P, H, P, P, 4, H
        return arr

    def bwd_jobs(widths):
        arr = (_lib.LnBwdJob * max(len(widths), 1))()
        for a, H in zip(arr, widths):
            a.dy, a.lddy, a.x, a.ldx, a.mean, a.rstd, a.gamma, a.beta, a.dx, a.lddx = P, H, P, H, P, P, P, P, P, H
            a.dgamma, a.dbeta, a.ws, a.rows, a.H = P, P, P, 4, H
        return arr
    for n in (0, 5):
        assert lib.r3d_layernorm_fwd_multi(fwd_jobs([16] * n), n, None) == E
        assert lib.r3d_layernorm_bwd_multi(bwd_jobs([16] * n), n, None) == E
    assert lib.r3d_layernorm_fwd_multi(fwd_jobs([16, 32]), 2, None) == E                      # widths that differ
    assert lib.r3d_layernorm_bwd_multi(bwd_jobs([16, 32]), 2, None) == E
    assert lib.r3d_layernorm_fwd_multi(fwd_jobs([16, 16, 8]), 3, None) == E
    # mod = 0, ld < cols
    assert lib.r3d_rowmod_sum(P, 8, 4, 8, 0, P, 8, 0, None) == E and lib.r3d_rowmod_sum(P, 7, 4, 8, 2, P, 8, 0, None) == E
    assert lib.r3d_rowmod_sum(P, 8, 4, 8, 2, P, 7, 0, None) == E
    assert lib.r3d_add_rowbcast(P, 8, P, 8, 0, P, 8, 4, 8, None) == E and lib.r3d_add_rowbcast(P, 7, P, 8, 2, P, 8, 4, 8, None) == E
    assert lib.r3d_add_rowbcast(None, 0, P, 7, 2, P, 8, 4, 8, None) == E and lib.r3d_add_rowbcast(None, 0, P, 8, 2, P, 7, 4, 8, None) == E
    assert lib.r3d_rowmod_sum_batched(P, 1, 8, 0, None) == E and lib.r3d_rowmod_sum_batched(P, 0, 8, 1, None) == E
    assert lib.r3d_colsum(P, 7, 4, 8, P, None, 0, None) == E and lib.r3d_colsum(P, 8, 0, 8, P, None, 0, None) == E
    assert lib.r3d_colsum(P, 8, 65, 8, P, None, 0, None) == E                                  # two chunks and no workspace
