"""Host-side checks of tests/erank_cases.py (no GPU): every row's plan, route and admission against the plan query
(ops.erank_plan, r3d_erank_plan) and the admission predicates, and the rows against every instance the plan query can
return -- so that tests/test_erank_shapes_gpu.py, which runs the rows, launches every reachable Jacobi instance."""
import pytest

from tests import erank_cases as EC


@pytest.fixture(scope="module")
def ops():
    from r3d_amd import build, ops
    build.build(verbose=False)
    return ops


def _route_plan(ops, m):
    return ops.erank_plan(m.R, m.C, warm=m.route == "warm", blocked=m.route == "blocked")


@pytest.mark.parametrize("m", EC.MATRICES, ids=EC.matrix_id)
def test_matrix_row_plan(ops, m):
    p = _route_plan(ops, m)
    assert p is not None, f"{EC.matrix_id(m)}: the route does not take the matrix"
    assert EC.plan_key(p, m.route) == m.plan, (EC.plan_key(p, m.route), m.plan)
    if m.route == "lds":
        assert ops.erank_fits(m.R, m.C)
    if m.route == "warm":
        assert ops.erank_fits_warm(m.R, m.C)
    if m.route == "blocked":
        assert ops.erank_blocked_supported(m.R, m.C)
    if not isinstance(m.layout, str):
        assert m.route == "lds" and m.layout[0] == "batch" and m.layout[1] > 1 and m.layout[2] > 0
    if m.layout == "xt":
        assert m.route == "blocked"
    assert m.spectrum in ("sep", "clu") and m.why


@pytest.mark.parametrize("s", EC.STEPS, ids=EC.step_id)
def test_step_row_admission_route_and_plan(ops, s):
    from r3d_amd import engine as E
    N = s.B * s.S
    if s.refuse is not None:
        with pytest.raises(ValueError, match=s.refuse):
            E.check_erank_shape(s.B, s.S, s.H)
        return
    E.check_erank_shape(s.B, s.S, s.H)
    assert ops.erank_fits(N, s.H) == (s.route == "lds")
    assert s.flip == (s.route == "blocked" and N < s.H)
    assert (s.warm and ops.erank_fits_warm(N, s.H) and s.route == "lds") == s.used
    if s.route == "blocked":
        R, C = (s.H, N) if s.flip else (N, s.H)
        p = ops.erank_plan(R, C, blocked=True)
    else:
        p = ops.erank_plan(N, s.H, warm=s.used)
    assert EC.plan_key(p, s.route) == s.plan, (EC.plan_key(p, s.route), s.plan)
    assert E.fuser_chain_shape_ok(s.B, s.S, s.H, EC.K, EC.Q, s.heads) == s.chain
    assert s.check in ("model", "fused")
    if s.check == "model":                        # the CPU oracle's cost: N <= ~1000 and H <= 512, or N <= 32
        assert (N <= 1000 and s.H <= 512) or N <= 32, EC.step_id(s)


def _reachable(ops):
    """Every instance the plan query returns, over a grid of (R, C) holding every bound: all C up to 160 (both lane groups,
    odd and even, every power of two of the level order) and the wide ones, all R up to each route's limit."""
    import ctypes
    from r3d_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int32 * 9)()
    po = ctypes.cast(out, ctypes.c_void_p)
    seen = {}
    cols = sorted(set(range(1, 161)) | {255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048})
    for warm in (0, 1):
        for C in cols:
            R = 1
            while lib.r3d_erank_plan(R, C, warm, 0, po) == 0:
                seen.setdefault(EC.instance(dict(zip(ops.ERANK_PLAN_FIELDS, out))), (R, C))
                R += 1
    for R in range(1, 9700):
        for C in (1, 2, 3, 17, 33):
            if lib.r3d_erank_plan(R, C, 0, 1, po) == 0:
                seen.setdefault(EC.instance(dict(zip(ops.ERANK_PLAN_FIELDS, out))), (R, C))
    return seen


def test_every_reachable_instance_has_a_matrix_row(ops):
    seen = _reachable(ops)
    covered = {EC.instance(_route_plan(ops, m)) for m in EC.MATRICES}
    missing = {k: v for k, v in seen.items() if k not in covered}
    assert not missing, f"instances without a MATRICES row (first (R, C) reaching each): {missing}"
    assert covered <= set(seen)
    print(f"[erank instances] {len(seen)} reachable ({sum(k[0] == 'blocked' for k in seen)} blocked), all covered by "
          f"{len(EC.MATRICES)} rows")
    # the edges the issue names, beyond one row per instance
    rows = EC.MATRICES
    assert any(m.R < m.C and m.route == "lds" and m.C >= 1024 for m in rows)
    assert any(m.C % 2 == 1 and m.route == "lds" for m in rows) and any(m.R % 4 and m.route == "lds" for m in rows)
    assert any(m.layout == "xt" for m in rows) and any(m.layout == "ld" and m.route == "blocked" for m in rows)
    assert any(m.route == "blocked" and m.C < _route_plan(ops, m)["b"] for m in rows)
    assert any(m.route == "blocked" and _route_plan(ops, m)["nreal"] % 2 for m in rows)
    assert any(m.route == "blocked" and m.R == 9596 for m in rows)
    clu = {(_route_plan(ops, m)["b"] if m.route == "blocked" else "lds") for m in rows if m.spectrum == "clu"}
    assert {"lds", 16, 8, 4, 2} <= clu, clu


def test_byte_bounds_flip_exactly(ops):
    for C, last in EC.LDS_BOUNDS:
        assert ops.erank_fits(last, C) and not ops.erank_fits(last + 1, C)
        assert ops.erank_plan(last, C) is not None and ops.erank_plan(last + 1, C) is None
    prev = None
    for last, b in EC.BLOCK_BOUNDS:
        assert ops.erank_plan(last, 64, blocked=True)["b"] == b
        nxt = ops.erank_plan(last + 1, 64, blocked=True)
        if b > 2:
            assert nxt["b"] == b // 2
        else:
            assert nxt is None and not ops.erank_blocked_supported(last + 1, 64) and ops.erank_blocked_supported(last, 64)
        if prev is not None:
            assert ops.erank_plan(prev + 1, 64, blocked=True)["b"] == b
        prev = last
    from r3d_amd import engine as E
    E.check_erank_shape(1, 9596, 128)
    with pytest.raises(ValueError, match="rank penalty"):
        E.check_erank_shape(1, 9597, 128)
    E.check_erank_shape(79, 4, 128)                      # 316 x 128: the LDS kernel
    assert not ops.erank_fits(320, 128) and ops.erank_plan(320, 128, blocked=True)["b"] == 16


def test_plan_query_refuses_what_the_launchers_refuse(ops):
    assert ops.erank_plan(0, 8) is None and ops.erank_plan(8, 0, blocked=True) is None
    assert ops.erank_plan(300, 128, warm=True) is None and ops.erank_plan(300, 128) is not None
    assert not ops.erank_fits_warm(300, 128) and ops.erank_fits(300, 128)
    p = ops.erank_plan(128, 128)
    assert p["level"] == 1 and p["warm"] == 0 and p["blocked"] == 0 and p["b"] == 0
    assert ops.erank_plan(128, 128, warm=True)["level"] == 0          # the basis never rides the level order
