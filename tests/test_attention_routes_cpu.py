"""r3d_amd/attention.py without a GPU: the rule and the kept wrappers (engine.cross_attention_route / max_clip_len,
engine_unsup.query_attention_route / max_query_clip_len) against tests/golden/attention_routes_parent.json, recorded at the
commit before the module; the one ops.mha_* call a site's forward / backward makes on each route, argument by argument, as
FusionEngine._cross_fwd / _cross_bwd and decoder_composed's attend / attend_bwd made it at that commit; the keys and shapes
of what a site keeps."""
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_routes_parent.json")
MAX_POS = 2000
QUERY_ALLOWED = ("core", "tiled")


@pytest.fixture(scope="module")
def A():
    from r3d_amd import attention, build
    build.build(verbose=False)
    return attention


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


# ---- the rule ----------------------------------------------------------------------------------------------------------
def test_cross_routes_are_the_parents(A, golden):
    from r3d_amd import engine as E
    assert A.ROUTES == E.CROSS_ROUTES == ("core", "splitk", "tiled")
    assert len(golden["cross"]) == 768
    for Q, S, dh, train, long, want in golden["cross"]:
        assert E.cross_attention_route(Q, S, dh, train, long) == want, (Q, S, dh, train, long)
        assert A.pick(Q, S, dh, train, A.ROUTES if long else ("core",)) == want, (Q, S, dh, train, long)
        for r in A.ROUTES:              # a forced route runs exactly where the rule, allowed that route alone, picks it
            assert E.cross_route_supported(r, Q, S, dh, train) == (A.pick(Q, S, dh, train, (r,)) == r)


def test_query_routes_are_the_parents(A, golden):
    from r3d_amd import engine_unsup as U
    assert len(golden["query"]) == 160
    assert [9, 1024, 8, True, True, "tiled"] in golden["query"]         # Lq = 9 <= 16, yet never the split-key core
    for S, H, heads, train, long, want in golden["query"]:
        assert U.query_attention_route(S, H, heads, train, long) == want, (S, H, heads, train, long)
        assert A.pick(S, S, H // heads, train, QUERY_ALLOWED if long else ("core",)) == want, (S, H, heads, train, long)
        assert want != "splitk"


def test_longest_clips_are_the_parents(A, golden):
    from r3d_amd import engine as E, engine_unsup as U
    assert len(golden["max_clip"]) == 72 and len(golden["max_query"]) == 52
    for H, heads, Q, train, long, want in golden["max_clip"]:
        assert E.max_clip_len(H, heads, Q, MAX_POS, train, long) == want, (H, heads, train, long)
    for H, heads, train, long, want in golden["max_query"]:
        assert U.max_query_clip_len(H, heads, MAX_POS, train, long) == want, (H, heads, train, long)
    for n in (0, 1, 7, 100):
        assert A.longest(lambda s: s <= n, 100) == n
    assert A.longest(lambda s: True, 0) == 0


def test_an_allowed_route_is_taken_in_the_order_of_routes(A):
    assert A.pick(8, 2000, 16, True, ("tiled", "splitk")) == "splitk"          # (the caller's order does not count)
    assert A.pick(8, 2000, 16, True, ("tiled",)) == "tiled"
    assert A.pick(8, 2000, 16, True, ("core",)) is None and A.pick(8, 2000, 16, True, ()) is None
    assert A.pick(8, 16, 16, True, A.ROUTES) == "core"
    assert A.long_clips_hint(8, 2000, 16, True, A.ROUTES) == " (the split-key core runs this shape: --long_clips)"
    assert A.long_clips_hint(24, 2000, 16, True, A.ROUTES) == " (the tiled core runs this shape: --long_clips)"
    assert A.long_clips_hint(9, 9, 128, True, QUERY_ALLOWED) == " (the tiled core runs this shape: --long_clips)"
    assert A.long_clips_hint(8, 2000, 129, True, A.ROUTES) == ""


# ---- the launches ------------------------------------------------------------------------------------------------------
NAMES = [f"mha_{r}_{d}" for r in ("core", "splitk", "tiled") for d in ("fwd", "bwd")]
DIMS = (3, 8, 8, 300, 16)
C = {k: k for k in ("ca_o", "p_ca", "lse_ca", "ws_ca", "sa_o", "p_sa", "lse_sa")}
KEYS = dict(key_labels="labels", pad_idx=18)
DROP = dict(drop_mask="keep", drop_scale=1.25)

# (route, site, key mask given) -> (ops name, positional arguments, keyword arguments), as the parent's call sites made them
FWD = {
    ("core", "ca", True): ("mha_core_fwd", ("q", "k", "v", "p_ca", "ca_o") + DIMS, {**KEYS, **DROP}),
    ("splitk", "ca", True): ("mha_splitk_fwd", ("q", "k", "v", "ca_o", "lse_ca", "ws_ca") + DIMS, {**KEYS, **DROP}),
    ("tiled", "ca", True): ("mha_tiled_fwd", ("q", "k", "v", "ca_o", "lse_ca") + DIMS, {**KEYS, **DROP}),
    ("core", "sa", False): ("mha_core_fwd", ("q", "k", "v", "p_sa", "sa_o") + DIMS, DROP),
    ("tiled", "sa", False): ("mha_tiled_fwd", ("q", "k", "v", "sa_o", "lse_sa") + DIMS, DROP),
}
BWD = {
    ("core", "ca", True): ("mha_core_bwd", ("q", "k", "v", "p_ca", "d_o", "dq", "dk", "dv") + DIMS, DROP),
    ("splitk", "ca", True): ("mha_splitk_bwd", ("q", "k", "v", "ca_o", "lse_ca", "d_o", "delta", "dq", "dk", "dv", "ws_ca") + DIMS,
                             {**KEYS, **DROP}),
    ("tiled", "ca", True): ("mha_tiled_bwd", ("q", "k", "v", "ca_o", "lse_ca", "d_o", "delta", "dq", "dk", "dv") + DIMS,
                            {**KEYS, **DROP}),
    ("core", "sa", False): ("mha_core_bwd", ("q", "k", "v", "p_sa", "d_o", "dq", "dk", "dv") + DIMS, DROP),
    ("tiled", "sa", False): ("mha_tiled_bwd", ("q", "k", "v", "sa_o", "lse_sa", "d_o", "delta", "dq", "dk", "dv") + DIMS, DROP),
}


@pytest.fixture
def calls(monkeypatch):
    from r3d_amd import ops
    got = []
    for name in NAMES:
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: got.append((_n, a, kw)))
    return got


@pytest.mark.parametrize("route,site,masked", list(FWD), ids=lambda v: str(v))
def test_a_site_makes_the_parents_one_call_each_way(A, calls, route, site, masked):
    keys = KEYS if masked else {}
    A.forward(route, site, C, "q", "k", "v", DIMS, "keep", 1.25, **keys)
    assert calls == [FWD[route, site, masked]]
    del calls[:]
    A.backward(route, site, C, "q", "k", "v", "d_o", "dq", "dk", "dv", "delta", DIMS, "keep", 1.25, **keys)
    assert calls == [BWD[route, site, masked]]


# ---- the buffers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True])
def test_a_site_keeps_exactly_these_tensors(A, train):
    from r3d_amd import ops
    B, heads, Lq, Lk, dh = DIMS
    shape = lambda *s: s          # noqa: E731
    assert A.saved("core", "ca", shape, *DIMS, train) == {"p_ca": (B, heads, Lq, Lk)}
    assert A.saved("core", "sa", shape, B, heads, Lq, Lq, dh, train) == {"p_sa": (B, heads, Lq, Lq)}
    assert A.saved("tiled", "sa", shape, B, heads, Lq, Lq, dh, train) == {"lse_sa": (B, heads, Lq)}
    assert A.saved("tiled", "ca", shape, *DIMS, train) == {"lse_ca": (B, heads, Lq)}
    n = -(-Lk // ops.mha_splitk_chunk(Lk, dh))
    fwd, bwd = B * heads * n * Lq * (dh + 2), B * heads * n * Lq * dh         # (r3d_mha_splitk_ws_floats, include/r3d_hip.h)
    assert A.saved("splitk", "ca", shape, *DIMS, train) == {"lse_ca": (B, heads, Lq), "ws_ca": (max(fwd, bwd if train else 0),)}
    for route in A.ROUTES:
        want = (B, heads, Lq) if train and route != "core" else None
        assert A.delta_buffer(route, shape, B, heads, Lq, train) == want


def test_thirds_are_the_column_slices(A):
    H = 6
    t = torch.arange(4 * 3 * H, dtype=torch.float32).reshape(4, 3 * H)
    q, k, v = A.thirds(t)
    for got, want in ((q, t[:, :H]), (k, t[:, H:2 * H]), (v, t[:, 2 * H:])):
        assert got.data_ptr() == want.data_ptr() and got.shape == want.shape and got.stride() == want.stride()
