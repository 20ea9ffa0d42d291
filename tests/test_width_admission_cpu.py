"""Every row of tests/width_cases.py against the engine's host-side admission predicates, and the predicates' boundaries
(no GPU: the attention limit is the library's own host-only r3d_mha_core_supported)."""
import pytest

from r3d_amd import engine as E, ops
from tests import width_cases as WC

MAX_POS = 2000                  # the reference's max_pos_len


@pytest.fixture(scope="module", autouse=True)
def lib():
    from r3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def variant_kw(c):
    return dict(bn=c.variant == "bn", vary=c.variant == "vary", plain=c.variant == "plain")


def admit(c):
    """None if the row's training step is admitted, else the ValueError's message."""
    try:
        E.check_engine_shape(c.H, c.heads, WC.Q, **variant_kw(c))
        E.check_clip_shape(c.S, c.H, c.heads, WC.Q, MAX_POS, True)
        if c.erank:
            E.check_erank_shape(c.B, c.S, c.H)
    except ValueError as e:
        return str(e)
    return None


@pytest.mark.parametrize("c", WC.CASES, ids=WC.case_id)
def test_row_admission_and_path(c):
    msg = admit(c)
    if c.refuse is None:
        assert msg is None, (c, msg)
    else:
        assert msg is not None and c.refuse in msg, (c, msg)
        if WC.engine_refused(c):
            with pytest.raises(ValueError):
                E.check_engine_shape(c.H, c.heads, WC.Q, **variant_kw(c))
        return
    dh = c.H // c.heads
    # the composed path: both hidden-128 chains refuse every row
    assert not E.fuser_chain_shape_ok(c.B, c.S, c.H, c.K, WC.Q, c.heads, c.variant == "bn")
    assert not E.decoder_chain_shape_ok(c.B, c.S, c.H, WC.Q, c.heads, 1)
    # engine.forward_begin / forward_finish: token fusion's fused embedding seam at hidden <= 1024 (train mode), the plain
    # fuser's seam in every mode, the BN-blend and activation-magnitude fusers' own seams after the selection
    assert c.variant in WC.SEAMS
    assert c.seam == (c.H <= 1024 if c.variant == "tf" else True), c
    assert c.tail1 == E.tail_in_decoder_chain(c.B, c.H, c.K, WC.Q)
    assert c.attn == ("small" if c.S <= 64 and dh in (16, 32, 64, 128) else "general")      # attention.hip mha_small_ok
    assert c.side == (c.H >= 512)                                       # FusionEngine._multi_stream
    assert ops.mha_core_supported(WC.Q, c.S, dh, True) and ops.mha_core_supported(WC.Q, WC.Q, dh, True)


def test_table_covers_what_the_issue_names():
    adm = [c for c in WC.CASES if c.refuse is None]
    assert {(c.H, c.heads) for c in adm} >= {(40, 8), (96, 8), (136, 8), (200, 8), (384, 6), (520, 8), (768, 12), (1032, 12),
                                            (2048, 16), (128, 4), (128, 1)}
    assert {c.variant for c in adm} == {"tf", "bn", "vary", "plain"}
    assert any(c.erank for c in adm) and any(not isinstance(c.pad, str) for c in adm)
    assert max(c.S for c in adm if c.H == 128) >= 1000
    for v in ("bn", "vary", "plain"):
        rows = [c for c in adm if c.variant == v]
        hs = {c.H for c in rows}
        # a row in every row-kernel bracket up to the seams' 1024 (EPL 2, 8, 16), one off the 64-column grid and one at 1024
        assert any(h <= 128 for h in hs) and any(128 < h <= 512 for h in hs) and any(512 < h <= 1024 for h in hs), (v, hs)
        assert 1024 in hs and any(h % 64 for h in hs if h > 512), (v, hs)
        assert (128, 4) in {(c.H, c.heads) for c in rows}, v
        assert any(c.attn == "small" for c in rows) and any(c.erank for c in rows), v
        assert any(not isinstance(c.pad, str) for c in rows), v
    assert {(c.variant, c.refuse) for c in WC.CASES if c.refuse and c.variant != "tf"} >= {
        ("bn", "BN-blend"), ("vary", "activation-magnitude"), ("plain", "plain SA-Fuser"), ("plain", "head width"),
        ("vary", "head width"), ("plain", "clip length")}


@pytest.mark.parametrize("H,heads,last,first", WC.CLIP_BOUNDS)
def test_clip_length_bound_flips_exactly(H, heads, last, first):
    assert E.max_clip_len(H, heads, WC.Q, 10 ** 5, True) == last
    E.check_clip_shape(last, H, heads, WC.Q, MAX_POS, True)
    with pytest.raises(ValueError, match="clip length .* LDS"):
        E.check_clip_shape(first, H, heads, WC.Q, MAX_POS, True)
    # the forward alone (validation) needs less LDS: the training bound admits it too
    E.check_clip_shape(first, H, heads, WC.Q, MAX_POS, False)


@pytest.mark.parametrize("H,heads,last,first,limit", WC.VAL_CLIP_BOUNDS)
def test_forward_only_clip_length_bound_flips_exactly(H, heads, last, first, limit):
    """The validation forward's bound: the forward attention core's LDS or pos_embedding's rows, whichever is smaller."""
    assert min(E.max_clip_len(H, heads, WC.Q, 10 ** 5, False), MAX_POS) == last
    assert E.max_clip_len(H, heads, WC.Q, MAX_POS, False) == last
    E.check_clip_shape(last, H, heads, WC.Q, MAX_POS, False)
    with pytest.raises(ValueError, match=limit):
        E.check_clip_shape(first, H, heads, WC.Q, MAX_POS, False)
    # the training bound is lower: the backward attention core keeps more in LDS
    assert E.max_clip_len(H, heads, WC.Q, MAX_POS, True) < last
    with pytest.raises(ValueError, match="clip length .* LDS"):
        E.check_clip_shape(last, H, heads, WC.Q, MAX_POS, True)


@pytest.mark.parametrize("v", WC.VAL_CASES, ids=WC.val_id)
def test_val_rows_are_admitted(v):
    variant, H, heads = v
    E.check_engine_shape(H, heads, WC.Q, bn=variant == "bn", vary=variant == "vary", plain=variant == "plain")
    E.check_clip_shape(16, H, heads, WC.Q, MAX_POS, False)
    assert not E.fuser_chain_shape_ok(2, 16, H, 17, WC.Q, heads, variant == "bn")


def test_val_table_covers_what_the_issue_names():
    assert {(v, H) for v, H, _ in WC.VAL_CASES} >= {(v, H) for v in ("tf", "bn", "vary", "plain") for H in (40, 136, 520, 1000)}
    assert {(v, H) for v, H, _ in WC.VAL_CASES if H > 1024} == {("tf", 1032), ("tf", 2048)}


@pytest.mark.parametrize("H,heads,last,first", WC.CLIP_BOUNDS)
def test_clip_bound_matches_the_attention_lds_formula(H, heads, last, first):
    """mha_lds_bytes (attention.hip), backward: 2 Lq dh + 3 Lq Lk + 128 (dh + 1) floats within 160 KiB."""
    dh, Lq = H // heads, WC.Q
    f = lambda Lk: (2 * Lq * dh + 3 * Lq * Lk + 128 * (dh + 1)) * 4      # noqa: E731
    assert f(last) <= 160 * 1024 < f(first)


def test_engine_shape_bounds_flip_exactly():
    E.check_engine_shape(1024, 8, WC.Q)                    # dh 128: 8 x 128 = 1024 outputs
    with pytest.raises(ValueError, match="head width 129"):
        E.check_engine_shape(1032, 8, WC.Q)
    E.check_engine_shape(2048, 16, WC.Q)
    with pytest.raises(ValueError, match="2048"):
        E.check_engine_shape(2056, 257, WC.Q)
    for bn, vary in ((True, False), (False, True)):
        E.check_engine_shape(1024, 8, WC.Q, bn=bn, vary=vary)
        with pytest.raises(ValueError, match="> 1024"):
            E.check_engine_shape(1032, 12, WC.Q, bn=bn, vary=vary)
        E.check_engine_shape(1032, 12, WC.Q)               # token fusion takes the un-seamed route there
    with pytest.raises(ValueError, match="hidden % 8"):
        E.check_engine_shape(132, 4, WC.Q)
    with pytest.raises(ValueError, match="hidden % n_head"):
        E.check_engine_shape(136, 16, WC.Q)


def test_rank_penalty_bound_flips_exactly():
    """The blocked Jacobi's two 2-column blocks of R-long columns within 150 KiB: R = max(B * S, H) <= 9596."""
    E.check_erank_shape(1, 9596, 128)
    E.check_erank_shape(4, 2399, 2048)
    with pytest.raises(ValueError, match="rank penalty"):
        E.check_erank_shape(1, 9597, 128)
    with pytest.raises(ValueError, match="rank penalty"):
        E.check_erank_shape(8, 1200, 128)


def test_clip_length_is_bounded_by_pos_embedding():
    E.check_clip_shape(MAX_POS, 128, 8, WC.Q, MAX_POS, False)
    with pytest.raises(ValueError, match="max_pos_len"):
        E.check_clip_shape(MAX_POS + 1, 128, 8, WC.Q, MAX_POS, False)
    with pytest.raises(ValueError, match="at least one frame"):
        E.check_clip_shape(0, 128, 8, WC.Q, MAX_POS, True)
