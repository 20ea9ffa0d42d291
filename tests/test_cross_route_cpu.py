"""Host side of the fusion engine's cross-attention route (engine.cross_attention_route, opts --long_clips) and of the
split-key core (csrc/attention_splitk.hip): the library's host-only predicates, the rule over every boundary row of
tests/width_cases.py, and a float64 restatement of the kernel's chunk partials and their combine -- the handling of -inf
(a chunk whose keys are all masked, a clip whose keys are all masked) pinned before any GPU run.  No GPU needed."""
import numpy as np
import pytest

from tests import width_cases as WC

MAX_POS = 2000


@pytest.fixture(scope="module")
def E():
    from r3d_amd import build, engine
    build.build(verbose=False)
    return engine


def _bounds():
    rows = [(H, heads, last, first, True) for H, heads, last, first in WC.CLIP_BOUNDS]
    rows += [(H, heads, last, first, False) for H, heads, last, first, _ in WC.VAL_CLIP_BOUNDS]
    return rows


@pytest.mark.parametrize("H,heads,last,first,train", _bounds())
def test_route_on_both_sides_of_every_clip_bound(E, H, heads, last, first, train):
    """Without the flag "core" up to the bound and None past it; with it "core" up to the bound (the same launches, whatever
    the flag) and "splitk" past it, up to max_pos_len.  (At hidden 128 a forward alone is bounded by max_pos_len, not by
    the core: the rows past it are judged by check_clip_shape.)"""
    dh = H // heads
    core_last = E.max_clip_len(H, heads, WC.Q, 10 ** 5, train)
    assert min(core_last, MAX_POS) == last
    for S in (1, 64, 65, last):
        assert E.cross_attention_route(WC.Q, S, dh, train, False) == "core"
        assert E.cross_attention_route(WC.Q, S, dh, train, True) == "core"
    for S in (core_last + 1, core_last + 2, 2 * core_last) + ((MAX_POS,) if MAX_POS > core_last else ()):
        assert E.cross_attention_route(WC.Q, S, dh, train, False) is None, S
        assert E.cross_attention_route(WC.Q, S, dh, train, True) == "splitk", S
    # through check_clip_shape: the flag admits everything up to max_pos_len, and nothing past it
    E.check_clip_shape(last, H, heads, WC.Q, MAX_POS, train)
    E.check_clip_shape(last, H, heads, WC.Q, MAX_POS, train, long_clips=True)
    if first <= MAX_POS:
        with pytest.raises(ValueError, match=f"clip length {first} at head width {dh}.*--long_clips"):
            E.check_clip_shape(first, H, heads, WC.Q, MAX_POS, train)
        E.check_clip_shape(first, H, heads, WC.Q, MAX_POS, train, long_clips=True)
    E.check_clip_shape(MAX_POS, H, heads, WC.Q, MAX_POS, train, long_clips=True)
    for flag in (False, True):
        with pytest.raises(ValueError, match="max_pos_len") as e:
            E.check_clip_shape(MAX_POS + 1, H, heads, WC.Q, MAX_POS, train, long_clips=flag)
        assert "long_clips" not in str(e.value)
    assert E.max_clip_len(H, heads, WC.Q, MAX_POS, train, long_clips=True) == MAX_POS
    assert E.max_clip_len(H, heads, WC.Q, MAX_POS, train) == last


def test_more_than_sixteen_queries_take_the_tiled_core(E):
    dh, Q = 16, 24
    S = E.max_clip_len(8 * dh, 8, Q, 10 ** 5, True) + 1            # the first clip past the core with 24 queries
    assert 1 < S <= MAX_POS
    assert E.cross_attention_route(Q, S - 1, dh, True, True) == "core"
    assert E.cross_attention_route(Q, S, dh, True, False) is None
    assert E.cross_attention_route(Q, S, dh, True, True) == "tiled"
    assert E.cross_attention_route(Q, MAX_POS, dh, True, True) == "tiled"
    assert E.cross_attention_route(16, MAX_POS, dh, True, True) == "splitk"
    assert E.cross_attention_route(17, MAX_POS, dh, True, True) == "tiled"
    assert E.cross_attention_route(8, MAX_POS, 129, True, True) is None          # no core runs head width 129


def test_the_hint_is_appended_only_where_the_flag_would_admit(E):
    with pytest.raises(ValueError) as e:
        E.check_clip_shape(1606, 128, 8, WC.Q, MAX_POS, True)
    msg = str(e.value)
    assert msg.startswith("clip length 1606 at head width 16: the cross-attention core's backward keeps 8 x 1606 scores in LDS, "
                          "past its 160 KiB")
    assert msg.endswith("--long_clips)")
    with pytest.raises(ValueError) as e:          # head width 256: no route, no hint
        E.check_clip_shape(1606, 2048, 8, WC.Q, MAX_POS, True)
    assert "long_clips" not in str(e.value)


def test_cross_route_names(E):
    assert E.CROSS_ROUTES == ("core", "splitk", "tiled")
    assert E.cross_route_supported("splitk", 8, 16, 17, True) and not E.cross_route_supported("splitk", 17, 16, 17, True)
    assert E.cross_route_supported("tiled", 24, 16, 17, True) and not E.cross_route_supported("core", 8, 1606, 16, True)
    with pytest.raises(ValueError, match="cross_route"):
        E.cross_route_supported("flash", 8, 16, 16, True)


def test_splitk_host_predicates(E):
    from r3d_amd import ops
    for bwd in (False, True):
        assert ops.mha_splitk_supported(1, 1, 1, bwd) and ops.mha_splitk_supported(16, 2000, 128, bwd)
        assert not ops.mha_splitk_supported(17, 64, 16, bwd)
        assert not ops.mha_splitk_supported(8, 64, 129, bwd)
        assert not ops.mha_splitk_supported(0, 64, 16, bwd) and not ops.mha_splitk_supported(8, 0, 16, bwd)
        assert not ops.mha_splitk_supported(8, 64, 0, bwd)
    for Lk in (1, 63, 64, 65, 300, 1142, 2000, 10 ** 6):
        for dh in (1, 5, 16, 25, 64, 128):
            C = ops.mha_splitk_chunk(Lk, dh)
            assert C > 0 and C % 64 == 0, (Lk, dh, C)
            assert C == ops.mha_splitk_chunk(Lk, dh)
            n = -(-Lk // C)
            assert ops.mha_splitk_ws_floats(3, 8, 8, Lk, dh, False) == 3 * 8 * n * 8 * (dh + 2)
            assert ops.mha_splitk_ws_floats(3, 8, 8, Lk, dh, True) == 3 * 8 * n * 8 * dh
    assert ops.mha_splitk_ws_floats(3, 8, 17, 64, 16, True) == 0


def test_flag_reaches_the_four_fuser_models():
    import argparse
    import importlib
    import torch
    from r3d_amd import opts
    assert opts.parser.parse_args([]).long_clips is False and opts.parser.parse_args(["--long_clips"]).long_clips is True
    for name in ("futr_safuser_tokenfusion", "futr_safuser_tokenfusion_vary", "futr_safuser_batchnormalization",
                 "futr_safuser_depth"):
        FUTR = importlib.import_module(f"r3d_amd.model.{name}").FUTR
        for flag in (True, False):
            args = argparse.Namespace(input_dim=12, seg=True, anticipate=True, max_pos_len=50, input_type="i3d_transcript",
                                      long_clips=flag)
            m = FUTR(5, 64, 6, torch.device("cpu"), args, n_query=8, n_head=8, num_encoder_layers=1, num_decoder_layers=1,
                     depth_pixels=12)
            assert m.r3d_long_clips is flag, name
        del args.long_clips
        assert FUTR(5, 64, 6, torch.device("cpu"), args, n_query=8, n_head=8, num_encoder_layers=1, num_decoder_layers=1,
                    depth_pixels=12).r3d_long_clips is False


# ---- the kernel's arithmetic, restated in float64 -------------------------------------------------------------------------
def _chunk_partials(s, v, keepf, C):
    """Per chunk of C keys, as the forward kernel writes them: (m_c, l_c, acc_c).  s [Lq, Lk] with -inf at masked keys.  Inside
    a chunk the kernel subtracts 0 instead of a maximum of -inf, so that exp(-inf - m) is 0 and never NaN."""
    parts = []
    for k0 in range(0, s.shape[1], C):
        sc, vc, kc = s[:, k0:k0 + C], v[k0:k0 + C], keepf[:, k0:k0 + C]
        m = sc.max(axis=1)
        mu = np.where(np.isneginf(m), 0.0, m)
        p = np.exp(sc - mu[:, None])
        parts.append((m, p.sum(axis=1), (p * kc) @ vc))
    return parts


def _combine(parts):
    """The combine launch: chunks in chunk order; all keys masked: 0 / 0 = NaN rows and lse = -inf."""
    m = np.max(np.stack([p[0] for p in parts]), axis=0)
    mu = np.where(np.isneginf(m), 0.0, m)
    l, o = 0.0, 0.0
    for mc, lc, acc in parts:
        f = np.exp(mc - mu)
        l = l + lc * f
        o = o + acc * f[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return o / l[:, None], m + np.log(l)


@pytest.mark.parametrize("mask", ["none", "first_chunk", "last_one", "all"])
@pytest.mark.parametrize("C", [64, 128])
def test_chunk_partials_and_combine_equal_the_masked_softmax_product(mask, C):
    rng = np.random.default_rng(7)
    Lq, Lk, dh = 8, 2 * C + 1, 16
    s = rng.standard_normal((Lq, Lk)) * 3.0
    v = rng.standard_normal((Lk, dh))
    keepf = (rng.random((Lq, Lk)) > 0.1) / 0.9
    masked = np.zeros(Lk, dtype=bool)
    if mask == "first_chunk":
        masked[:C] = True
    elif mask == "last_one":                  # a single valid key, in the last chunk: every other chunk is wholly masked
        masked[:] = True
        masked[Lk - 1] = False
    elif mask == "all":
        masked[:] = True
    s[:, masked] = -np.inf
    with np.errstate(invalid="ignore"):
        o, lse = _combine(_chunk_partials(s, v, keepf, C))
    if mask == "all":
        assert np.isnan(o).all() and np.isneginf(lse).all()
        return
    m = s.max(axis=1, keepdims=True)
    p = np.exp(s - m)
    want = ((p / p.sum(axis=1, keepdims=True)) * keepf) @ v
    assert np.isfinite(o).all() and np.isfinite(lse).all()
    np.testing.assert_allclose(o, want, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(lse, (m + np.log(p.sum(axis=1, keepdims=True)))[:, 0], rtol=1e-12, atol=1e-13)
    if mask == "last_one":
        np.testing.assert_allclose(o, keepf[:, -1:] * v[-1][None, :], rtol=1e-12, atol=1e-13)
