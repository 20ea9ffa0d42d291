"""Host side of the tiled attention route (csrc/attention_tiled.hip, opts --long_clips): the library's own host-only
r3d_mha_tiled_supported, engine_unsup's route rule and admission predicates with the flag on, and -- with the flag off --
exactly today's answers for every row of tests/query_cases.py.  No GPU."""
import pytest

from r3d_amd import engine_unsup as U, ops
from tests import query_cases as QC

MAX_POS = 2000


@pytest.fixture(scope="module", autouse=True)
def lib():
    from r3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("bwd", [False, True])
def test_tiled_supported_states_the_limits(bwd):
    for Lq, Lk, dh in [(65, 65, 16), (2000, 2000, 128), (1, 1, 1), (70, 133, 5)]:
        assert ops.mha_tiled_supported(Lq, Lk, dh, bwd) is True, (Lq, Lk, dh)
    for Lq, Lk, dh in [(65, 65, 129), (65, 65, 0), (0, 65, 16), (65, 0, 16), (-1, 5, 16), (5, 5, -4)]:
        assert ops.mha_tiled_supported(Lq, Lk, dh, bwd) is False, (Lq, Lk, dh)


@pytest.mark.parametrize("H,heads,S,route", [(128, 8, 64, "core"), (128, 8, 65, "tiled"), (64, 8, 113, "tiled"),
                                             (1024, 8, 9, "tiled"), (2048, 8, 5, None)])
def test_route_table_with_the_flag_on(H, heads, S, route):
    assert U.query_attention_route(S, H, heads, True, True) == route
    if route == "tiled":                     # the same shape without the flag: refused, and the message names the flag
        assert U.query_attention_route(S, H, heads, True, False) is None
        with pytest.raises(ValueError, match=f"clip length {S} at head width {H // heads}.*--long_clips"):
            U.check_query_clip_shape(S, H, heads, MAX_POS, True)
        U.check_query_clip_shape(S, H, heads, MAX_POS, True, long_clips=True)
    if route is None:                        # head widths above 128 keep today's limit and message, flag or not
        with pytest.raises(ValueError, match=f"clip length {S} at head width {H // heads}") as e:
            U.check_query_clip_shape(S, H, heads, MAX_POS, True, long_clips=True)
        assert "long_clips" not in str(e.value)


def test_forward_alone_stays_on_the_core_where_it_fits():
    assert U.query_attention_route(113, 64, 8, False, True) == "core"
    assert U.query_attention_route(113, 64, 8, False, False) == "core"
    assert U.query_attention_route(300, 128, 8, False, True) == "tiled"


def test_flag_lifts_the_clip_bound_to_the_positional_tables():
    assert U.max_query_clip_len(128, 8, 2000, True, long_clips=True) == 2000
    assert U.max_query_clip_len(1024, 8, 2000, True, long_clips=True) == 2000
    assert U.max_query_clip_len(2048, 8, 2000, True, long_clips=True) == 4           # dh 256: today's bound
    assert U.max_query_clip_len(2048, 4, 2000, True, long_clips=True) == 0
    U.check_query_clip_shape(2000, 128, 8, MAX_POS, True, long_clips=True)
    with pytest.raises(ValueError, match="max_pos_len"):
        U.check_query_clip_shape(2001, 128, 8, MAX_POS, True, long_clips=True)
    with pytest.raises(ValueError, match="at least one frame"):
        U.check_query_clip_shape(0, 128, 8, MAX_POS, True, long_clips=True)
    U.check_query_engine_shape(1024, 8, long_clips=True)
    with pytest.raises(ValueError, match="head width 512"):
        U.check_query_engine_shape(2048, 4, long_clips=True)


def _answer(fn, *a, **k):
    try:
        return fn(*a, **k)
    except ValueError as e:
        return str(e).split(" (the tiled core runs this shape")[0]       # (the hint is appended to today's message)


@pytest.mark.parametrize("c", QC.CASES, ids=QC.case_id)
def test_flag_off_is_todays_answer_for_every_row(c):
    dh = c.H // c.heads
    for train in (True, False):
        got = _answer(U.check_query_clip_shape, c.S, c.H, c.heads, MAX_POS, train)
        assert got == _answer(U.check_query_clip_shape, c.S, c.H, c.heads, MAX_POS, train, long_clips=False)
        admitted = ops.mha_core_supported(c.S, c.S, dh, train)              # today's rule: the core alone
        assert (got is None) == admitted, (c, got)
        assert U.query_attention_route(c.S, c.H, c.heads, train, False) == ("core" if admitted else None)
    if c.refuse == "clip length":
        msg = _answer(U.check_query_clip_shape, c.S, c.H, c.heads, MAX_POS, True)
        assert msg.startswith(f"clip length {c.S} at head width {dh}: the decoder's attention cores run") and \
            msg.endswith("S x S scores in 160 KiB of LDS"), msg
    if QC.engine_refused(c):
        with pytest.raises(ValueError, match=c.refuse):
            U.check_query_engine_shape(c.H, c.heads)
    else:
        U.check_query_engine_shape(c.H, c.heads)


@pytest.mark.parametrize("H,heads,dh,last", QC.QUERY_BOUNDS)
def test_flag_off_keeps_the_clip_bounds(H, heads, dh, last):
    assert U.max_query_clip_len(H, heads, 10 ** 5, True) == last
    assert U.max_query_clip_len(H, heads, 10 ** 5, True, long_clips=False) == last
    assert U.query_attention_route(last + 1, H, heads, True, False) is None
    # with the flag the core still takes every clip it took: same launches, same bits for short clips
    for S in ((1, last) if last else ()):
        assert U.query_attention_route(S, H, heads, True, True) == "core"


def test_option_defaults_to_off_and_reaches_the_models():
    import argparse
    import torch
    from r3d_amd import opts
    assert opts.parser.parse_args([]).long_clips is False
    assert opts.parser.parse_args(["--long_clips"]).long_clips is True
    from r3d_amd.model.futr_unsupervised_depth import FUTR as Depth
    from r3d_amd.model.futr_proposed import FUTR as Label
    for flag in (False, True):
        args = argparse.Namespace(input_dim=32, seg=True, anticipate=True, max_pos_len=16, input_type="i3d_transcript",
                                  long_clips=flag)
        kw = dict(n_query=8, n_head=8, num_encoder_layers=1, num_decoder_layers=1)
        assert Depth(5, 64, 6, torch.device("cpu"), args, depth_pixels=12, **kw).r3d_long_clips is flag
        assert Label(5, 64, 6, torch.device("cpu"), args, **kw).r3d_long_clips is flag
    del args.long_clips
    assert Depth(5, 64, 6, torch.device("cpu"), args, depth_pixels=12, **kw).r3d_long_clips is False
