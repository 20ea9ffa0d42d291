"""Every row of tests/query_cases.py against the query models' host-side admission predicates, the predicates' boundaries and
README's table of them (no GPU: the attention limit is the library's own host-only r3d_mha_core_supported)."""
import os
import re

import pytest

from r3d_amd import engine_unsup as U, ops
from tests import query_cases as QC

MAX_POS = 2000                  # the reference's max_pos_len
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def lib():
    from r3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def admit(c, train=True):
    """None if the row's step (train) or forward alone is admitted, else the ValueError's message."""
    try:
        U.check_query_engine_shape(c.H, c.heads)
        U.check_query_clip_shape(c.S, c.H, c.heads, MAX_POS, train)
    except ValueError as e:
        return str(e)
    return None


@pytest.mark.parametrize("c", QC.CASES, ids=QC.case_id)
def test_row_admission_and_route(c):
    msg = admit(c)
    assert (admit(c, train=False) is None) == c.fwd, (c, admit(c, train=False))
    if c.refuse is not None:
        assert msg is not None and c.refuse in msg, (c, msg)
        if QC.engine_refused(c):
            with pytest.raises(ValueError, match=c.refuse):
                U.check_query_engine_shape(c.H, c.heads)
        else:
            U.check_query_engine_shape(c.H, c.heads)
        return
    assert msg is None, (c, msg)
    dh = c.H // c.heads
    assert c.attn == ("small" if QC.small_route(c.S, dh) else "general"), c
    # both decoder attentions run S queries against S keys, forward and backward
    assert ops.mha_core_supported(c.S, c.S, dh, False) and ops.mha_core_supported(c.S, c.S, dh, True)
    assert c.S <= U.max_query_clip_len(c.H, c.heads, MAX_POS, True)


def test_table_covers_what_the_issue_names():
    adm = [c for c in QC.CASES if c.refuse is None]
    dh = lambda c: c.H // c.heads      # noqa: E731
    assert {(c.S, dh(c)) for c in adm if c.variant == "depth"} >= {(1, 16), (7, 5), (8, 16), (8, 128), (9, 16), (64, 16),
                                                                   (112, 8), (40, 25), (15, 65), (4, 256)}
    assert {c.heads for c in adm} >= {1, 6, 8} and max(c.n_dec for c in adm) >= 3 and max(c.K for c in adm) == 122
    assert any(not isinstance(c.pad, str) for c in adm)
    assert {c.S for c in adm if c.variant == "label"} >= {5, 9, 64} and QC.N_USED < QC.QUERY_NUM
    assert {c.attn for c in adm} == {"small", "general"}
    ref = [c for c in QC.CASES if c.refuse is not None]
    assert {(c.S, dh(c)) for c in ref if c.refuse == "clip length"} == {(65, 16), (17, 64), (113, 8)}
    assert any(c.fwd for c in ref) and {(c.H, c.heads) for c in ref if QC.engine_refused(c)} == {(2048, 4), (2056, 8)}


@pytest.mark.parametrize("H,heads,dh,last", QC.QUERY_BOUNDS)
def test_clip_length_bound_flips_exactly(H, heads, dh, last):
    assert H // heads == dh
    assert U.max_query_clip_len(H, heads, 10 ** 5, True) == last
    if last:
        U.check_query_engine_shape(H, heads)
        U.check_query_clip_shape(last, H, heads, MAX_POS, True)
    else:
        with pytest.raises(ValueError, match=f"head width {dh}"):
            U.check_query_engine_shape(H, heads)
    with pytest.raises(ValueError, match="clip length"):
        U.check_query_clip_shape(last + 1, H, heads, MAX_POS, True)
    assert ops.mha_core_supported(last + 1, last + 1, dh, True) is False
    # the forward alone needs less LDS: its bound is never shorter
    assert U.max_query_clip_len(H, heads, 10 ** 5, False) >= last


@pytest.mark.parametrize("H,heads,dh,last", QC.QUERY_BOUNDS)
def test_clip_bound_matches_the_attention_formula(H, heads, dh, last):
    """attention.hip, Lq = Lk = S: S * dh <= 1024 outputs per wave, and the backward's mha_lds_bytes
    (2 S dh + 3 S^2 + 128 (dh + 1) floats) within 160 KiB; the forward's is S dh + 2 S^2 + 128 (dh + 1)."""
    ok = lambda S, bwd: S * dh <= 1024 and ((2 if bwd else 1) * S * dh + (3 if bwd else 2) * S * S      # noqa: E731
                                            + 128 * (dh + 1)) * 4 <= 160 * 1024
    assert (last == 0 or ok(last, True)) and not ok(last + 1, True)
    fwd_last = U.max_query_clip_len(H, heads, 10 ** 5, False)
    assert (fwd_last == 0 or ok(fwd_last, False)) and not ok(fwd_last + 1, False)


def test_engine_shape_bounds_flip_exactly():
    U.check_query_engine_shape(2048, 8)                    # dh 256: S <= 4
    with pytest.raises(ValueError, match="head width 512"):
        U.check_query_engine_shape(2048, 4)
    with pytest.raises(ValueError, match="hidden 2056 > 2048"):
        U.check_query_engine_shape(2056, 8)
    with pytest.raises(ValueError, match="hidden % 8"):
        U.check_query_engine_shape(132, 4)
    with pytest.raises(ValueError, match="hidden % n_head"):
        U.check_query_engine_shape(136, 16)
    # the widest head that trains at all: one frame, 2 dh + 3 + 128 (dh + 1) floats within 160 KiB -> dh <= 314
    U.check_query_engine_shape(314 * 4, 4)
    assert U.max_query_clip_len(314 * 4, 4, MAX_POS, True) == 1
    with pytest.raises(ValueError, match="head width 316"):
        U.check_query_engine_shape(316 * 2, 2)


def test_clip_length_is_bounded_by_the_positional_tables():
    U.check_query_clip_shape(8, 128, 8, 8, True)
    with pytest.raises(ValueError, match="max_pos_len"):
        U.check_query_clip_shape(9, 128, 8, 8, True)
    with pytest.raises(ValueError, match="at least one frame"):
        U.check_query_clip_shape(0, 128, 8, MAX_POS, True)
    assert U.max_query_clip_len(32, 8, 100, True) == 100       # (the positional tables bind before the attention core)


def test_readme_states_the_limits_the_helper_computes():
    """README's "Supported shapes" table of the query models' longest training clip is the helper's output."""
    text = open(os.path.join(ROOT, "README.md")).read()
    widths = re.search(r"^\| head width \|(.*)\|$", text, re.M)
    longest = re.search(r"^\| longest training S \|(.*)\|$", text, re.M)
    assert widths and longest, "README lost the query models' clip-length table"
    cells = lambda m: [x.strip() for x in m.group(1).split("|")]       # noqa: E731
    got = dict(zip(cells(widths), cells(longest)))
    want = {str(dh): str(last) if last else "none" for _, _, dh, last in QC.QUERY_BOUNDS}
    assert got == want
    for H, heads, dh, last in QC.QUERY_BOUNDS:
        assert U.max_query_clip_len(H, heads, MAX_POS, True) == last
