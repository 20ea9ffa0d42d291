"""The admission predicates of the hidden-128 chain kernels are host-only: every row of tests/chain_cases.py must route to
the path its row states, and the boundaries of each predicate stay where the kernels' tiling puts them.  A predicate
change shows up here before anything runs on a GPU."""
import pytest

from tests import chain_cases as CC


@pytest.fixture(scope="module")
def lib():
    from r3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def routed(c):
    """The path the engine's own shape predicates give a case row (training step, default switches)."""
    from r3d_amd import engine as E
    fuser = E.fuser_chain_shape_ok(c.B, c.S, CC.H, c.K, CC.Q, CC.HEADS)
    dec = E.decoder_chain_shape_ok(c.B, c.S, CC.H, CC.Q, CC.HEADS, 1)
    return dict(fuser=fuser, bwd=("bf3" if E.bwd_chain_bf3(True, c.K) else "fp32") if fuser else None, dec=dec,
                defer=bool(dec and E.tail_in_decoder_chain(c.B, CC.H, c.K, CC.Q)))


@pytest.mark.parametrize("c", CC.CASES, ids=CC.case_id)
def test_case_table_paths_match_the_predicates(lib, c):
    assert routed(c) == dict(fuser=c.fuser, bwd=c.bwd, dec=c.dec, defer=c.defer), c.why


@pytest.mark.parametrize("B,S,K,dec", CC.VAL_CASES, ids=[f"val-B{b}-S{s}-K{k}" for b, s, k, _ in CC.VAL_CASES])
def test_val_case_paths_match_the_predicates(lib, B, S, K, dec):
    """Validation forwards at B = 1: the fuser chain's query role is refused (B*Q = 8), the decoder chain as the row says."""
    from r3d_amd import engine as E
    assert not E.fuser_chain_shape_ok(B, S, CC.H, K, CC.Q, CC.HEADS)
    assert E.decoder_chain_shape_ok(B, S, CC.H, CC.Q, CC.HEADS, 1) == dec


def test_case_table_covers_every_path():
    rows = CC.CASES
    assert any(c.fuser and c.bwd == "bf3" for c in rows) and any(c.fuser and c.bwd == "fp32" for c in rows)
    assert any(not c.fuser and c.dec for c in rows) and any(c.fuser and not c.dec for c in rows)
    assert any(c.defer for c in rows) and any(c.dec and not c.defer for c in rows)
    assert {c.S for c in rows} >= {1, 7, 63, 64, 65} and {c.B for c in rows} >= {8, 9, 10, 16, 32}
    assert {c.K for c in rows} >= {23, 24, 32, 33, 128, 129, 122}
    assert CC.CASES[0][:4] == (8, 16, 17, "tail") and CC.CASES[0].fuser and CC.CASES[0].dec and CC.CASES[0].defer


def test_fuser_chain_boundaries(lib):
    f = lib.r3d_fuser_chain_supported
    assert f(128, 128, 128, 8, 8, 8) == 1 and f(128, 128, 129, 8, 8, 8) == 0      # K <= 128 (8 segmentation-head tiles)
    assert f(128, 128, 1, 8, 8, 8) == 1 and f(128, 128, 0, 8, 8, 8) == 0
    assert f(56, 128, 17, 8, 8, 8) == 1 and f(60, 128, 17, 10, 8, 8) == 0          # 2N % 16: N = 56 yes, N = 60 no
    assert f(8, 128, 17, 8, 8, 8) == 1 and f(4, 128, 17, 4, 8, 8) == 0             # S = 1: 2N = 16 yes, 2N = 8 no
    assert f(144, 128, 17, 9, 8, 8) == 0 and f(120, 128, 17, 10, 8, 8) == 1        # B*Q = 72 no, 80 yes
    assert f(128, 64, 17, 8, 8, 8) == 0 and f(128, 256, 17, 8, 8, 8) == 0          # hidden 128 only
    assert f(128, 128, 17, 8, 4, 8) == 0 and f(128, 128, 17, 8, 8, 4) == 0         # 8 queries, 8 heads


def test_decoder_chain_boundaries(lib):
    d = lib.r3d_decoder_chain_supported
    assert [d(128, 8, 8, s) for s in (0, 1, 7, 63, 64, 65)] == [0, 1, 1, 1, 1, 0]
    assert d(64, 8, 8, 16) == 0 and d(128, 4, 8, 16) == 0 and d(128, 8, 4, 16) == 0


def test_tail_in_chain_and_backward_precision_boundaries(lib):
    from r3d_amd import engine as E
    t = lib.r3d_decoder_tail_losses_supported
    assert t(128, 24, 8, 64) == 1 and t(128, 25, 8, 64) == 0                       # K + 1 <= 24
    assert t(128, 18, 8, 1024) == 1 and t(128, 18, 8, 1032) == 0
    assert E.tail_in_decoder_chain(8, 128, 23, 8) and not E.tail_in_decoder_chain(8, 128, 24, 8)
    assert E.BWD_BF3_MAX_K == 32
    assert E.bwd_chain_bf3(True, 32) and not E.bwd_chain_bf3(True, 33) and not E.bwd_chain_bf3(False, 17)
    # the decoder chain's own limit on the engine side: B*Q <= 1024 rows
    assert E.decoder_chain_shape_ok(128, 16, 128, 8, 8, 1) and not E.decoder_chain_shape_ok(129, 16, 128, 8, 8, 1)
    assert not E.decoder_chain_shape_ok(8, 16, 128, 8, 8, 2)                      # one decoder layer only
    assert not E.fuser_chain_shape_ok(8, 16, 128, 17, 8, 8, bn=True)              # the BN-blend variant never takes it
