"""Sanity of tests/gemm_f32_cases.py: the table keeps covering what tests/test_gemm_f32_gpu.py claims to pin (tiles,
layouts, grid modes, epilogues), every row is one gemm_validate admits, and r3d_gemm_plan does put an engine's TN
bias_grad product on the k-split-wave tile 4.  Nothing here needs a GPU."""
import ctypes as C

import pytest

from tests import gemm_f32_cases as G


def _raw_like(c):
    return c.kind in ("raw", "bias_grad")


def test_every_grid_mode_occurs_at_its_edges():
    modes = {}
    for c in G.CASES:
        if c.kind == "adam":
            continue
        mode, Gm, NG = G.case_mode(c)
        modes.setdefault(mode, []).append((c, Gm, NG))
    assert set(modes) == {0, 1, 2, 3}
    for mode in (2, 3):
        assert any(NG % 8 != 0 for _, _, NG in modes[mode]), f"mode {mode}: no group count off the XCD count"
        assert any(NG % 8 == 0 for _, _, NG in modes[mode]), f"mode {mode}: no group count on the XCD count"
        assert any(Gm == 16 for _, Gm, _ in modes[mode]), f"mode {mode}: never at its 16-member limit"
        assert any(Gm == 2 for _, Gm, _ in modes[mode]), f"mode {mode}: never at its 2-member limit"
        assert {c.layout for c, _, _ in modes[mode]} == {G.NT, G.NN, G.TN}
        assert {c.tile for c, _, _ in modes[mode]} >= {1, 2}
    assert any(c.tile == 5 for c, _, _ in modes[2])
    assert any(Gm == 32 and NG % 8 != 0 for _, Gm, NG in modes[1]), "mode 1 never at its 32-tile limit"
    assert {c.layout for c, Gm, _ in modes[1] if Gm == 32} == {G.NT, G.NN, G.TN}
    assert any(G.tiles_of(c) == 33 and G.nsplits(c.K, c.splitk) > 1 for c, _, _ in modes[0]), "no 33-tile split-K launch"
    # the first shapes past each rule stay on the plain grid
    past = {(G.cdiv(c.M, 32), G.cdiv(c.N, 32)) for c, _, _ in modes[0] if c.tile == 1 and c.splitk == 1}
    assert {(17, 17), (2, 15), (1, 17), (15, 2)} <= past


def test_grid_mode_rule():
    """the rule itself at its boundaries (tile 1: 32 x 32)"""
    assert G.grid_mode(1, 64, 512, 1) == (2, 2, 16) and G.grid_mode(1, 64, 480, 1) == (0, 1, 1)
    assert G.grid_mode(1, 512, 512, 1) == (2, 16, 16)               # both rules hold: mode 2 wins
    assert G.grid_mode(1, 544, 512, 1) == (3, 16, 17) and G.grid_mode(1, 544, 544, 1) == (0, 1, 1)
    assert G.grid_mode(1, 32, 1024, 1) == (0, 1, 1)
    assert G.grid_mode(1, 128, 256, 9) == (1, 32, 9) and G.grid_mode(1, 96, 352, 9) == (0, 1, 1)
    assert G.grid_mode(1, 32, 32, 9) == (0, 1, 1)                   # a single tile: nothing to place
    assert G.grid_mode(5, 130, 2050, 1) == (2, 2, 17) and G.grid_mode(3, 130, 2050, 2) == (0, 1, 1)
    for row in G.GRID_ROWS:
        tile, (M, N, K), sk, what = row
        assert what.startswith(f"mode {G.grid_mode(tile, M, N, G.nsplits(K, sk))[0]}:"), row


@pytest.mark.parametrize("tile", G.KSPLIT_WAVE_TILES)
def test_ksplit_wave_tiles_are_covered(tile):
    rows = [c for c in G.CASES if c.tile == tile]
    for L in (G.NT, G.NN, G.TN):
        for pad in (0, 3):
            assert any(c.kind == "raw" and c.layout == L and c.pad == pad and c.splitk == 1 for c in rows), (L, pad)
            assert any(c.kind == "raw" and c.layout == L and c.pad == pad and G.nsplits(c.K, c.splitk) > 1 for c in rows), (L, pad)
    for pad in (0, 3):
        for epi in (frozenset(), frozenset({"b_add"})):
            assert any(c.kind == "bias_grad" and c.pad == pad and c.epi == epi for c in rows), (pad, epi)
    # more than one row tile writes bias_grad, and more than one column tile has the chance to
    bg = [c for c in rows if c.kind == "bias_grad"]
    assert any(G.cdiv(c.M, G.TILE_SZ[tile]) > 1 and G.cdiv(c.N, G.TILE_SZ[tile]) > 1 for c in bg)
    # one k-step, an odd and an even number of them, and a last step that is not full
    steps = {G.k_steps(c) for c in rows if c.kind == "raw" and c.splitk == 1}
    assert 1 in steps and any(s > 1 and s % 2 for s in steps) and any(s % 2 == 0 for s in steps), steps
    assert any(c.K % G.TILE_BK[tile] for c in rows if c.kind == "raw")
    assert any(c.kind == "epi" and G.nsplits(c.K, c.splitk) > 1 for c in rows)


@pytest.mark.parametrize("tile", G.EPI_TILES)
def test_every_large_tile_gets_the_full_epilogue(tile):
    rows = [c for c in G.CASES if c.tile == tile]
    epi = [c for c in rows if c.kind == "epi"]
    assert {(c.M, c.N, c.K) for c in epi if c.layout == G.NT} >= set(G.EPI_SHAPES)
    for sk in (1, 3):
        assert any(c.layout == G.NT and c.splitk == sk and {"a_add", "a_row_xor"} <= c.epi for c in epi), sk
    assert any(c.layout == G.NN and {"a_add", "a_row_xor"} <= c.epi for c in epi)
    assert any(c.M % G.TILE_SZ[tile] and c.N % G.TILE_SZ[tile] for c in epi), "no ragged epilogue shape"
    assert {c.splitk for c in rows if c.kind == "xor"} == {1, 3}
    assert any(G.nsplits(c.K, c.splitk) > 1 for c in epi), "splitk asked for but no slab made"


def test_adam_and_grouped_rows_are_covered():
    adam = [c for c in G.CASES if c.kind == "adam"]
    for t in (2, 3, 0):
        assert {c.layout for c in adam if c.tile == t} == {G.TN, G.NT}
        assert {(c.M, c.N, c.K) for c in adam if c.tile == t} == set(G.ADAM_SHAPES)
    # a shape whose last float4 column group ends exactly at N inside a tile, and one that fills its tiles
    assert any(c.N % G.TILE_SZ[2] for c in adam) and any(c.N % G.TILE_SZ[2] == 0 for c in adam)
    have = {(g.layout, g.tile) for g in G.GROUP_CASES}
    assert {(G.NN, 1), (G.NN, 2), (G.NT, 2)} <= have
    used = {p[3] for g in G.GROUP_CASES for p in g.problems}
    assert used == set(G.GROUP_EPI), "an engine keyword set is in no group"
    assert any(len(g.problems) > 32 for g in G.GROUP_CASES)


def _validate(kind, layout, tile, M, N, K, splitk, epi, ldc=None):
    """gemm_validate's rules that need no pointer (csrc/gemm_f32.hip)"""
    assert M > 0 and N > 0 and K > 0 and layout in (0, 1, 2) and 1 <= tile <= 5
    ns = G.nsplits(K, splitk)
    if layout == G.TN:
        assert not ({"a_add", "a_row_xor"} & epi)
    if layout == G.NT:
        assert "b_add" not in epi
    if {"a_row_xor", "c_row_xor"} & epi or kind == "xor":
        assert M % 2 == 0, "the pair swap needs an even row count"
    if kind == "bias_grad":
        assert layout == G.TN and ns == 1
    if kind == "adam":
        assert tile in (2, 3) and ns == 1 and N % 4 == 0 and ldc % 4 == 0 and ldc > N and G.ADAM["alpha"] != 0
        assert not epi
    if ns > 1:
        kps = G.cdiv(G.cdiv(K, splitk), 16) * 16
        assert kps % 16 == 0 and G.cdiv(K, kps) == ns <= splitk
    if "mul1" in epi or "mul2" in epi:
        assert "aux" in epi


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_row_is_admitted(c):
    assert c.kind in ("raw", "bias_grad", "epi", "xor", "adam") and c.pad in (0, 3)
    tiles = (2, 3) if (c.kind == "adam" and c.tile == 0) else (c.tile,)
    for t in tiles:
        _validate(c.kind, c.layout, t, c.M, c.N, c.K, c.splitk, c.epi, ldc=c.N + G.ADAM_LDC_PAD)
    if c.kind == "epi":
        assert c.M % 2 == 0 or "a_row_xor" not in c.epi


@pytest.mark.parametrize("g", G.GROUP_CASES, ids=G.group_id)
def test_group_is_admitted(g):
    assert g.tile in (1, 2)                       # r3d_gemm_grouped_prepare takes no other
    for (M, N, K, name) in g.problems:
        _validate("raw", g.layout, g.tile, M, N, K, 1, G.GROUP_EPI[name])


def test_case_ids_are_unique():
    ids = [G.case_id(c) for c in G.CASES] + [G.group_id(g) for g in G.GROUP_CASES]
    assert len(ids) == len(set(ids))


def test_planner_puts_an_engine_weight_gradient_on_tile_4():
    """Why tile 4's reduction matters: r3d_gemm_plan picks it for engine_rnn's input_embed.weight gradient (TN with
    bias_grad) at the default widths on 512-frame clips.  The planner asks for K-slabs there; ops.gemm drops them for a
    bias_grad product and keeps the tile.  (On short clips, e.g. 64 frames, the same product is planned onto tile 1.)"""
    from r3d_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()

    def plan(Kc, M, N):
        d = _lib.GemmDesc()
        d.layout, d.M, d.N, d.K = G.TN, M, N, Kc
        d.lda, d.ldb, d.ldc, d.alpha = M, N, N, 1.0
        d.bias_grad = 16                         # (never dereferenced by the planner: it only keeps the panel kernel out)
        assert lib.r3d_gemm_plan(C.byref(d)) == 0
        return int(d.tile)
    assert plan(**G.PLANNED_TILE4) == 4
    assert plan(8 * 64, 128, 2048) == 1
