"""Case table of the fp32 tiled GEMM kernels (csrc/gemm_f32.hip: gemm_f32_kernel, gemm_grouped_kernel,
splitk_reduce_kernel) for tests/test_gemm_f32_cpu.py and tests/test_gemm_f32_gpu.py.  No torch.cuda here: the table and
its helpers import on a machine without a GPU.

One `Case` is one launch (an "epi" case is the same launch repeated over act x mul, an "adam" case over two steps):

    kind    raw        plain product, C = A op B
            bias_grad  TN weight gradient with the fused column sums of A (r3d_gemm_desc::bias_grad)
            epi        the full epilogue of test_gemm_epilogue_and_prologue (EPI_FULL), looped over act and mul in 0..2
            xor        c_row_xor = 1 with res1 (test_gemm_c_row_xor_is_pair_swap)
            adam       the AdamW epilogue (r3d_gemm_desc::adam_*), tile 0 = the tile ops.gemm picks
    layout  0 NT a[M,K] b[N,K]; 1 NN a[M,K] b[K,N]; 2 TN a[K,M] b[K,N]
    tile    1..5 (launch_layout's cases); the bf16x3 tiles and the panel kernels are not in this table (tests/gemm_bf3_cases.py has 7 to 12)
    splitk  what is passed to ops.gemm; `nsplits` gives the number of slabs that makes
    pad     0 or 3: operand leading dimension = columns + pad (3: not a multiple of 4 -> the scalar-load twin)
    epi     frozenset of extra operand names on top of the kind: a_add, a_row_xor, b_add

`GroupCase` is one grouped launch: a layout, a tile and its problems (M, N, K, keywords), the keywords being names of
`GROUP_EPI` -- the keyword sets r3d_amd/engine.py puts in its groups (fwd_pairs: g1, g2, g3; bwd_vh1 / bwd_pairs)."""
from collections import namedtuple

Case = namedtuple("Case", "kind layout tile M N K splitk pad epi tag")
GroupCase = namedtuple("GroupCase", "layout tile problems tag")

NT, NN, TN = 0, 1, 2
LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN"}
TILE_SZ = {1: 32, 2: 64, 3: 128, 4: 64, 5: 128}       # BM = BN of launch_layout's cases
TILE_BK = {1: 64, 2: 64, 3: 32, 4: 64, 5: 32}
KSPLIT_WAVE_TILES = (4, 5)                            # WK = 2
EPI_FULL = frozenset({"bias", "pre_out", "drop", "aux", "res1", "res2", "alpha", "accumulate"})
ADD_MOD = 8                                           # rows of the broadcast addend of a_add / b_add


def cdiv(a, b):
    return (a + b - 1) // b


def nsplits(K, splitk):
    """Number of K-slabs ops.gemm makes of `splitk` for the fp32 tiles (a copy of its rounding: slabs are multiples of 16
    deep, and fewer than two slabs means no split)."""
    if splitk <= 1:
        return 1
    kps = cdiv(cdiv(K, splitk), 16) * 16
    ns = cdiv(K, kps)
    return ns if ns >= 2 else 1


def grid_mode(tile, M, N, nsplit):
    """(mode, G, NG) of a launch: the XCD placement rule of launch_cfg in csrc/gemm_f32.hip.  This is a COPY of that
    rule (the host code is not callable without a launch): the two are changed together.  mode 0 is the plain 2-D grid;
    otherwise NG groups of G workgroups, the grid padded to 8 * G * cdiv(NG, 8) workgroups."""
    tm, tn = cdiv(M, TILE_SZ[tile]), cdiv(N, TILE_SZ[tile])
    if nsplit > 1 and 1 < tm * tn <= 32:
        return 1, tm * tn, nsplit
    if nsplit == 1 and 2 <= tm <= 16 and tn >= 16:
        return 2, tm, tn
    if nsplit == 1 and 2 <= tn <= 16 and tm >= 16:
        return 3, tn, tm
    return 0, 1, 1


def tiles_of(c):
    return cdiv(c.M, TILE_SZ[c.tile]) * cdiv(c.N, TILE_SZ[c.tile])


def case_mode(c):
    return grid_mode(c.tile, c.M, c.N, nsplits(c.K, c.splitk))


def k_steps(c):
    """k-steps of one workgroup (of its longest slab)"""
    ns = nsplits(c.K, c.splitk)
    kps = c.K if ns == 1 else cdiv(cdiv(c.K, c.splitk), 16) * 16
    return cdiv(kps, TILE_BK[c.tile])


def case_id(c):
    e = "+".join(sorted(c.epi))
    return f"{c.tag}-{c.kind}-{LAYOUT_NAME[c.layout]}-t{c.tile}-{c.M}x{c.N}x{c.K}-sk{c.splitk}-p{c.pad}" + (f"-{e}" if e else "")


def _case(kind, layout, tile, shape, splitk=1, pad=0, epi=(), tag=""):
    M, N, K = shape
    return Case(kind, layout, tile, M, N, K, splitk, pad, frozenset(epi), tag)


# ----------------------------------------------------------------------------------------------------------
# a. the k-split-wave tiles 4 and 5: every layout, vector and scalar loads
# ----------------------------------------------------------------------------------------------------------
# tile 4 (BK 64): 1, 1, 2, 2, 4 (K % BK != 0) and 3 k-steps; tile 5 (BK 32): 2, 2, 3, 4, 7, 5 and 3 k-steps, 1 at K = 24
WK_SHAPES = {4: [(64, 64, 64), (50, 17, 33), (130, 260, 70), (64, 1, 128), (70, 96, 200), (70, 96, 136)],
             5: [(64, 64, 64), (50, 17, 33), (130, 260, 70), (64, 1, 128), (70, 96, 200), (70, 96, 136), (130, 132, 96),
                 (130, 132, 24)]}
WK_CASES = [_case("raw", L, t, s, 1, pad, tag="wk") for t in KSPLIT_WAVE_TILES for s in WK_SHAPES[t] for L in (NT, NN, TN)
            for pad in (0, 3)]
WK_CASES += [_case("raw", L, t, (70, 96, 200), 3, pad, tag="wk-splitk") for t in KSPLIT_WAVE_TILES for L in (NT, NN, TN)
             for pad in (0, 3)]

# ----------------------------------------------------------------------------------------------------------
# b. TN bias_grad on tiles 4 and 5 (M, N, K = the (Kc, M, N) of the issue reordered)
# ----------------------------------------------------------------------------------------------------------
# (70, 96, 200): two column tiles on tile 4 (only n0 == 0 writes); (130, 40, 33): three / two row tiles;
# (130, 132, 96): two row and two column tiles on tile 5 as well
BIAS_GRAD_SHAPES = [(70, 96, 200), (130, 40, 33), (130, 132, 96)]
BIAS_GRAD_CASES = [_case("bias_grad", TN, t, s, 1, pad, epi, tag="db") for t in KSPLIT_WAVE_TILES for s in BIAS_GRAD_SHAPES
                   for pad in (0, 3) for epi in ((), ("b_add",))]

# ----------------------------------------------------------------------------------------------------------
# c. the full epilogue on tiles 2..5 (gemm_epilogue_tile: two EpiOps<8> halves; split-K: splitk_reduce_kernel)
# ----------------------------------------------------------------------------------------------------------
EPI_SHAPES = [(96, 72, 64), (70, 100, 40)]
EPI_TILES = (2, 3, 4, 5)
EPI_CASES = [_case("epi", NT, t, s, sk, 0, ("a_add", "a_row_xor"), tag="epi") for t in EPI_TILES for s in EPI_SHAPES
             for sk in (1, 3)]
EPI_CASES += [_case("epi", NN, t, (70, 100, 40), sk, 0, ("a_add", "a_row_xor"), tag="epi") for t in EPI_TILES for sk in (1, 3)]
EPI_CASES += [_case("epi", TN, t, (70, 100, 40), 1, 0, (), tag="epi") for t in EPI_TILES]
EPI_CASES += [_case("epi", NT, t, (70, 100, 40), 1, 3, ("a_add", "a_row_xor"), tag="epi-scalar") for t in (2, 4)]
XOR_CASES = [_case("xor", NT, t, s, sk, 0, (), tag="xor") for t in EPI_TILES for s in EPI_SHAPES for sk in (1, 3)]

# ----------------------------------------------------------------------------------------------------------
# d. grid modes (launch_cfg): (tile, (M, N, K), splitk, what it reaches)
# ----------------------------------------------------------------------------------------------------------
GRID_ROWS = [
    (1, (40, 520, 24), 1, "mode 2: G = 2, NG = 17"),
    (1, (40, 512, 24), 1, "mode 2: G = 2, NG = 16 (no padding groups)"),
    (1, (500, 530, 24), 1, "mode 2: G = 16, NG = 17"),
    (2, (70, 1030, 40), 1, "mode 2: tile 2, G = 2, NG = 17"),
    (5, (130, 2050, 40), 1, "mode 2: tile 5, G = 2, NG = 17"),
    (1, (520, 40, 24), 1, "mode 3: G = 2, NG = 17"),
    (1, (512, 40, 24), 1, "mode 3: G = 2, NG = 16"),
    (1, (530, 500, 24), 1, "mode 3: G = 16, NG = 17"),
    (2, (1030, 70, 40), 1, "mode 3: tile 2, G = 2, NG = 17"),
    (1, (530, 530, 24), 1, "mode 0: tm = tn = 17, past both rules"),
    (1, (40, 480, 24), 1, "mode 0: tn = 15, below the mode-2 rule"),
    (1, (32, 520, 24), 1, "mode 0: tm = 1, below the mode-2 rule"),
    (1, (480, 40, 24), 1, "mode 0: tm = 15, below the mode-3 rule"),
    (1, (128, 256, 144), 9, "mode 1: 32 tiles, NG = 9"),
    (1, (128, 264, 144), 9, "mode 0: 36 tiles with split-K"),
    (1, (96, 352, 144), 9, "mode 0: 33 tiles with split-K, the first count past the mode-1 rule"),
    (4, (70, 96, 144), 9, "mode 1: tile 4, 4 tiles, NG = 9"),
]
GRID_CASES = [_case("raw", L, t, s, sk, 0, tag="grid") for (t, s, sk, _) in GRID_ROWS for L in (NT, NN, TN)]
GRID_CASES += [_case("raw", NT, 1, (40, 520, 24), 1, 3, tag="grid"), _case("raw", TN, 1, (520, 40, 24), 1, 3, tag="grid")]

# ----------------------------------------------------------------------------------------------------------
# e. the AdamW epilogue of the fp32 tiles (M, N, K = the (K, M, N) of the issue reordered); tile 0: ops.gemm's choice
# ----------------------------------------------------------------------------------------------------------
ADAM_SHAPES = [(70, 100, 64), (130, 132, 96), (64, 64, 40)]
ADAM_LDC_PAD = 8                                       # parameter and moments live in [M, N + 8] buffers
ADAM_CASES = [_case("adam", L, t, s, 1, 0, tag="adam") for t in (2, 3, 0) for s in ADAM_SHAPES for L in (TN, NT)]
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-3, grad_scale=0.25, alpha=0.5, lr=1e-3)

CASES = WK_CASES + BIAS_GRAD_CASES + EPI_CASES + XOR_CASES + GRID_CASES + ADAM_CASES

# ----------------------------------------------------------------------------------------------------------
# f. grouped launches
# ----------------------------------------------------------------------------------------------------------
# keyword sets of the engine's groups (r3d_amd/engine.py): name -> operand names the problem carries
GROUP_EPI = {
    "plain": frozenset(),
    "v_swap": frozenset({"c_row_xor"}),                             # fwd_pairs g1 / bwd_vh1: V of the other token
    "qkv_pos": frozenset({"a_add", "bias"}),                        # fwd_pairs g1, g3: (x + pos) W^T + b
    "mlp_gelu": frozenset({"bias", "act2", "pre_out"}),             # fwd_pairs g2: mlp.0 with its GELU, pre-activation kept
    "proj_drop": frozenset({"bias", "drop"}),                       # fwd_pairs g2: out_proj with its dropout
    "head": frozenset({"bias"}),                                    # fwd_pairs g3: fc_seg
    "gelu_bwd": frozenset({"aux", "mul2"}),                         # bwd_pairs: d_u = (d_x3 W2) * gelu'(u)
}


def _ragged(n):
    """the ragged problems of test_gemm_grouped_problem_lookup"""
    return tuple((20 + 13 * (i % 5), 30 + 17 * (i % 4), 24 + 8 * (i % 3), "plain") for i in range(n))


GROUP_CASES = [
    GroupCase(NN, 1, _ragged(7), "ragged"),
    GroupCase(NN, 2, _ragged(7), "ragged"),
    GroupCase(NT, 2, _ragged(7), "ragged"),
    GroupCase(NN, 1, _ragged(35), "ragged-search"),                  # more than 32 problems: the prefix search in memory
] + [
    # the engine's forward groups (NT) and backward groups (NN), rows even for the pair swap, ragged against both tiles
    GroupCase(NT, t, ((70, 40, 40, "v_swap"), (24, 100, 40, "qkv_pos"), (70, 136, 40, "mlp_gelu"), (24, 40, 40, "proj_drop"),
                      (35, 9, 40, "head")), "engine-fwd") for t in (1, 2)
] + [
    GroupCase(NN, t, ((70, 40, 40, "v_swap"), (70, 40, 40, "v_swap"), (24, 100, 120, "plain"), (70, 136, 40, "gelu_bwd")),
              "engine-bwd") for t in (1, 2)
]


def group_id(g):
    return f"{g.tag}-{LAYOUT_NAME[g.layout]}-t{g.tile}-n{len(g.problems)}"


# A TN bias_grad product of an engine at its defaults that r3d_gemm_plan puts on tile 4: input_embed.weight's gradient
# in engine_rnn (hidden 128, input_dim 2048, batch 8) on 512-frame clips: dY [4096, 128]^T . X [4096, 2048].
PLANNED_TILE4 = dict(Kc=8 * 512, M=128, N=2048)
