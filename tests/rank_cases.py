"""The streaming QR (r3d_qr_append / r3d_qr_merge, r3d_amd/rankstream.StreamingRank) over the shapes it admits.
tests/test_rank_stream_gpu.py runs every row on the device against float64; tests/test_rank_stream_cpu.py runs the float32
numpy restatement of the append (tests/rank_oracle.py) over the rows marked cpu, which pins the method independently of
the kernel.

Columns:
  N, H    -- the matrix; N may be "T-1", "T", "T+1": T = ops.qr_append_tile_rows(H), resolved where the library is loaded;
  chunk   -- rows per update() call (None: the whole matrix in one call);
  lanes   -- independent accumulators (merged by finalize());
  input   -- "gauss": standard normal; "sep": singular values linspace(0.2, 2.0) prescribed through QR; "clu": clusters of four
             singular values 0.1 % apart, sigma_max / sigma_min = 1e4 (as tests/erank_cases.py); "col": one dominant direction
             and a gaussian tail at 1e-4 of it (the collapsed representation an fp32 Gram accumulation loses); "relu": ReLU of
             a gaussian shifted by 0.5;
  ldx     -- None (contiguous) or the row stride of the wider matrix the rows are a column slice of;
  cpu     -- the row is also run through the float32 numpy restatement."""
import collections

Case = collections.namedtuple("Case", "N H chunk lanes input ldx cpu why")


def _c(N, H, chunk, lanes, input="gauss", ldx=None, cpu=False, why=""):
    return Case(N, H, chunk, lanes, input, ldx, cpu, why)


CASES = [
    _c(1, 8, 1, 1, why="a single row"),
    _c(37, 8, 5, 1, why="smallest H, ragged chunks"),
    _c("T-1", 128, None, 1, "sep", why="one row short of a tile"),
    _c("T", 128, None, 1, "sep", why="exactly one tile"),
    _c("T+1", 128, None, 1, "sep", why="a second tile of one row"),
    _c(700, 128, 96, 3, "clu", cpu=True, why="odd lane count through the merge tree, 1e4-conditioned clusters"),
    _c(3000, 128, 256, 4, "col", cpu=True, why="the collapsed case the fp32 Gram route misses"),
    _c(1500, 256, 96, 8, "col", cpu=True, why="collapsed at H 256"),
    _c(40, 200, 16, 2, cpu=True, why="N < H, H % 8 only, surplus sigma"),
    _c(600, 136, 77, 1, "relu", why="off the 64-column grid"),
    _c(900, 512, 130, 2, why="H 512: one row group of 512 threads, seven calls of 65 rows per lane"),
    _c(400, 512, 200, 1, why="more than one tile per call: 200 rows walk three tiles of 77"),
    _c(100, 1024, 33, 1, why="H 1024: the widest single-column-per-thread layout"),
    _c(40, 2048, 40, 2, why="the widest admitted, smallest tile"),
    _c(300, 70, 64, 2, ldx=130, why="a column slice of a wider matrix"),
]

# the project's existing tolerances (tests/test_erank_shapes_gpu.py)
SIGMA_RTOL = 1e-4
SIGMA_ATOL_REL = 1e-4           # x sigma_max
SURPLUS_REL = 1e-5              # surplus singular values when N < H, x sigma_max


def erank_tol(er):
    return 5e-3 * max(1.0, er / 50)


def case_id(c):
    return f"{c.N}x{c.H}-{c.input}-chunk{c.chunk}-lanes{c.lanes}" + (f"-ld{c.ldx}" if c.ldx else "")


def resolve_n(c, tile_rows):
    """The row count of a case (tile_rows: ops.qr_append_tile_rows(c.H))."""
    if isinstance(c.N, int):
        return c.N
    return tile_rows + {"T-1": -1, "T": 0, "T+1": 1}[c.N]
