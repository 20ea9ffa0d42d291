"""CPU-side checks of the data-set rank measurement: the --erank_report flag (default, help, the drop-in parser), the host
queries of the streaming-QR kernel, and the method itself -- the float32 numpy restatement of the append
(tests/rank_oracle.py) against float64 on the collapsed, clustered and N < H rows of tests/rank_cases.py, at the tolerances the
device kernel is held to.  No launches."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rank_cases as RC
from tests import rank_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from r3d_amd import build, ops
    build.build(verbose=False)
    return ops


def test_flag_default_and_help():
    from r3d_amd.opts import parser
    assert parser.parse_args([]).erank_report is False
    assert parser.parse_args(["--erank_report"]).erank_report is True
    act = next(a for a in parser._actions if "--erank_report" in a.option_strings)
    for word in ("effective rank", "RGB", "depth", "fused", "validat"):
        assert word in act.help, (word, act.help)
    # the flags it sits beside are as they were
    a = parser.parse_args([])
    assert a.erank_every == 0 and a.erank_weight == 0.0


def test_dropin_parser_has_the_flag_and_readme_mirrors_it(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    script = ("from opts import parser\nimport r3d_amd.opts as O\nassert parser is O.parser\n"
              "a = parser.parse_args(['--erank_report'])\nassert a.erank_report is True\n"
              "assert parser.parse_args([]).erank_report is False\nprint('ok')\n")
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    readme = open(os.path.join(ROOT, "dropin", "README.md")).read()
    assert "--erank_report" in readme and "Effective rank over" in readme


def test_host_queries(ops):
    for H in (1, 128, 2048):
        assert ops.qr_append_supported(H) is True
        T = ops.qr_append_tile_rows(H)
        assert T >= 1 and T * ((H + 3) // 4 * 4) * 4 <= 160 * 1024, (H, T)
    for H in (0, 2049, -3):
        assert ops.qr_append_supported(H) is False
        assert ops.qr_append_tile_rows(H) == 0
    assert 200 <= ops.qr_append_tile_rows(128) <= 320          # about 256 rows at H 128
    assert ops.qr_append_tile_rows(2048) >= 16
    # one more row would not fit beside the step's vectors: the tile is the largest that does
    assert ops.qr_append_tile_rows(128) > ops.qr_append_tile_rows(256) > ops.qr_append_tile_rows(1024)


def test_refusals_return_einval_without_a_device(ops):
    """The entry points validate before they touch a pointer or launch: H 0 / 2049, lanes 0 / 65, ldx < H."""
    from r3d_amd import _lib
    lib = _lib.load()
    R = 0x1000                                                   # never dereferenced: every call is refused on the host
    for H, lanes, ldx in ((0, 1, 8), (2049, 1, 2049), (128, 0, 128), (128, 65, 128), (128, 2, 127)):
        assert lib.r3d_qr_append(R, ldx, 4, H, None, 0, R, None, lanes, None) == -1, (H, lanes, ldx)
    assert lib.r3d_qr_append(R, 128, -1, 128, None, 0, R, None, 1, None) == -1
    assert lib.r3d_qr_append(R, 128, 4, 128, None, 0, None, None, 1, None) == -1
    for H, lanes in ((0, 2), (2049, 2), (128, 0), (128, 65)):
        assert lib.r3d_qr_merge(R, None, H, lanes, 1, None) == -1, (H, lanes)
    assert lib.r3d_qr_append(None, 128, 0, 128, None, 0, R, None, 4, None) == 0      # n = 0: a no-op, nothing is launched


CPU_CASES = [c for c in RC.CASES if c.cpu]


@pytest.mark.parametrize("tile", [256, 64])
@pytest.mark.parametrize("c", CPU_CASES, ids=RC.case_id)
def test_float32_householder_append_meets_the_tolerances(c, tile):
    assert {k.input for k in CPU_CASES} >= {"col", "clu"} and any(k.N < k.H for k in CPU_CASES if isinstance(k.N, int))
    x = RO.make_input(c.input, c.N, c.H, seed=c.N + 7 * c.H)
    R = RO.stream_f32(x, c.chunk, c.lanes, tile)
    worst, er_ref = RO.check_against_fp64(R, x, RC.case_id(c))
    er = RO.erank_of_sigma(RO.svdvals64(R))
    print(f"[rank f32 {RC.case_id(c)} tile {tile}] sigma err/max {worst:.2e}, erank {er:.6f} vs {er_ref:.6f}")
    assert abs(er - er_ref) <= RC.erank_tol(er_ref), (er, er_ref)


@pytest.mark.parametrize("c", [k for k in CPU_CASES if k.input == "col"], ids=RC.case_id)
def test_fp32_gram_loses_the_collapsed_case(c):
    """Why the accumulator is a QR and not X^T X: on the collapsed rows the float32 Gram route misses the project's bound,
    the float32 Householder append stays far inside it."""
    x = RO.make_input(c.input, c.N, c.H, seed=c.N + 7 * c.H).astype(np.float32)
    er_ref = RO.erank64(x)
    g = np.zeros((c.H, c.H), dtype=np.float32)
    for c0 in range(0, c.N, c.chunk):
        g += x[c0:c0 + c.chunk].T @ x[c0:c0 + c.chunk]
    ev = np.linalg.eigvalsh(g.astype(np.float64))
    er_gram = RO.erank_of_sigma(np.sqrt(np.clip(ev, 0, None)))
    er_qr = RO.erank_of_sigma(RO.svdvals64(RO.stream_f32(x, c.chunk, c.lanes, 256)))
    print(f"[rank gram vs qr {RC.case_id(c)}] fp64 {er_ref:.6f}, fp32 gram {er_gram:.6f}, fp32 householder {er_qr:.6f}")
    assert abs(er_gram - er_ref) > RC.erank_tol(er_ref)
    assert abs(er_qr - er_ref) < 1e-2 * RC.erank_tol(er_ref)
