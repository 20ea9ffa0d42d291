"""The tall rank route on the host: the numpy restatement (tests/erank_tall_oracle.py) against float64 autograd through
svdvals, how far its float32 form lands (the yardstick of the GPU tolerances), the admission of both routes, the fold
rule against its measurement, and the parser's default."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import futr_oracle as O
from tests import erank_tall_cases as TC
from tests import erank_tall_oracle as TO
from tests.test_erank_shapes_gpu import make_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def erank64(x):
    xr = torch.from_numpy(np.asarray(x, dtype=np.float64)).clone().requires_grad_(True)
    er = O.effective_rank_torch(xr)
    er.backward()
    return float(er.detach()), xr.grad.numpy()


@pytest.mark.parametrize("kind", TC.SPECTRA)
@pytest.mark.parametrize("N,H,lanes", [(74, 64, 1), (128, 128, 3), (600, 128, 8), (320, 128, 5)])
def test_oracle_against_fp64_autograd(N, H, lanes, kind):
    x = make_matrix(N, H, kind, seed=N + 7 * H).float().numpy()
    er_ref, g_ref = erank64(x)
    er, dx, s = TO.route(x, lanes, np.float64)
    sv = np.linalg.svd(x.astype(np.float64), compute_uv=False)
    assert np.abs(np.sort(s)[::-1] - sv).max() <= 1e-12 * sv[0]
    assert abs(er - er_ref) <= 1e-9 * er_ref
    assert TO.grad_err(dx, g_ref) <= 1e-7, TO.grad_err(dx, g_ref)
    # the same route in float32: the working precision's own distance from the reference
    er32, dx32, _ = TO.route(x, lanes, np.float32)
    e32 = TO.grad_err(dx32, g_ref)
    print(f"[tall oracle {N}x{H} {kind} lanes {lanes}] fp32 restatement: gradient err/scale {e32:.2e}, |d erank| {abs(er32 - er_ref):.1e}")
    assert e32 <= TC.GRAD_TOL_KERNEL / 3 and abs(er32 - er_ref) < 1e-6 * max(1.0, er_ref)


def test_oracle_fold_and_merge_keep_the_gram_matrix():
    x = TC.fold_input(333, 48, seed=3, kind="zeros").astype(np.float64)
    for lanes in (1, 3, 8, 64):
        R = TO.merge(TO.fold(x, lanes))
        assert np.array_equal(np.tril(R, -1), np.zeros_like(R))
        assert np.abs(R.T @ R - x.T @ x).max() <= 1e-12 * np.abs(x.T @ x).max()
    R = TO.fold(x[:5], 8)                       # lanes without rows stay zero, short lanes are zero-padded
    assert not R[5:].any() and not R[0, 1:].any()


def test_admission_of_both_routes():
    from r3d_amd import build
    from r3d_amd.engine import check_erank_shape
    build.build(verbose=False)
    check_erank_shape(8, 1200, 128, route="tall")
    check_erank_shape(16, 1142, 128, route="tall")
    check_erank_shape(1, 64, 64, route="tall")
    check_erank_shape(4, 80, 128, route="tall")
    check_erank_shape(4, 80, 128)
    with pytest.raises(ValueError, match="N >= H"):
        check_erank_shape(1, 63, 64, route="tall")
    with pytest.raises(ValueError, match="2048"):
        check_erank_shape(2, 4096, 2064, route="tall")
    with pytest.raises(ValueError, match=r"2\^31"):
        check_erank_shape(1024, 2048, 1024, route="tall")
    check_erank_shape(1023, 2048, 1024, route="tall")
    with pytest.raises(ValueError, match="erank_route"):
        check_erank_shape(4, 80, 128, route="gram")
    # the default route refuses what it refused, and says where the shape is admitted
    for args in ((1, 9597, 128), (8, 1200, 128)):
        with pytest.raises(ValueError, match=r"rank penalty.*past its 150 KiB \(--erank_route tall admits it\)"):
            check_erank_shape(*args)
        with pytest.raises(ValueError):
            check_erank_shape(*args, route="jacobi")
    check_erank_shape(1, 9596, 128)


def test_effective_rank_tall_refuses_on_the_host():
    from r3d_amd.erank import effective_rank, ErankTall
    with pytest.raises(ValueError, match="N >= H"):
        effective_rank(torch.zeros(63, 64), route="tall")
    with pytest.raises(ValueError, match="2048"):
        effective_rank(torch.zeros(4096, 2064), route="tall")
    with pytest.raises(ValueError, match="fold"):
        ErankTall(128, 64, "cpu", fold="gram")


def test_fold_kernel_admission_and_fold_pays_on_the_host():
    from r3d_amd import build, ops
    from r3d_amd import erank
    build.build(verbose=False)
    wide = [H for H in range(0, 2100) if ops.qr_fold_wy_supported(H)]
    assert set(range(16, 513, 16)) <= set(wide) and all(H % 16 == 0 for H in wide)
    for H in range(0, 2100, 8):
        T = ops.qr_fold_wy_tile_rows(H)
        assert (T > 0) == (H in wide) and T % 16 == 0
        if T:       # the launch's dynamic LDS: tile + VQ + VP rows, 16 rows of R, part, S, T, the waves' scratch, tau, fs
            ld = H if H % 32 == 16 else H + 16
            fixed = 16 * ld + 2 * 32 * 16 + 2 * 16 * 20 + 8 * 16 * 20 + 2 * 16
            assert 4 * (T * (ld + 16 + 18) + fixed) <= 160 * 1024 - 256
            assert T == 512 or 4 * ((T + 16) * (ld + 16 + 18) + fixed) > 160 * 1024 - 256      # and the largest that does
    # the rule is the measurement's: every shape of profiles/erank_tall_speed.json takes the fold that was faster there
    prof = json.load(open(os.path.join(ROOT, "profiles", "erank_tall_speed.json")))
    rows = prof["fold"]
    assert {(r["n"], r["H"]) for r in rows} == {(9600, 128), (18272, 128), (4096, 256), (4096, 512)}
    for r in rows:
        want = "wy" if r["wy_ms"] < r["column_ms"] else "column"
        assert erank.fold_pays(r["n"], r["H"]) == want == r["fold_pays"], r
    # shapes nobody timed and widths the kernel refuses take the column fold; no launch, no device
    for N, H in [(9600, 100), (9600, 1024), (100000, 2048), (64, 64), (9600, 96)]:
        assert erank.fold_pays(N, H) == "column", (N, H)
    assert all(erank.fold_pays(N, H) in erank.FOLDS for N in (128, 5000, 20000) for H in (64, 128, 256, 512))


def test_parser_default_is_the_jacobi_route():
    from r3d_amd.opts import parser
    assert parser.parse_args([]).erank_route == "jacobi"
    assert parser.parse_args(["--erank_route", "tall"]).erank_route == "tall"
    with pytest.raises(SystemExit):
        parser.parse_args(["--erank_route", "gram"])


def test_multi_gpu_wrappers_refuse_the_tall_route():
    from r3d_amd.parallel import refuse_tall_route

    class E:
        erank_route = "tall"
    with pytest.raises(ValueError, match="one GPU"):
        refuse_tall_route(E(), "a data-parallel step")
    E.erank_route = "jacobi"
    refuse_tall_route(E(), "a data-parallel step")
