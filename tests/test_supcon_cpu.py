"""Host-side checks of the supervised contrastive loss: the float64 restatement (tests/supcon_oracle.py) against the
fixtures recorded from the imported reference (tests/golden/supcon_cases.npz, a float32 run: 1e-5 relative for the loss,
1e-4 of the gradient's scale), the ignore cases against the reference on the kept rows, finiteness where the reference is
nan; the drop-in import; the module's refusals (none of them touches a GPU); the --supcon_weight flag."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import supcon_cases as SC, supcon_oracle as SO
from tests.helpers import stats
from tests.test_engine_gpu import close_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "supcon_cases.npz"), allow_pickle=False)
    fx = {k: z[k] for k in z.files}
    fx["meta"] = json.loads(str(fx["meta"]))
    return fx


def restated(case):
    x, y = SC.make(case)
    loss, g, lse, P = SO.supcon_with_grad(SO.contrast_rows(x), SC.oracle_labels(case, y), **SC.oracle_kwargs(case))
    return x, y, loss, torch.stack(g.split(case["bsz"]), 1)


@pytest.mark.parametrize("name", [c["name"] for c in SC.CASES])
def test_restatement_equals_the_reference_fixture(golden, name):
    case = SC.BY_NAME[name]
    kind = golden["meta"][name]
    x, y, loss, grad = restated(case)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    if kind == "no_reference":                                   # every row ignored: there is nothing to run the reference on
        assert float(loss) == 0.0 and not bool(grad.any())
        return
    want = float(golden[f"loss_{name}"])
    if kind == "nan":                                            # the reference's nan: the restatement is finite (above)
        assert np.isnan(want)
        return
    assert abs(float(loss) - want) <= 1e-5 * max(abs(want), 1e-5), (float(loss), want)
    if kind == "full":
        close_rel(grad, torch.from_numpy(golden[f"grad_{name}"]), f"{name} gradient", rtol=1e-4)
        if case["ignore"]:                                       # an ignored row has no gradient
            assert not bool(grad[y == SC.IGNORE].any())
    else:
        got, ref = stats(grad), golden[f"gstat_{name}"]
        assert np.abs(got[:3] - ref[:3]).max() <= 1e-4 * ref[2]          # norm, sum, abs-sum: on the abs-sum's scale
        assert np.abs(got[3:] - ref[3:]).max() <= 1e-4 * float(grad.abs().max())


def test_nan_cases_are_the_ones_the_issue_names(golden):
    nan = sorted(k for k, v in golden["meta"].items() if v == "nan")
    assert nan == ["n1_d16", "raw_03_randn"]


def test_ignored_rows_equal_the_loss_of_the_kept_rows():
    case = SC.BY_NAME["ign_scattered"]
    x, y = SC.make(case)
    kept = y != SC.IGNORE
    assert 40 < int((~kept).sum()) < 90
    full, _, _ = SO.supcon(x[:, 0], y, ignore_index=SC.IGNORE)
    sub, _, _ = SO.supcon(x[kept][:, 0], y[kept])
    assert abs(float(full) - float(sub)) <= 1e-12 * abs(float(sub))


DROPIN = r'''
from loss.spc import SupConLoss                                      # main_nturgbd.py:15
import r3d_amd.loss.spc as R
assert SupConLoss is R.SupConLoss
c = SupConLoss(temperature=0.1)
assert (c.temperature, c.contrast_mode, c.base_temperature, c.ignore_index, c.normalize) == (0.1, 'all', 0.07, None, False)
print("ok")
'''


def test_reference_import_line_resolves_through_dropin(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", DROPIN], env=env, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]


@pytest.fixture(scope="module")
def SupConLoss():
    from r3d_amd import build
    build.build(verbose=False)                                   # (the width limit is the library's own host-only check)
    from r3d_amd.loss import SupConLoss as S
    return S


def test_module_refusals_are_host_only(SupConLoss):
    f, y = torch.randn(6, 1, 8), torch.arange(6)
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        SupConLoss()(f[:, 0], y)
    with pytest.raises(ValueError, match="both `labels` and `mask`"):
        SupConLoss()(f, y, torch.eye(6))
    with pytest.raises(ValueError, match="does not match"):
        SupConLoss()(f, y[:5])
    with pytest.raises(ValueError, match="Unknown mode"):
        SupConLoss(contrast_mode="some")(f, y)
    with pytest.raises(NotImplementedError, match="mask"):
        SupConLoss()(f, mask=torch.eye(6))
    with pytest.raises(ValueError, match="256"):
        SupConLoss()(torch.randn(6, 1, 257), y)
    with pytest.raises(ValueError, match="256"):
        SupConLoss()(torch.randn(6, 1, 3, 100), y)              # more than 3 dimensions are flattened: 300 wide
    with pytest.raises(TypeError, match="no torch fallback"):
        SupConLoss()(f, y)                                       # a CPU tensor


def test_width_limit_is_the_librarys(SupConLoss):
    from r3d_amd import ops
    from r3d_amd.engine_rnn import RNN_MAX_H
    assert [ops.supcon_supported(d) for d in (0, 1, 256, 257)] == [False, True, True, False]
    assert RNN_MAX_H == 256
    assert ops.supcon_ws_floats(9136) * 4 < 160 * 1024           # the workspace of the README's DARai shape: 4 N + 4 floats


def test_supcon_weight_parses_and_the_other_loops_refuse_it():
    from r3d_amd import opts, train_proposed_depth, train_tcn
    assert opts.parser.parse_args([]).supcon_weight == 0.0
    assert opts.parser.parse_args(["--supcon_weight", "0.5"]).supcon_weight == 0.5
    args = argparse.Namespace(supcon_weight=0.5)
    with pytest.raises(ValueError, match="supcon_weight"):
        train_proposed_depth.train(args, *[None] * 10)
    with pytest.raises(ValueError, match="supcon_weight"):
        train_tcn.train(args, *[None] * 9)
