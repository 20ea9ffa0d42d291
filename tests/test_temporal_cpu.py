"""Host-side checks of the temporal auxiliary losses: the float64 restatement (tests/temporal_oracle.py) against the fixtures
recorded from the imported reference on .double() inputs (tests/golden/temporal_cases.npz: 1e-9 relative for the loss, the
float32 rounding the gradients are stored with for the gradients); the loop form against the restatement;
runs_from_intervals; the ValueErrors of every limit (none of them touches a GPU); the drop-in import."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import temporal_cases as TC, temporal_oracle as TO
from tests.helpers import stats
from tests.test_engine_gpu import close_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "temporal_cases.npz"), allow_pickle=False)
    fx = {k: z[k] for k in z.files}
    fx["meta"] = json.loads(str(fx["meta"]))
    return fx


def fixture_intervals(golden, name):
    B = TC.BY_NAME[name]["B"]
    out = [[] for _ in range(B)]
    for b, s, e in golden[f"iv_{name}"].tolist():
        out[b].append((s, e))
    return out


def restated(case):
    """(loss, gradient) of the float64 restatement"""
    if case["kind"] == "focal":
        pred, gold = TC.make(case)
        return TO.with_grad(lambda p: TO.focal(p, gold, case["pad"], case["exclude"], case["alpha"], case["gamma"],
                                               case["penalty"])[0], pred)
    x, iv = TC.make(case)
    if case["kind"] == "cluster":
        return TO.with_grad(TO.cluster, x, iv)
    return TO.with_grad(TO.contrastive, x, iv, case["temperature"])


@pytest.mark.parametrize("name", [c["name"] for c in TC.CASES])
def test_restatement_equals_the_reference_fixture(golden, name):
    case = TC.BY_NAME[name]
    loss, grad = restated(case)
    want = float(golden[f"loss_{name}"])
    assert abs(float(loss) - want) <= 1e-9 * abs(want) + 1e-11, (float(loss), want)
    if golden["meta"][name] == "full":
        close_rel(grad, torch.from_numpy(golden[f"grad_{name}"]), f"{name} gradient", rtol=2e-7)     # (stored as float32)
    else:
        got, ref = stats(grad), golden[f"gstat_{name}"]
        assert np.abs(got[:3] - ref[:3]).max() <= 1e-9 * ref[2]
        assert np.abs(got[3:] - ref[3:]).max() <= 1e-9 * float(grad.abs().max())
    if case["kind"] == "focal":
        pred, gold = TC.make(case)
        _, flags, n_correct, n_word = TO.focal(pred, gold, case["pad"], case["exclude"])
        assert np.array_equal(flags.numpy(), golden[f"flags_{name}"])
        assert [n_correct, n_word] == golden[f"counts_{name}"].tolist()
    else:
        x, iv = TC.make(case)
        assert fixture_intervals(golden, name) == iv == TO.intervals(TC.labels_of(iv, case["T"]))


def test_case_table_covers_what_it_claims():
    e = TC.structure("e", 63)
    assert e[:2] == [(0, 1), (2, 6)]
    m = TO.positive_mask(e, 63)
    assert not bool(m[4, 2]) and bool(m[4, 4]) and bool(m[2, 2]) and not bool(m[0, 0]) and not bool(m[1, 1])
    d = TC.structure("d", 65)
    assert (3, 3) in d and TO.positive_mask(d, 65)[3].nonzero().flatten().tolist() == [3]      # only the self pair
    c = TC.structure("c", 200)
    assert c == [(0, 63), (64, 64), (65, 199)]
    g = [TC.structure(p, 65) for p in TC.BY_NAME["c_t65_c48_g"]["patterns"]]
    assert len(g[-1]) == 1 and len(g[-2]) > 1
    assert all(len(TC.structure(p, 64)) == 1 for p in TC.BY_NAME["c_t64_c5_h"]["patterns"])
    zero = TC.BY_NAME["c_t8_c5_zero"]
    x, iv = TC.make(zero)
    loss, grad = TO.with_grad(TO.cluster, x, iv)
    assert len(iv[0]) == 3 and abs(float(loss) - 3 * 1e5 / 2) < 1e-6 and not bool(grad.any())


@pytest.mark.parametrize("name", ["n_t65_d16_g", "c_t65_c48_g", "c_t64_c5_h", "f_n65_c122"])
def test_loop_form_equals_the_restatement(name):
    case = TC.BY_NAME[name]
    loss, _ = restated(case)
    if case["kind"] == "focal":
        pred, gold = TC.make(case)
        gold = torch.where((gold < 0) | (gold >= case["C"]), torch.tensor(case["pad"]), gold)
        got, _ = TO.loop_focal(pred.double(), gold, case["pad"], case["exclude"], case["alpha"], case["gamma"], case["penalty"])
    else:
        x, iv = TC.make(case)
        assert TO.loop_intervals(TC.labels_of(iv, case["T"])) == iv
        fn = TO.loop_cluster if case["kind"] == "cluster" else TO.loop_contrastive
        got = fn(x.double(), iv)
    assert abs(float(got) - float(loss)) <= 1e-9 * abs(float(loss))


# ---------------------------------------------------------------------------------------------------------------------
# the public module: host-only checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def TL():
    from r3d_amd import build
    build.build(verbose=False)                                   # (the width limit is the library's own host-only check)
    from r3d_amd.loss import temporal
    return temporal


def test_runs_from_intervals_accepts_the_reference_lists(TL, golden):
    for name in ("n_t200_d48_f", "c_t65_c48_g", "n_t130_d20_r"):
        iv, T = fixture_intervals(golden, name), TC.BY_NAME[name]["T"]
        r = TL.runs_from_intervals(iv, T, "cpu")
        first, last, count = TO.frame_runs(iv, T)
        assert torch.equal(r.first.long(), first) and torch.equal(r.last.long(), last) and torch.equal(r.count.long(), count)
        assert r.first.dtype == r.last.dtype == r.starts.dtype == r.count.dtype == torch.int32
        assert r.intervals() == iv
        for b, clip in enumerate(iv):
            assert r.starts[b].tolist() == [s for s, _ in clip] + [T] * (T - len(clip))


@pytest.mark.parametrize("iv,T", [
    ([[(0, 2), (4, 7)]], 8),                    # a gap
    ([[(0, 4), (4, 7)]], 8),                    # an overlap
    ([[(4, 7), (0, 3)]], 8),                    # wrong order
    ([[(0, 3), (4, 7)]], 9),                    # wrong T: too short
    ([[(0, 3), (4, 8)]], 8),                    # wrong T: too long
    ([[(1, 7)]], 8),                            # does not start at 0
    ([[(0, 7)], []], 8),                        # a clip without intervals
    ([], 8),
])
def test_runs_from_intervals_refuses_what_is_no_partition(TL, iv, T):
    with pytest.raises(ValueError):
        TL.runs_from_intervals(iv, T, "cpu")


def test_shape_limits_raise_value_errors_on_the_host(TL):
    from r3d_amd import ops
    assert [ops.temporal_width_supported(w) for w in (0, 1, 256, 257)] == [False, True, True, False]
    lab = torch.zeros(2, 8, dtype=torch.int64)
    for fn in (TL.temporal_cluster_loss, TL.temporal_contrastive_loss):
        with pytest.raises(ValueError, match="256"):
            fn(torch.randn(2, 8, 257), lab)
        with pytest.raises(ValueError, match="T >= 1"):
            fn(torch.randn(2, 0, 4), torch.zeros(2, 0, dtype=torch.int64))
        with pytest.raises(ValueError, match=r"\[B, T, C\]"):
            fn(torch.randn(8, 4), lab)
        with pytest.raises(ValueError, match="do not match"):
            fn(torch.randn(2, 8, 4), lab[:, :7])                 # label shape mismatch
        with pytest.raises(TypeError, match="no torch fallback"):
            fn(torch.randn(2, 8, 4), lab)                        # a CPU tensor
    for tau in (0.0, -0.07, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            TL.temporal_contrastive_loss(torch.randn(2, 8, 4), lab, temperature=tau)
    pred, gold = torch.randn(5, 6), torch.zeros(5, dtype=torch.int64)
    for gamma in (0.5, 0.0, -1.0):
        with pytest.raises(ValueError, match="gamma"):
            TL.focal_loss(pred, gold, 5, gamma=gamma)
    with pytest.raises(ValueError, match="does not match"):
        TL.focal_loss(pred, gold[:4], 5)
    with pytest.raises(ValueError, match=r"\[N, C\]"):
        TL.focal_loss(pred[0], gold, 5)
    with pytest.raises(TypeError, match="no torch fallback"):
        TL.focal_loss(pred, gold, 5)
    with pytest.raises(ValueError, match="integer"):
        TL.label_runs(torch.zeros(2, 8))
    with pytest.raises(ValueError, match="interval lists"):
        TL._as_runs([[(0, 7)]], 2, 8, "cpu")
    with pytest.raises(ValueError, match="the runs describe"):
        TL._as_runs(TL.runs_from_intervals([[(0, 7)]], 8, "cpu"), 2, 8, "cpu")
    assert ops.tcontrast_ws_floats(8, 1142) == 5 * 8 * 1142 and ops.tcluster_ws_floats(8, 1142, 257) == 0


DROPIN = r'''
from utils import cal_performance_focal, temporal_cluster_loss, temporal_contrastive_loss, focal_loss, normalize_duration
import r3d_amd.loss.temporal as R
assert temporal_cluster_loss is R.temporal_cluster_loss and temporal_contrastive_loss is R.temporal_contrastive_loss
assert focal_loss is R.focal_loss and cal_performance_focal is R.cal_performance_focal
import inspect
assert list(inspect.signature(focal_loss).parameters) == ["pred", "gold", "trg_pad_idx", "exclude_class_idx", "alpha", "gamma",
                                                           "penalty_weight"]
assert list(inspect.signature(cal_performance_focal).parameters) == ["pred", "gold", "trg_pad_idx", "exclude_class_idx",
                                                                      "smoothing", "reference", "target_ref"]
assert list(inspect.signature(temporal_contrastive_loss).parameters) == ["predictions", "cluster_intervals", "temperature"]
print("ok")
'''


def test_reference_import_line_resolves_through_dropin(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", DROPIN], env=env, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]
