"""The TCN baseline without a GPU: the float64 restatement against the fixtures generated from the imported reference, the
model's state_dict keys / shapes / seeded init against the recorded ones, the drop-in imports, and check_tcn_shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import synth
from tests import tcn_cases as TC
from tests import tcn_oracle as TO
from tests.helpers import load_fixture, fixture_params, assert_close, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = [c[0] for c in TC.STEP_CASES]


def _batch(m):
    b = synth.make_batch(m["B"], m["S"], m["n_class"], m["pad_idx"], m["seed"], depth_hw=(2, 2))
    return torch.from_numpy(b[0]), torch.from_numpy(b[4])


def test_cases_cover_what_the_model_has():
    assert set(TO.CONVS) <= set(TC.CONV_KINDS)
    assert {(c[1], c[2], c[3]) for c in TC.STEP_CASES} == {(2, 5, 17), (8, 16, 122), (13, 37, 17), (4, 200, 49)}
    assert len(TC.CONV_CASES) == len(TC.CONV_KINDS) * len(TC.CONV_B) * len(TC.CONV_S)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference_fixture(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    feats, tgt = _batch(m)
    assert int((tgt == m["pad_idx"]).sum()) > 0, "the all-rows mean needs padded rows"
    tr = TO.Trainer(fixture_params(fx), m["pad_idx"], lr=m["lr"], wd=m["wd"])
    with torch.no_grad():
        ev = TO.forward(tr.p, feats.double())
    sc = lambda a: 1e-5 * max(1.0, float(np.abs(a).max()))       # noqa: E731
    assert_close(ev, fx["eval_out"], rtol=1e-4, atol=sc(fx["eval_out"]), what="eval")
    loss, nc, nt, out = tr.step(feats, tgt)
    assert_close(out, fx["out"], rtol=1e-4, atol=sc(fx["out"]), what="out")
    assert abs(float(loss) - float(fx["loss"])) <= 1e-5 * max(1.0, float(fx["loss"]))
    assert [nc, nt] == fx["counts"].tolist()
    for j, n in enumerate(fx["param_names"]):
        gs, want = stats(tr.p[n].grad), fx["grad_stats"][j]
        assert abs(gs[0] - want[0]) <= 1e-4 * max(1e-3, float(want[0])), (n, gs[0], want[0])
        if "grad::" + n in fx:
            full = fx["grad::" + n]
            assert_close(tr.p[n].grad, full, rtol=1e-3, atol=1e-4 * max(1e-3, float(np.abs(full).max())), what=n)
        ps, want = stats(tr.p[n]), fx["post_stats"][j]
        assert abs(ps[0] - want[0]) <= 1e-4 * max(1.0, float(want[0])), (n, ps[0], want[0])


def test_loss_is_the_mean_over_all_rows():
    g = torch.Generator().manual_seed(2)
    out = torch.randn(2, 8, 5, generator=g, dtype=torch.float64)
    tgt = torch.randint(0, 4, (2, 8), generator=g)
    tgt[0, 5:] = 4
    tgt[1, 7] = 4
    out[0, 0, 4] = 9.0                                         # a live row whose arg-max is pad_idx: + 2.0
    loss, nc, nt = TO.loss_counts(out, tgt, 4)
    live = tgt.reshape(-1) != 4
    ce = torch.nn.functional.cross_entropy(out.reshape(-1, 5)[live], tgt.reshape(-1)[live], reduction="sum")
    n_pen = int(((out.reshape(-1, 5).argmax(dim=1) == 4) & live).sum())
    assert n_pen >= 1 and abs(float(loss) - (float(ce) + 2.0 * n_pen) / 16) < 1e-12 and nt == 12


def test_conv_products_match_conv1d_autograd():
    g = torch.Generator().manual_seed(4)
    B, S, ci, co, d = 2, 11, 6, 5, 4
    x = torch.randn(B, S, ci, generator=g, dtype=torch.float64, requires_grad=True)
    v = torch.randn(co, ci, 3, generator=g, dtype=torch.float64, requires_grad=True)
    dz = torch.randn(B, S, co, generator=g, dtype=torch.float64)
    y = torch.nn.functional.conv1d(x.permute(0, 2, 1), v, padding=2 * d, dilation=d)[:, :, :-2 * d].permute(0, 2, 1)
    y.backward(dz)
    p, dx, gv = TO.conv_products(x, v, dz, d)
    assert torch.allclose(p, y.detach(), atol=1e-12) and torch.allclose(dx, x.grad, atol=1e-12)
    assert torch.allclose(gv, v.grad, atol=1e-12)


@pytest.mark.parametrize("tag", TAGS)
def test_model_keys_shapes_and_seeded_init_match_reference(tag):
    from r3d_amd.model.tcn import MustafaNet1DTCN
    fx = load_fixture(tag)
    torch.manual_seed(1)
    model = MustafaNet1DTCN(num_classes=fx["meta"]["num_classes"], anticipated_frames=8)
    sd = model.state_dict()
    assert list(sd.keys()) == json.loads(str(fx["state_keys"])) and len(sd) == 56
    assert [list(v.shape) for v in sd.values()] == json.loads(str(fx["state_shapes"]))
    named = list(model.named_parameters())
    assert [n for n, _ in named] == fx["param_names"] and len(named) == 32
    assert [list(p.shape) for _, p in named] == fx["param_shapes"]
    sums = np.array([[float(p.detach().double().sum()), float((p.detach().double() ** 2).sum())] for _, p in named])
    np.testing.assert_allclose(sums, fx["init_sums"], rtol=1e-9, atol=1e-12)
    assert [(n, tuple(s)) for n, s in zip(fx["param_names"], fx["param_shapes"])] == TO.names_shapes(fx["meta"]["num_classes"])
    assert model.load_state_dict({k: torch.zeros(s) for k, s in zip(sd.keys(), json.loads(str(fx["state_shapes"])))},
                                 strict=True).missing_keys == []
    assert sd["tcn_local.network.0.net.0.weight_v"].data_ptr() == sd["tcn_local.network.0.conv1.weight_v"].data_ptr()


def test_model_refuses_the_cpu():
    from r3d_amd.model.tcn import MustafaNet1DTCN
    with pytest.raises(RuntimeError, match="MI355X"):
        MustafaNet1DTCN(17)(torch.zeros(1, 4, 2048))


def test_train_loop_fixture_records_the_eval_mode_second_epoch():
    fx = load_fixture(TC.TRAIN_LOOP["tag"])
    out = json.loads(str(fx["stdout"]))
    assert out.startswith("Training Start\n") and out.count("Epoch [") == 2 and out.count("Validation Acc") == 2
    assert int(fx["training_after"]) == 0 and all(f.startswith("checkpoint") and f.endswith(".ckpt") for f in fx["ckpt_files"])
    assert len(fx["ckpt_keys"]) in (0, 56)


SCRIPT = """
import json, sys
from model.tcn import MustafaNet1DTCN, TemporalConvNet1D, TemporalBlock1D, Chomp1d
from train_tcn import train, validate
import model.tcn, train_tcn
print(json.dumps(dict(model=model.tcn.MustafaNet1DTCN.__module__, train=train.__module__, validate=validate.__module__)))
"""


def test_dropin_imports_resolve_to_r3d_amd():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", SCRIPT], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().split("\n")[-1])
    assert got == dict(model="r3d_amd.model.tcn", train="r3d_amd.train_tcn", validate="r3d_amd.train_tcn")


@pytest.mark.parametrize("B,S,K,Q,word", TC.REFUSED)
def test_check_tcn_shape_refuses(B, S, K, Q, word):
    from r3d_amd.engine_tcn import check_tcn_shape
    with pytest.raises(ValueError, match=word.replace("^", r"\^")):
        check_tcn_shape(B, S, K, Q)


@pytest.mark.parametrize("B,S,K,Q", TC.ADMITTED)
def test_check_tcn_shape_admits(B, S, K, Q):
    from r3d_amd.engine_tcn import check_tcn_shape
    check_tcn_shape(B, S, K, Q)


@pytest.mark.parametrize("B,S,K,Q", TC.ADMITTED)
def test_kernel_queries_admit_what_the_engine_admits(B, S, K, Q):
    """The library loads without a GPU; its *_supported queries are host arithmetic."""
    from r3d_amd import build, ops
    from r3d_amd.engine_tcn import TCN_IN, TCN_CHANNELS
    build.build(verbose=False)
    chans = (TCN_IN,) + TCN_CHANNELS
    for i in range(4):
        assert ops.tconv_supported(B * S, S, chans[i], chans[i + 1], 2 ** i)
        assert ops.tconv_supported(B * S, S, chans[i + 1], chans[i + 1], 2 ** i)
    assert ops.ce_rows_supported(B * Q, K)
    assert not ops.tconv_supported(B * S, S, 2040, 256, 1) and not ops.tconv_supported(B * S + 1, S + 2, 256, 256, 1)
