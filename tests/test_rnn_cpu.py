"""The RNN baseline without a GPU: the float64 restatement (tests/rnn_oracle.py) against the fixtures generated from the
imported reference, the host-side shape admission of engine_rnn, and main_nturgbd.py's import lines resolving through
dropin/ in a fresh interpreter with the reference's state_dict keys, shapes and seeded initial values."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import synth
from tests import rnn_oracle as RO
from tests.helpers import load_fixture, fixture_params, assert_close, stats
from tests.rnn_cases import ADMITTED_H, REFUSED_H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(fx):
    m = fx["meta"]
    b = synth.make_batch(m["B"], m["S"], m["n_class"], m["pad_idx"], m["seed"], depth_hw=tuple(m["depth_hw"]))
    if m.get("with_exclusion"):
        b[2][0, 1:4] = 120
        b[2][2, 0] = 120
        b[4][1, 0] = 120
        b[4][3, 1] = 120
    return [torch.from_numpy(x) for x in b]


@pytest.mark.parametrize("tag", ["rnn_tiny", "rnn_cfg"])
def test_restatement_matches_reference_fixture(tag):
    fx = load_fixture(tag)
    batch = _batch(fx)
    tr = RO.Trainer(fixture_params(fx), fx["meta"]["pad_idx"])
    with torch.no_grad():
        to = RO.forward(tr.p, batch[0].double())
    res, out, _ = tr.step(batch)
    for k in ("action", "duration", "seg"):
        assert_close(out[k].detach(), fx["out_" + k], rtol=1e-5, atol=1e-5, what=k)
        assert_close(to[k], fx["test_" + k], rtol=1e-5, atol=1e-5, what="test " + k)
    assert_close(torch.tensor([res[k].item() for k in ("loss_seg", "loss_action", "loss_dur", "loss")]), fx["losses"],
                 rtol=1e-5, atol=1e-6, what="losses")
    assert [res[k] for k in ("seg_correct", "seg_total", "act_correct", "act_total")] == fx["counts"].tolist()
    live = [n for n, q in tr.p.items() if q.grad is not None]
    assert sorted(live) == sorted(fx["live_names"])
    assert sorted(json.loads(str(fx["dead_names"]))) == sorted(n for n in tr.p if n not in live)
    for j, n in enumerate(fx["live_names"]):
        g = stats(tr.p[n].grad)
        assert abs(g[0] - fx["grad_stats"][j][0]) <= 1e-5 * max(1e-3, fx["grad_stats"][j][0]), n
        if "grad::" + n in fx:
            assert_close(tr.p[n].grad, fx["grad::" + n], rtol=1e-4, atol=1e-7, what=n)


def test_exclusion_is_exercised_by_the_k122_fixture():
    fx = load_fixture("rnn_cfg")
    _, _, lab, _, tgt = _batch(fx)
    assert fx["meta"]["n_class"] == 122 and int((lab == 120).sum()) >= 4 and int((tgt == 120).sum()) >= 2
    pad = fx["meta"]["pad_idx"]
    assert fx["counts"][1] == int(((lab != pad) & (lab != 120)).sum())
    assert fx["counts"][3] == int(((tgt != pad) & (tgt != 120)).sum())


def test_restated_lstm_gate_adjoint_matches_autograd():
    g = torch.Generator().manual_seed(3)
    B, S, H = 3, 7, 8
    h = H // 2
    w = {(k, d): torch.randn(*(sh), generator=g, dtype=torch.float64) * 0.4
         for d in (0, 1) for k, sh in (("w_ih", (4 * h, H)), ("w_hh", (4 * h, h)), ("b_ih", (4 * h,)), ("b_hh", (4 * h,)))}
    x = torch.randn(B, S, H, generator=g, dtype=torch.float64)
    dy = torch.randn(B, S, H, generator=g, dtype=torch.float64)
    r = RO.lstm_layer_grads(x, w, dy)
    # d b_ih (autograd) = column sums of the explicit adjoint's dG, per direction
    for d in (0, 1):
        assert torch.allclose(r["dg"][..., 4 * h * d:4 * h * (d + 1)].sum((0, 1)), r["db"][d], atol=1e-10)
    # dX (autograd) = dG W_ih, summed over the directions
    wih = torch.cat([w[("w_ih", 0)], w[("w_ih", 1)]], 0)
    assert torch.allclose(r["dg"] @ wih, r["dx"], atol=1e-10)


@pytest.mark.parametrize("H", ADMITTED_H)
def test_check_rnn_shape_admits(H):
    from r3d_amd.engine_rnn import check_rnn_shape
    check_rnn_shape(H, 8, 0.0)


@pytest.mark.parametrize("H", REFUSED_H)
def test_check_rnn_shape_refuses_hidden(H):
    from r3d_amd.engine_rnn import check_rnn_shape
    with pytest.raises(ValueError, match="hidden"):
        check_rnn_shape(H, 8, 0.0)


@pytest.mark.parametrize("n_query", [1, 7, 9, 19])
def test_check_rnn_shape_refuses_n_query(n_query):
    from r3d_amd.engine_rnn import check_rnn_shape
    with pytest.raises(ValueError, match="n_query"):
        check_rnn_shape(128, n_query, 0.0)


def test_check_rnn_shape_refuses_erank_weight():
    from r3d_amd.engine_rnn import check_rnn_shape
    with pytest.raises(ValueError, match="erank_weight"):
        check_rnn_shape(128, 8, 0.1)


def test_engine_range_matches_kernel_range():
    from r3d_amd import build, ops
    from r3d_amd.engine_rnn import check_rnn_shape
    build.build(verbose=False)
    for H in range(0, 300):
        try:
            check_rnn_shape(H, 8, 0.0)
            ok = True
        except ValueError:
            ok = False
        assert ok == ops.lstm_supported(H), H


SCRIPT = r'''
import json, sys, torch
from opts import parser                                              # main_nturgbd.py:12
from pl_bolts.optimizers.lr_scheduler import LinearWarmupCosineAnnealingLR   # :13
from utils import read_mapping_dict                                  # :16
from model.rnn import FUTR                                           # :20
from train_unimodal import train                                     # :32
from predict_nturgbd import predict                                  # :40
import r3d_amd.model.rnn as R, r3d_amd.train_unimodal as TU, r3d_amd.predict as P
assert FUTR is R.FUTR and train is TU.train and predict is P.predict_nturgbd
args = parser.parse_args([])
args.hidden_dim, args.n_query = int(sys.argv[1]), 8
torch.manual_seed(1)
m = FUTR(int(sys.argv[2]), args.hidden_dim, device=torch.device("cpu"), args=args, src_pad_idx=int(sys.argv[2]) + 1,
         n_query=args.n_query, n_head=args.n_head, num_encoder_layers=args.n_encoder_layer,
         num_decoder_layers=args.n_decoder_layer)
sd = m.state_dict()
print(json.dumps(dict(keys=list(sd), shapes=[list(v.shape) for v in sd.values()],
                      sums=[[float(p.double().sum()), float((p.double() ** 2).sum())] for _, p in m.named_parameters()])))
'''


@pytest.mark.parametrize("tag", ["rnn_tiny", "rnn_cfg"])
def test_main_nturgbd_imports_resolve_through_dropin(tmp_path, tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", SCRIPT, str(m["H"]), str(m["n_class"])], env=env, capture_output=True,
                       text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().split("\n")[-1])
    assert got["keys"] == json.loads(str(fx["state_keys"]))
    assert got["shapes"] == json.loads(str(fx["state_shapes"]))
    np.testing.assert_allclose(np.array(got["sums"]), fx["init_sums"], rtol=1e-9, atol=1e-9)
