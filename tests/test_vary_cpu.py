"""The activation-magnitude fuser variant (model/futr_safuser_tokenfusion_vary.py) without a GPU: the CPU restatement
against the fixtures generated from the imported reference, the state_dict layout, the drop-in import path and the new
entry points of the C ABI."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import load_fixture
from tests import vary_oracle as V
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["vary_tiny", "vary_cfg2", "vary_k122"]


def _batch(fx):
    m = fx["meta"]
    return [torch.from_numpy(x) for x in synth.make_batch(m["B"], m["S"], m["n_class"], m["pad_idx"], m["seed"],
                                                          depth_hw=tuple(m["depth_hw"]))]


def _close(a, b, name, rtol=2e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.abs(a - b).max())
    assert err <= rtol * max(1.0, float(np.abs(b).max())), f"{name}: {err}"


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference_fixture(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    batch = _batch(fx)
    tr = V.Trainer(V.vary_params(fx), m["pad_idx"], 8, m["n_dec"], lr=m["lr"], wd=m["wd"])
    with torch.no_grad():
        vo, vaux = V.forward(tr.p, (batch[0], batch[2]), batch[1], "val", m["pad_idx"], 8, m["n_dec"])
    for k in ("action", "duration", "seg"):
        _close(vo[k], fx["val_" + k], f"{tag}/val {k}")
    assert np.array_equal(vaux["idx_rgb"].numpy(), fx["val_idx_rgb"])
    res, out, aux = tr.step(batch, apply=False)
    for k in ("action", "duration", "seg"):
        _close(out[k].detach(), fx["out_" + k], f"{tag}/{k}")
    _close(aux["fused"].detach(), fx["fused"], f"{tag}/fused")
    assert np.array_equal(aux["idx_rgb"].numpy(), fx["idx_rgb"])
    assert np.array_equal(aux["idx_dep"].numpy(), fx["idx_dep"])
    _close([float(res[k]) for k in ("loss_seg", "loss_action", "loss_dur", "loss")], fx["losses"], f"{tag}/losses")
    assert [int(res[k]) for k in ("seg_correct", "seg_total", "act_correct", "act_total")] == fx["counts"].tolist()
    assert sorted(fx["live_names"]) == sorted(n for n, q in tr.p.items() if q.grad is not None)
    _close(tr.p["fuser.alpha"].grad, fx["grad::fuser.alpha"], f"{tag}/d alpha", rtol=5e-5)
    assert float(tr.p["fuser.alpha"].grad.abs().max()) > 0
    for j, n in enumerate(fx["live_names"]):
        _close(tr.p[n].grad.double().norm(), fx["grad_stats"][j][0], f"{tag}/|grad {n}|", rtol=5e-5)


def test_tie_case_selects_by_the_topk_rule():
    """vary_tiny: 20 RGB channels score exactly 0 and k = 16 of them are chosen; the fixture pins which."""
    fx = load_fixture("vary_tiny")
    dead = fx["meta"]["dead_rgb"]
    assert len(dead) == 20 and fx["gap_rgb"][0] == 0.0
    assert set(fx["idx_rgb"].tolist()) < set(dead)


def _model(H=64, K=17):
    from r3d_amd.model.futr_safuser_tokenfusion_vary import FUTR
    args = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    return FUTR(K, H, K + 1, torch.device("cpu"), args, n_query=8, n_head=8, num_encoder_layers=2, num_decoder_layers=1)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_layout_matches_reference(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    model = _model(m["H"], m["n_class"])
    names = [n for n, _ in model.named_parameters()]
    assert names == fx["param_names"]
    assert [list(p.shape) for _, p in model.named_parameters()] == fx["param_shapes"]
    assert torch.equal(model.fuser.alpha, torch.ones(1, 1, m["H"]))


def test_seeded_init_equals_token_fusion_model():
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR as Base
    args = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    torch.manual_seed(3)
    a = _model()
    torch.manual_seed(3)
    b = Base(17, 64, 18, torch.device("cpu"), args, n_query=8, n_head=8, num_encoder_layers=2, num_decoder_layers=1)
    sb = b.state_dict()
    for n, t in a.state_dict().items():
        if n != "fuser.alpha":
            assert torch.equal(t, sb[n]), n


def test_dropin_import_path():
    code = ("from model.futr_safuser_tokenfusion_vary import FUTR, CMFuser; "
            "import r3d_amd.model.futr_safuser_tokenfusion_vary as M; assert FUTR is M.FUTR and CMFuser is M.CMFuser")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_abi_declares_and_exports_the_scaled_exchange():
    from r3d_amd import build, _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r3d_hip.h")).read(), flags=re.S)
    build.build(verbose=False)
    lib = _lib.load()
    for name in ("r3d_scaled_exchange_fwd", "r3d_scaled_exchange_bwd"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.r3d_abi_version() == 2


def test_scaled_exchange_rejects_bad_arguments_before_launching():
    """Null pointers and unsupported widths return R3D_EINVAL on the host (no device memory is touched)."""
    from r3d_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    fake = 1 << 20                                             # never dereferenced: the checks fail first
    assert lib.r3d_scaled_exchange_fwd(None, fake, fake, fake, fake, None, 1.0, fake, fake, fake, fake, fake, fake,
                                       4, 64, None) == -1
    assert lib.r3d_scaled_exchange_fwd(fake, fake, fake, fake, fake, None, 1.0, fake, fake, fake, fake, fake, fake,
                                       4, 2048, None) == -1
    assert lib.r3d_scaled_exchange_bwd(fake, fake, fake, fake, fake, None, None, 1.0, fake, fake, fake, fake, fake,
                                       fake, fake, None, None, 4, 64, None) == -1
    assert lib.r3d_scaled_exchange_bwd(fake, fake, fake, fake, fake, None, None, 1.0, fake, fake, fake, fake, fake,
                                       fake, fake, fake, None, 0, 64, None) == -1
