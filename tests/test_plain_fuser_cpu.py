"""The plain SA-Fuser model (model/futr_safuser_depth.py) without a GPU: the CPU restatement against the fixtures
generated from the imported reference, the state_dict layout and seeded init, the drop-in import path and the new entry
points of the C ABI."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import load_fixture
from tests import plain_oracle as PO
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["plain_tiny", "plain_cfg2", "plain_k122"]


def _batch(fx):
    m = fx["meta"]
    return [torch.from_numpy(x) for x in synth.make_batch(m["B"], m["S"], m["n_class"], m["pad_idx"], m["seed"],
                                                          depth_hw=tuple(m["depth_hw"]))]


def _close(a, b, name, rtol=2e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.abs(a - b).max())
    assert err <= rtol * max(1.0, float(np.abs(b).max())), f"{name}: {err}"


def _model(H=64, n_class=17, n_dec=1):
    from r3d_amd.model.futr_safuser_depth import FUTR
    args = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    return FUTR(n_class, H, n_class + 1, torch.device("cpu"), args, n_query=8, n_head=8, num_encoder_layers=2,
                num_decoder_layers=n_dec)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference_fixture(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    batch = _batch(fx)
    tr = PO.Trainer(PO.plain_params(fx), m["pad_idx"], 8, m["n_dec"], lr=m["lr"], wd=m["wd"])
    with torch.no_grad():
        vo, vaux = PO.forward(tr.p, batch[0], batch[1], "val", m["pad_idx"], 8, m["n_dec"])    # the bare tensor
    for k in ("action", "duration", "seg"):
        _close(vo[k].numpy(), fx["val_" + k], f"val/{k}")
    _close(vaux["fused"].numpy(), fx["val_fused"], "val/fused")
    res, out, aux = tr.step(batch, apply=True)
    for k in ("action", "duration", "seg"):
        _close(out[k].detach().numpy(), fx["out_" + k], k)
    _close(aux["fused"].detach().numpy(), fx["fused"], "fused")
    _close([float(res[k].detach()) for k in ("loss_seg", "loss_action", "loss_dur", "loss")], fx["losses"], "losses")
    assert [int(res[k]) for k in ("seg_correct", "seg_total", "act_correct", "act_total")] == list(fx["counts"])
    live = fx["live_names"]
    assert sorted(live) == sorted(n for n, q in tr.p.items() if q.grad is not None)
    g = tr.p["fuser.modality_token"].grad.numpy()
    _close(g, fx["grad::fuser.modality_token"], "d modality_token", rtol=5e-5)
    assert np.abs(g).max() > 1e-3                      # the token is live and its gradient is not trivially zero


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_layout_matches_reference(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    model = _model(m["H"], m["n_class"], m["n_dec"])
    assert [n for n, _ in model.named_parameters()] == fx["param_names"]
    assert [list(p.shape) for _, p in model.named_parameters()] == fx["param_shapes"]
    import json
    assert list(model.state_dict().keys()) == json.loads(str(fx["state_keys"]))
    assert not any("fusion_conv" in n for n in model.state_dict())
    assert model.depth_projection.in_features == 160 * 120


@pytest.mark.parametrize("tag", TAGS)
def test_seeded_init_matches_reference(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    torch.manual_seed(1)
    model = _model(m["H"], m["n_class"], m["n_dec"])
    sums = np.array([[float(p.detach().double().sum()), float((p.detach().double() ** 2).sum())]
                     for _, p in model.named_parameters()])
    ref = fx["init_sums"]
    assert sums.shape == ref.shape
    np.testing.assert_allclose(sums, ref, rtol=1e-9, atol=1e-9)


def test_dropin_import_path():
    code = ("from model.futr_safuser_depth import FUTR, CMFuser; "
            "import r3d_amd.model.futr_safuser_depth as M; assert FUTR is M.FUTR and CMFuser is M.CMFuser; "
            "assert CMFuser.r3d_fuser_kind == 'plain'")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_training_loop_accepts_the_model():
    from r3d_amd.train_proposed_depth import _unwrap
    m = _model()
    assert _unwrap(m) is m


def test_engine_refuses_hidden_past_the_seam():
    from r3d_amd import engine
    engine.check_engine_shape(1024, 8, 8, plain=True)
    with pytest.raises(ValueError, match="plain SA-Fuser"):
        engine.check_engine_shape(1040, 16, 8, plain=True)
    engine.check_engine_shape(1040, 16, 8)                    # (the token-fusion model has no such limit)


def test_abi_declares_and_exports_the_plain_seam():
    from r3d_amd import build, _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r3d_hip.h")).read(), flags=re.S)
    build.build(verbose=False)
    lib = _lib.load()
    for name in ("r3d_plain_fuse_fwd", "r3d_plain_fuse_bwd"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.r3d_abi_version() == 2


def test_plain_seam_rejects_bad_arguments_before_launching():
    """Null pointers, unsupported widths and a half-given output set return R3D_EINVAL on the host (no device memory is
    touched)."""
    from r3d_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    f = 1 << 20                                             # never dereferenced: the checks fail first

    def fwd(tok=f, H=64, N=4, ns_d=1, jobs=None, nj=0, nb=0):
        return lib.r3d_plain_fuse_fwd(f, 0, None, f, ns_d, None, f, f, tok, None, 1.0, f, f, f, f, f, f, f, f, f, f, f,
                                      N, H, jobs, nj, nb, None)
    assert fwd(tok=None) == -1
    assert fwd(H=2048) == -1
    assert fwd(N=0) == -1
    assert fwd(ns_d=0) == -1
    assert fwd(jobs=f, nj=0, nb=4) == -1

    def bwd(t_tok=f, H=64, N=4, full=True, half=False):
        o = f if full else None
        return lib.r3d_plain_fuse_bwd(f, f, f, f, f, None, None, 1.0, f, f, f, f, f, f, o, None if half else o, o, o,
                                      t_tok, N, H, None)
    assert bwd(t_tok=None) == -1
    assert bwd(H=2048) == -1
    assert bwd(N=0) == -1
    assert bwd(half=True) == -1
