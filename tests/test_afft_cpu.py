"""The AFFT baseline (model/afft.py) without a GPU: the CPU restatement against the fixtures generated from the imported
reference, the state_dict layout and seeded init, the drop-in import path, the pooling windows against torch, the engine's
shape admission and refusals, the live set, and the new entry points of the C ABI."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import load_fixture, fixture_params
from tests import afft_cases as AC
from tests import afft_oracle as AO
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["afft_tiny", "afft_cfg2", "afft_odd"]


def _batch(fx):
    m = fx["meta"]
    return [torch.from_numpy(x) for x in synth.make_batch(m["B"], m["S"], m["n_class"], m["pad_idx"], m["seed"],
                                                          depth_hw=tuple(m["depth_hw"]))]


def _close(a, b, name, rtol=2e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.abs(a - b).max())
    assert err <= rtol * max(1.0, float(np.abs(b).max())), f"{name}: {err}"


def _model(H=64, n_class=17, seg=False, n_enc=2, **kw):
    from r3d_amd.model.afft import FUTR
    args = argparse.Namespace(input_dim=2048, seg=seg, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
    return FUTR(n_class, H, n_class + 1, torch.device("cpu"), args, n_query=8, n_head=8, num_encoder_layers=n_enc,
                num_decoder_layers=1, **kw)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference_fixture(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    batch = _batch(fx)
    tr = AO.Trainer(fixture_params(fx), m["pad_idx"], 8, 8, lr=m["lr"], wd=m["wd"])
    with torch.no_grad():
        vo, vaux = AO.forward(tr.p, batch[0], batch[1], "val", m["pad_idx"], 8, 8)              # the bare tensor
    assert sorted(vo) == ["action", "duration"]
    for k in ("action", "duration"):
        _close(vo[k].numpy(), fx["val_" + k], f"val/{k}")
    _close(vaux["fused"].numpy(), fx["val_fused"], "val/fused")
    res, out, aux = tr.step(batch, apply=True)
    for k in ("action", "duration"):
        _close(out[k].detach().numpy(), fx["out_" + k], k)
    _close(aux["fused"].detach().numpy(), fx["fused"], "fused")
    _close([float(res[k].detach()) for k in ("loss_seg", "loss_action", "loss_dur", "loss")], fx["losses"], "losses")
    assert [int(res[k]) for k in ("seg_correct", "seg_total", "act_correct", "act_total")] == list(fx["counts"])
    live = fx["live_names"]
    assert sorted(live) == sorted(n for n, q in tr.p.items() if q.grad is not None)
    for n in ("fuser.modality_token", "fuser.norm.weight", "depth_layernorm.weight", "input_embed.bias", "fc.bias", "fc_len.weight"):
        _close(tr.p[n].grad.numpy(), fx["grad::" + n], f"grad {n}", rtol=5e-5)
    assert np.abs(tr.p["fuser.modality_token"].grad.numpy()).max() > 1e-4


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_layout_and_seeded_init_match_reference(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    torch.manual_seed(1)
    model = _model(m["H"], m["n_class"], n_enc=m["n_encoder_layer"])
    assert [n for n, _ in model.named_parameters()] == fx["param_names"]
    assert [list(p.shape) for _, p in model.named_parameters()] == fx["param_shapes"]
    assert list(model.state_dict().keys()) == json.loads(str(fx["state_keys"]))
    assert model.depth_projection.in_features == 224 * 224
    sums = np.array([[float(p.detach().double().sum()), float((p.detach().double() ** 2).sum())]
                     for _, p in model.named_parameters()])
    assert sums.shape == fx["init_sums"].shape
    np.testing.assert_allclose(sums, fx["init_sums"], rtol=1e-9, atol=1e-9)
    with_seg = _model(m["H"], m["n_class"], seg=True, n_enc=m["n_encoder_layer"])
    assert list(with_seg.state_dict().keys()) == json.loads(str(fx["state_keys_seg"]))
    with_seg.load_state_dict(with_seg.state_dict(), strict=True)


def test_dropin_import_path():
    code = ("from model.afft import FUTR, CMFuser; import r3d_amd.model.afft as M; "
            "assert FUTR is M.FUTR and CMFuser is M.CMFuser and CMFuser.r3d_fuser_kind == 'plain'")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_training_loop_and_rank_stream_accept_the_model():
    from r3d_amd.rankstream import _fuser_core
    from r3d_amd.train_proposed_depth import _unwrap
    m = _model()
    assert _unwrap(m) is m and _fuser_core(m) is m
    assert m.depth_projection.in_features == 224 * 224 and _model(depth_pixels=48).depth_projection.in_features == 48


@pytest.mark.parametrize("Q", [1, 3, 8, 32])
def test_pool_windows_against_torch(Q):
    for S in range(1, 71):
        x = torch.arange(S, dtype=torch.float64)[None, :, None] * torch.tensor([1.0, -0.5])[None, None, :] + 0.25
        ref = torch.nn.functional.adaptive_avg_pool1d(x.permute(0, 2, 1), Q).permute(0, 2, 1)
        win = AO.pool_windows(S, Q)
        assert len(win) == Q and all(0 <= s0 < s1 <= S for s0, s1 in win), (S, Q, win)
        mine = torch.stack([x[:, s0:s1].mean(dim=1) for s0, s1 in win], dim=1)
        assert torch.allclose(mine, ref, rtol=0, atol=1e-12), (S, Q)
        assert torch.allclose(AO.pool(x, Q), ref, rtol=0, atol=1e-12), (S, Q)
        cover = sum(s1 - s0 for s0, s1 in win)
        assert (cover > S) == (S % Q != 0), (S, Q)          # frames repeat (S < Q) / windows overlap exactly when S % Q != 0
        assert all(win[q + 1][0] >= win[q][1] - 1 for q in range(Q - 1))        # ... by at most one frame


def test_check_afft_shape_admits_and_refuses():
    from r3d_amd import build
    from r3d_amd.engine_afft import check_afft_shape
    build.build(verbose=False)
    for row in AC.ADMITTED:
        check_afft_shape(*row)
    for row, word in AC.REFUSED:
        with pytest.raises(ValueError, match=re.escape(word)):
            check_afft_shape(*row)


def test_lds_limit_of_the_engine_is_the_kernels():
    from r3d_amd import build, _lib
    from r3d_amd import engine_afft as E
    build.build(verbose=False)
    lib = _lib.load()
    for H, Q, K1 in [(1024, 32, 123), (1024, 36, 18), (1024, 37, 18), (1024, 38, 18), (512, 64, 18), (1024, 64, 123),
                     (128, 8, 18), (8, 1, 2), (1024, 65, 18), (128, 8, 1024), (128, 8, 1025)]:
        host = (1 <= Q <= E.AFFT_MAX_Q and 1 <= K1 - 1 < E.AFFT_MAX_HEADS and 4 * Q * (H + K1) <= E.AFFT_LDS_BYTES)
        assert bool(lib.r3d_afft_head_supported(H, Q, K1)) == host, (H, Q, K1)


def test_refusals_name_their_reason():
    from r3d_amd.engine_afft import check_afft_args
    check_afft_args()
    with pytest.raises(ValueError, match="no 'seg' output"):
        check_afft_args(seg=True)
    with pytest.raises(ValueError, match="effective-rank penalty"):
        check_afft_args(erank_weight=0.1)
    with pytest.raises(ValueError, match="one GPU"):
        check_afft_args(parallel=True)


def test_live_set():
    from r3d_amd.engine_afft import is_live
    fx = load_fixture("afft_tiny")
    assert sorted(n for n in fx["param_names"] if is_live(n)) == sorted(fx["live_names"])
    assert sorted(n for n in fx["param_names"] if AO.is_live(n)) == sorted(fx["live_names"])
    dead = [n for n in fx["param_names"] if not is_live(n)]
    for pre in ("transformer.", "query_embed.", "pos_embedding", "l3_attention.", "query_attention.", "fc_l3.", "fuser.projection."):
        assert any(n.startswith(pre) for n in dead), pre
    assert is_live("fuser.blocks.0.attn.qkv.weight") and is_live("fuser.modality_token") and not is_live("fc_seg.weight")
    assert not is_live("fc_l3.weight") and is_live("fc_len.bias")


def test_abi_declares_exports_and_validates_the_pooled_head_chain():
    import ctypes as C
    from r3d_amd import build, _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r3d_hip.h")).read(), flags=re.S)
    build.build(verbose=False)
    lib = _lib.load()
    for name in ("r3d_afft_head_supported", "r3d_afft_head_fwd", "r3d_afft_head_step"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    f = 1 << 20                                             # never dereferenced: the checks fail first

    def args(**kw):
        a = _lib.AfftHeadArgs()
        base = dict(fused=f, ld_fused=64, w_head=f, b_head=f, n_head=18, pooled=f, out=f, ld_out=18, B=2, S=6, Q=8, K=17, H=64,
                    past_label=f, target=f, target_dur=f, pad_idx=18, exclude_idx=47, d_out=f, ld_dout=18, d_fused=f,
                    ld_dfused=64, gscale=1.0, add=0)
        base.update(kw)
        for k, v in base.items():
            setattr(a, k, v)
        return a
    fwd = lambda **kw: lib.r3d_afft_head_fwd(C.byref(args(**kw)), None)            # noqa: E731
    step = lambda ws=f, **kw: lib.r3d_afft_head_step(C.byref(args(**kw)), ws, None)     # noqa: E731
    assert lib.r3d_afft_head_fwd(None, None) == -1 and lib.r3d_afft_head_step(None, f, None) == -1
    for bad in (dict(fused=None), dict(pooled=None), dict(n_head=17), dict(B=0), dict(S=0), dict(Q=0), dict(Q=65), dict(H=66),
                dict(H=2048), dict(ld_fused=32), dict(ld_out=17), dict(H=1024, Q=64, ld_fused=1024)):
        assert fwd(**bad) == -1, bad
        assert step(**bad) == -1, bad
    assert fwd(fused=f + 4) == -2 and fwd(ld_fused=66) == -2
    for bad in (dict(target=None), dict(d_out=None), dict(d_fused=None), dict(ld_dout=17), dict(ld_dfused=32), dict(add=2)):
        assert step(**bad) == -1, bad
    assert step(ws=None) == -1 and step(ws=f + 4) == -2 and step(d_fused=f + 8) == -2 and step(ld_dfused=66) == -2
