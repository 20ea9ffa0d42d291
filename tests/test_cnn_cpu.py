"""The CNN baseline without a GPU: the float64 restatement (tests/cnn_oracle.py) against the fixtures generated from the
imported reference and the loop fixture's per-step statistics, the recorded kernel tolerances and arg-max margins of
tests/cnn_cases.py recomputed, the host-side admission of engine_cnn, the drop-in import in a fresh interpreter with the
reference's state_dict keys, shapes and seeded initial values, and train_unimodal._unwrap over both unimodal models."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import synth
from tests import cnn_cases as CC, cnn_oracle as CO
from tests.helpers import load_fixture, fixture_params, assert_close, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["cnn_tiny", "cnn_cfg", "cnn_odd"]


def _batch(fx, seed=None, B=None):
    m = fx["meta"]
    b = synth.make_batch(B or m["B"], m["S"], m["n_class"], m["pad_idx"], m["seed"] if seed is None else seed,
                         depth_hw=tuple(m["depth_hw"]))
    if m.get("with_exclusion") or "n_steps" in m:
        b[2][0, 1:4] = 120
        b[2][2, 0] = 120
        b[4][1, 0] = 120
        b[4][3, 1] = 120
    return [torch.from_numpy(x) for x in b]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference_fixture(tag):
    fx = load_fixture(tag)
    batch = _batch(fx)
    tr = CO.Trainer(fixture_params(fx), fx["meta"]["pad_idx"])
    with torch.no_grad():
        to = CO.forward(tr.p, batch[0].double())
    res, out, _ = tr.step(batch)
    for k in ("action", "duration", "seg"):
        assert_close(out[k].detach(), fx["out_" + k], rtol=1e-5, atol=1e-5, what=k)
        assert_close(to[k], fx["test_" + k], rtol=1e-5, atol=1e-5, what="test " + k)
    assert_close(torch.tensor(stats(out["supcon"])[:3]), fx["supcon_stats"][:3], rtol=1e-5, atol=1e-5, what="supcon")
    assert_close(torch.tensor([res[k].item() for k in ("loss_seg", "loss_action", "loss_dur", "loss")]), fx["losses"],
                 rtol=1e-5, atol=1e-6, what="losses")
    assert [res[k] for k in ("seg_correct", "seg_total", "act_correct", "act_total")] == fx["counts"].tolist()
    live = [n for n, q in tr.p.items() if q.grad is not None]
    assert sorted(live) == sorted(fx["live_names"]) and len(live) == 8
    assert sorted(json.loads(str(fx["dead_names"]))) == sorted(n for n in tr.p if n not in live)
    for j, n in enumerate(fx["live_names"]):
        g = stats(tr.p[n].grad)
        assert abs(g[0] - fx["grad_stats"][j][0]) <= 1e-5 * max(1e-3, fx["grad_stats"][j][0]), n
        if "grad::" + n in fx:
            assert_close(tr.p[n].grad, fx["grad::" + n], rtol=1e-4, atol=1e-7, what=n)
        if n != "fc_len.bias":              # (its gradient is zero up to rounding: AdamW moves it either way)
            ps = stats(tr.p[n])
            assert abs(ps[0] - fx["post_stats"][j][0]) <= 1e-5 * max(1.0, fx["post_stats"][j][0]), n


def test_state_dict_has_the_references_55_entries():
    fx = load_fixture("cnn_cfg")
    assert len(json.loads(str(fx["state_keys"]))) == 55


def test_exclusion_is_exercised_by_the_k122_fixture():
    fx = load_fixture("cnn_cfg")
    _, _, lab, _, tgt = _batch(fx)
    assert fx["meta"]["n_class"] == 122 and int((lab == 120).sum()) >= 4 and int((tgt == 120).sum()) >= 2
    pad = fx["meta"]["pad_idx"]
    assert fx["counts"][1] == int(((lab != pad) & (lab != 120)).sum())
    assert fx["counts"][3] == int(((tgt != pad) & (tgt != 120)).sum())


def test_restatement_follows_the_references_loop():
    fx = load_fixture("cnn_train_loop")
    m = fx["meta"]
    tr = CO.Trainer(fixture_params(fx), m["pad_idx"], lr=m["lr"], wd=m["wd"])
    for i in range(m["n_steps"]):
        tr.step(_batch(fx, seed=m["seed"] + i))
        ost = np.stack([stats(tr.p[n]) for n in fx["live_names"]])
        want = fx["post_stats"][i][:, :3]         # (the reference stepped in float32: 2e-5 of the statistics' scale)
        assert_close(ost[:, :3], want, rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(want).max())), what=f"step {i}")
    assert fx["ckpt_files"] == ["seed_1_best.ckpt", "seed_1_checkpoint0.ckpt"]


# ---------------------------------------------------------------------------------------------------------------------
# the kernel cases: recorded tolerances and arg-max margins
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_cross_and_every_pattern():
    shapes = {r[:3] for r in CC.CASES}
    assert {(N, H, K) for N in CC.NS for H in CC.HS for K in CC.KS} <= shapes
    assert {r[3] for r in CC.CASES} == set(CC.PATTERNS)
    assert any(r[3] == "excl120" and r[2] == 121 for r in CC.CASES)
    assert any(r[3] == "tile_masked" and r[0] > 128 for r in CC.CASES)
    assert len(set(r[:4] for r in CC.CASES)) == len(CC.CASES)


@pytest.mark.parametrize("lo", range(0, len(CC.CASES), 33))
def test_recorded_tolerances_and_margins(lo):
    for row in CC.CASES[lo:lo + 33]:
        c = CC.make_case(*row[:5])
        ref = CC.reference(c)
        got, tol = CC.measure(c, ref), CC.tolerances(row)
        for q in CC.QUANTITIES:
            assert got[q] <= tol[q] * (1 + 1e-6), (row[:5], q, got[q], tol[q])          # not below the measured error
            assert tol[q] <= CC.MARGIN * got[q] * (1 + 1e-3), (row[:5], q, got[q], tol[q])    # not above 8 times it
        assert CC.min_gap_ratio(c, ref, row[5][0]) >= CC.GAP_FACTOR, row[:5]
        if row[3] == "pad_inside" and row[0] >= 63 and row[1] >= 64:   # (a dozen built rows of a width where class 2 wins)
            assert (ref["valid"] & (ref["argmax"] == c["pad_idx"])).any(), row[:5]      # the + 2 penalty is exercised
        if row[3] in ("all_masked",) or (row[3] == "tile_masked" and row[0] <= 64):
            assert not ref["valid"].any()
        if row[3] == "oob":
            assert ((c["labels"] >= c["K"]) & (c["labels"] != c["pad_idx"]) & (c["labels"] != CC.EXCLUDE)).any()
        assert (c["x"] == 0).any() and (c["x"] > 0).any()


def test_kernel_restatement_agrees_with_the_loss_composition():
    """seg_rows' units, summed as r3d_losses_finalize does, are the seg loss and counters of losses()"""
    fx = load_fixture("cnn_cfg")
    batch = _batch(fx)
    p = {n: t.double() for n, t in fixture_params(fx).items()}
    aux = {}
    out = CO.forward(p, batch[0].double(), capture=aux)
    res = CO.losses(out, batch[2], batch[3].double(), batch[4], fx["meta"]["pad_idx"])
    H = aux["x"].shape[-1]
    r = CO.seg_rows(aux["x"].reshape(-1, H).numpy(), p["fc_seg.weight"].numpy(), p["fc_seg.bias"].numpy(),
                    batch[2].reshape(-1).numpy(), fx["meta"]["pad_idx"], CO.EXCLUDE)
    N = r["units"].shape[0]
    assert abs(r["units"][:, 0].sum() / N - float(res["loss_seg"])) <= 1e-12 * N
    assert int(r["units"][:, 1].sum()) == res["seg_correct"] and int(r["units"][:, 2].sum()) == res["seg_total"]
    assert_close(r["logits"], out["seg"].reshape(N, -1), rtol=1e-12, atol=1e-12, what="logits")


# ---------------------------------------------------------------------------------------------------------------------
# host-side admission
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CC.ENGINE_ADMITTED)
def test_check_cnn_shape_admits(kw):
    from r3d_amd.engine_cnn import check_cnn_shape
    check_cnn_shape(**dict(dict(n_class=17), **kw))


@pytest.mark.parametrize("kw,word", CC.ENGINE_REFUSALS)
def test_check_cnn_shape_refuses(kw, word):
    from r3d_amd.engine_cnn import check_cnn_shape
    with pytest.raises(ValueError, match=word.replace("^", r"\^")):
        check_cnn_shape(**dict(dict(n_class=17), **kw))


def test_kernel_admission_and_chain_pays_on_the_host():
    from r3d_amd import build, ops
    from r3d_amd.engine_cnn import chain_pays
    build.build(verbose=False)
    for H in range(0, 300):
        assert ops.cnn_seg_supported(H, 121) == (8 <= H <= 256 and H % 4 == 0), H
    for K in (0, 1, 64, 1023, 1024):
        assert ops.cnn_seg_supported(128, K) == (1 <= K <= 1023), K
    for H, K in CC.REFUSED_SHAPES:
        assert not ops.cnn_seg_supported(H, K)
    for N, H, K in {r[:3] for r in CC.CASES}:
        assert ops.cnn_seg_supported(H, K)
    # the route rule is the measurement's: every shape of profiles/cnn_step_speed.json goes to the route that was faster
    prof = json.load(open(os.path.join(ROOT, "profiles", "cnn_step_speed.json")))
    seen = 0
    for key, row in prof.items():
        if not key.startswith("B"):
            continue
        B, S = (int(v[1:]) for v in key.split("_"))
        want = row["chain_ms_per_step"] < row["composed_ms_per_step"]
        assert chain_pays(B, S, prof["H"], prof["K"] - 1) == want == (row["faster"] == "chain") == row["chain_pays"], key
        seen += 1
    assert seen == 3
    assert not chain_pays(8, 16, 128, 121) and not chain_pays(16, 256, 128, 121) and chain_pays(8, 1142, 128, 121)


# ---------------------------------------------------------------------------------------------------------------------
# drop-in import, _unwrap
# ---------------------------------------------------------------------------------------------------------------------
SCRIPT = r'''
import json, sys, torch
from opts import parser                                              # main_nturgbd.py:12
from model.cnn import FUTR                                           # :19
from train_unimodal import train                                     # :32
from predict_nturgbd import predict                                  # :40
import r3d_amd.model.cnn as R, r3d_amd.train_unimodal as TU, r3d_amd.predict as P
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


@pytest.mark.parametrize("tag", ["cnn_tiny", "cnn_cfg"])
def test_model_cnn_import_resolves_through_dropin(tmp_path, tag):
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


def _args(H):
    return argparse.Namespace(input_dim=32, seg=True, anticipate=True, max_pos_len=50, input_type="i3d_transcript",
                              hidden_dim=H, n_query=8, n_head=4)


def test_unwrap_takes_both_unimodal_models_and_refuses_the_others():
    from r3d_amd import train_unimodal as TU
    from r3d_amd.model.cnn import FUTR as Cnn
    from r3d_amd.model.rnn import FUTR as Rnn
    kw = dict(n_query=8, n_head=4, num_encoder_layers=1, num_decoder_layers=1)
    for cls in (Cnn, Rnn):
        m = cls(17, 16, 18, torch.device("cpu"), _args(16), **kw)
        assert TU._unwrap(m) is m and TU._unwrap(torch.nn.DataParallel(m)) is m
    with pytest.raises(TypeError):
        TU._unwrap(torch.nn.Linear(2, 2))
    for bad in (dict(input_type="gt"), dict(seg=False), dict(anticipate=False)):
        a = _args(16)
        for k, v in bad.items():
            setattr(a, k, v)
        with pytest.raises(NotImplementedError):
            Cnn(17, 16, 18, torch.device("cpu"), a, **kw)
    with pytest.raises(ValueError, match="erank_weight"):
        TU._check_shape(Cnn(17, 16, 18, torch.device("cpu"), _args(16), **kw), 0.1)
