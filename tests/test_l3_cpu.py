"""The L3 query model's kernels without a GPU: the float64 restatement (tests/l3_oracle.py) against autograd, the case
table's coverage and tolerances (tests/l3_cases.py), the tie condition, and the host-only admission of the cross-clip
attention."""
import numpy as np
import pytest
import torch

from r3d_amd import engine_l3, train_unsupervised  # noqa: F401  (the feature under test: without it nothing here is collected)
from tests import l3_cases as LC, l3_oracle as LO


# ---------------------------------------------------------------------------------------------------------------------
# cross-clip attention
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,H,heads", [(1, 3, 8, 8), (2, 1, 12, 3), (5, 4, 16, 2), (13, 3, 68, 2)])
def test_xclip_adjoint_equals_autograd(B, S, H, heads):
    g = torch.Generator().manual_seed(B * 100 + S)
    qkv = torch.randn(B, S, 3 * H, generator=g, dtype=torch.float64, requires_grad=True)
    d_o = torch.randn(B, S, H, generator=g, dtype=torch.float64)
    o = LO.xclip_fwd(qkv, heads)
    (auto,) = torch.autograd.grad(o, qkv, d_o)
    hand = LO.xclip_bwd(qkv.detach(), d_o, heads)
    assert LC.rel_err(hand, auto) < 1e-13


def test_xclip_restates_multihead_attention_over_the_clips():
    """nn.MultiheadAttention(batch_first=True) on 't b c' rows: batch = frames, sequence = clips"""
    B, S, H, heads = 5, 3, 16, 4
    torch.manual_seed(3)
    mha = torch.nn.MultiheadAttention(H, heads, batch_first=True).double()
    x = torch.randn(B, S, H, dtype=torch.float64)
    xt = x.transpose(0, 1)                                          # 'b t c -> t b c'
    want, _ = mha(xt, xt, xt)
    qkv = x @ mha.in_proj_weight.T + mha.in_proj_bias
    got = LO.xclip_fwd(qkv, heads) @ mha.out_proj.weight.T + mha.out_proj.bias
    assert LC.rel_err(got.detach(), want.detach().transpose(0, 1)) < 1e-13


def test_xclip_orders_are_the_same_function():
    case = LC.XCLIP_BY_NAME["B13_S5_H136_h4"] if "B13_S5_H136_h4" in LC.XCLIP_BY_NAME else LC.XCLIP[0]
    qkv, d_o = LC.xclip_inputs(case)
    (o1, d1), (o2, d2) = LO.xclip_orders(qkv, d_o, case["heads"])
    assert LC.rel_err(o1, o2) < 1e-4 and LC.rel_err(d1, d2) < 1e-4
    assert not torch.equal(o1, o2) or case["B"] == 1               # (a different order: other bits)


def test_xclip_table_covers_the_cross_and_both_sides_of_a_frame_run():
    from r3d_amd import build, ops
    build.build(verbose=False)
    seen = {}
    for c in LC.XCLIP:
        B, S, H, heads = c["B"], c["S"], c["H"], c["heads"]
        dh = H // heads
        assert ops.xclip_supported(B, dh) and B * S * 3 * H < 2 ** 31
        for bwd in (False, True):
            ft = ops.xclip_frame_run(B, S, heads, dh, bwd)
            assert 1 <= ft <= S
            seen.setdefault((B, dh, bwd), set()).add("one" if S <= ft else ("many_partial" if S % ft else "many"))
    assert {k[0] for k in seen} == set(LC.CLIPS) and {k[1] for k in seen} == {H // h for H, h in LC.WIDTHS}
    for key, kinds in seen.items():
        assert kinds & {"many", "many_partial"}, key
        assert "one" in kinds, key
    assert {c["S"] for c in LC.XCLIP} >= {1, 5, 64, 200}
    # a run longer than one frame occurs, with S below it, at it and above it
    runs = {(c["S"], ops.xclip_frame_run(c["B"], c["S"], c["heads"], c["H"] // c["heads"], False)) for c in LC.XCLIP}
    assert any(ft > 1 and S > ft and S % ft for S, ft in runs) and any(S == 1 for S, ft in runs)


def test_xclip_admission():
    from r3d_amd import build, ops
    build.build(verbose=False)
    for B in range(0, 70):
        assert ops.xclip_supported(B, 16) == (1 <= B <= 64), B
    for dh in (0, 1, 34, 128, 129, 256):
        assert ops.xclip_supported(8, dh) == (1 <= dh <= 128), dh
    assert ops.xclip_frame_run(65, 4, 8, 16, False) == 0 and ops.xclip_frame_run(8, 4, 8, 256, True) == 0


@pytest.mark.parametrize("name", [c["name"] for c in LC.XCLIP if c["B"] * c["S"] * c["H"] <= 120_000])
def test_xclip_tolerances_come_from_the_float32_restatement(name):
    ref = LC.xclip_reference(name)
    case = LC.XCLIP_BY_NAME[name]
    # float32: a few epsilon per operation over at most B + dh terms; never looser than 1e-4 of the tensor's scale
    bound = LC.MARGIN * 4 * LC.EPS32 * (case["B"] + case["H"] // case["heads"])
    assert ref["tol_o"] <= bound and ref["tol_d"] <= bound, (ref["tol_o"], ref["tol_d"], bound)
    if case["B"] > 1:
        assert ref["err_o"] > 0 and ref["err_d"] > 0                # (not exact by accident)


# ---------------------------------------------------------------------------------------------------------------------
# mix
# ---------------------------------------------------------------------------------------------------------------------
def test_mix_cases_cover_the_issue_list():
    assert {c["N"] for c in LC.MIX} >= {1, 63, 64, 65, 4097}
    assert {c["Kseg"] for c in LC.MIX} >= {2, 18, 123}
    assert {c["wf"] for c in LC.MIX} >= {0.0, 0.5, 1.0}
    assert any(c["ties"] for c in LC.MIX) and any(c["pad_rows"] > 0 for c in LC.MIX)


@pytest.mark.parametrize("name", [c["name"] for c in LC.MIX])
def test_mix_oracle_and_tie_condition(name):
    case = LC.MIX_BY_NAME[name]
    c, ref = LC.mix_reference(case)
    N = case["N"]
    # the tie condition: outside the constructed ties the two largest logits of every row differ
    gap = LO.top_two_gap(c["seg"])
    rest = np.setdiff1d(np.arange(N), c["tie_rows"])
    assert (gap[rest] > 0).all()
    assert (gap[c["tie_rows"]] == 0).all()
    # the rule itself, against torch on the untied rows and by construction on the tied ones
    t_arg = torch.from_numpy(c["seg"]).argmax(1).numpy()
    assert (LO.first_argmax(c["seg"])[rest] == t_arg[rest]).all()
    for row in c["tie_rows"]:
        assert ref["l2_correct"][row] == (row % 2 == 0)
    masked = c["label"] == c["pad"]
    assert not ref["l2_correct"][masked].any()
    if case["pad_rows"] > 0 and N > 2:
        assert masked[1] and LO.first_argmax(c["seg"])[1] == c["pad"]
    # m as torch forms it
    how = torch.where(torch.from_numpy(ref["l2_correct"] & c["l3"]), torch.tensor(1.0), torch.tensor(5.0))
    assert np.float32(how.mean().item()) == ref["m"]
    if case["kind"] == "all":
        assert ref["m"] == 1.0 and ref["a"] == 0.0 and ref["b"] == 0.0 and ref["c"] == 1.0
    if case["kind"] == "none":
        assert ref["m"] == 5.0
    # the mixed total against the reference's expression in torch float64
    L3, Lc, Lseg, Lact, Ldur = (torch.tensor(float(v), dtype=torch.float64) for v in c["losses"])
    hm, wf = how.double().mean() if N * 5 < 2 ** 24 else None, case["wf"]
    want = (1 - 1 / hm) * ((1 - wf) * L3 + wf * Lc) + (1 / hm) * (Lact + Ldur + Lseg)
    assert abs(float(want) - float(ref["total"])) <= 1e-6       # (m: the float32 mean, as the loop's float32 tensors give)
    assert abs(float(ref["a"] + ref["b"] + ref["c"]) - 1.0) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# whole step: the float64 restatement against the fixtures made from the reference; the tie condition; admission; dropin
# ---------------------------------------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402

from tests.helpers import load_fixture, fixture_params, stats  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TAGS = [c["tag"] for c in LC.STEP_CASES]


def _fixture_batch(fx):
    c = LC.STEP_BY_TAG[fx["meta"]["tag"]]
    b = LC.batch(c, fx["meta"]["seed"])
    b[1], b[4] = torch.from_numpy(fx["past_label"]), torch.from_numpy(fx["query_label"])
    return c, b


def test_step_fixtures_are_the_issue_shapes():
    want = {"l3_tiny": (8, 5, 16, 2), "l3_cfg": (8, 16, 128, 8), "l3_odd": (13, 37, 136, 4)}
    for tag, shape in want.items():
        m = load_fixture(tag)["meta"]
        assert (m["B"], m["S"], m["H"], m["n_head"]) == shape and m["query_num"] == 49
        assert m["wfs"] == [0.0, 1.0 / 30.0, 1.0]
    fx = load_fixture("l3_odd")
    assert (fx["past_label"][:, -1] == fx["meta"]["pad_idx"]).all()          # ragged clips ending in padding
    assert len({int((row == fx["meta"]["pad_idx"]).sum()) for row in fx["past_label"]}) > 1
    out = json.loads(str(load_fixture("l3_train_loop")["stdout"]))
    assert out.count("Epoch [") == 3 and "l3 accuracy" in out and "l3 loss" in out


@pytest.mark.parametrize("tag", STEP_TAGS)
def test_oracle_equals_the_reference_fixture_and_rows_are_untied(tag):
    fx = load_fixture(tag)
    c, b = _fixture_batch(fx)
    p0 = fixture_params(fx)
    for wi, wf in enumerate(LC.WFS):
        ref = LC.step_reference(c, b, p0, wf)
        res = ref["res"]
        got = np.array([float(res[k].detach()) for k in ("L3", "Lc", "Lseg", "Lact", "Ldur", "total")])
        assert np.abs(got - fx[f"losses_wf{wi}"]).max() <= 2e-5 * max(1.0, np.abs(got).max())
        live = fx["live_names"]
        assert sorted(live) == sorted(ref["live"])
        gs = np.stack([stats(ref["grads"][n]) for n in live])
        fs = fx[f"grad_stats_wf{wi}"]
        assert (np.abs(gs[:, 0] - fs[:, 0]) <= 5e-5 * np.maximum(1.0, fs[:, 0])).all()
        assert all(g is None for n, g in ref["grads"].items() if n not in live)
        if wi == 0:
            assert (ref["res"]["l3_correct"].numpy() == fx["l3_correct"]).all() and (res["l2_correct"].numpy() == fx["l2_correct"]).all()
            assert res["counts"] + res["l3_counts"] == fx["counts"].tolist()
            assert np.float32(float(res["m"])) == fx["m"] and 1.0 < float(fx["m"]) < 5.0
            # the float32 restatement decides every row as float64 does: the tolerances are not inflated by a flipped flag
            assert torch.equal(ref["flags32"][0], res["l3_correct"]) and torch.equal(ref["flags32"][1], res["l2_correct"])
            for k in ("action", "duration"):
                assert LC.rel_err(ref["out"][k].detach(), fx["out_" + k]) <= 2e-5
    # the tie condition: every row's top-two gap, seg and l3, exceeds 4 x the case's logit tolerance
    out64, tol = LC.forward_tolerances(c, b, p0)
    assert LC.tie_margin(out64, tol) > 1.0, LC.tie_margin(out64, tol)
    assert 0 < tol["seg"] < 1e-4 and 0 < tol["l3"] < 1e-4


@pytest.mark.parametrize("tag", STEP_TAGS)
def test_post_adamw_rule_reproduces_the_reference_optimizer(tag):
    """LC.adamw_first_step, the rule the GPU tests hold the post-AdamW state to, against torch.optim.AdamW's step on the
    reference model (the fixture's post_stats, taken at wf = 1/30), and the dead parameters it left alone"""
    fx = load_fixture(tag)
    c, b = _fixture_batch(fx)
    p0 = fixture_params(fx)
    ref = LC.step_reference(c, b, p0, LC.WFS[1])
    assert bool(fx["dead_unchanged"].all()) and len(fx["dead_unchanged"]) == len(fx["param_names"]) - len(fx["live_names"])
    for j, n in enumerate(fx["live_names"]):
        post = LC.adamw_first_step(p0[n], ref["grads"][n], c["lr"], c["wd"], torch.float64)
        got, want = stats(post), fx["post_stats"][j]
        # an element whose true gradient is 0 (the key third of an in_proj_bias, fc_len.bias) holds rounding noise in the
        # reference's float32 and moves by up to lr there: those tensors are bounded by lr per element
        loose = n.endswith("in_proj_bias") or n == LC.ZERO_GRAD
        bound = c["lr"] * np.sqrt(post.numel()) if loose else 2e-5 * max(1.0, float(want[0]))
        assert abs(got[0] - want[0]) <= bound, (n, got[0], want[0])
        if not loose:
            assert np.abs(got[3:] - want[3:]).max() <= 2e-5, n


def test_loop_fixture_meets_the_tie_condition_at_every_step():
    """the float64 oracle runs the loop fixture's six training steps and three validation forwards: at each, every row's
    top-two gap, seg and l3, exceeds 4 x the logit tolerance at the parameters of that moment"""
    fx = load_fixture("l3_train_loop")
    c = LC.STEP_BY_TAG["l3_tiny"]
    assert fx["meta"]["epochs"] == LC.LOOP_EPOCHS
    train, val = LC.loop_data(c, fx["meta"]["seed"])
    margins, pfin = LC.loop_tie_margins(c, train, val, fixture_params(fx))
    assert len(margins) == 9 and [w for w, _ in margins][:3] == ["epoch 0 step 0", "epoch 0 step 2", "epoch 0 validation 0"]
    for what, mg in margins:
        assert mg > 1.0, (what, mg)
    # the oracle's final parameters against the reference run's (well-conditioned tensors)
    for j, n in enumerate(fx["live_names"]):
        if n.endswith("in_proj_bias") or n == LC.ZERO_GRAD:
            continue
        want = fx["post_stats"][j]
        assert abs(stats(pfin[n])[0] - want[0]) <= 5e-5 * max(1.0, float(want[0])), n


def test_tiny_fixture_holds_full_gradients():
    fx = load_fixture("l3_tiny")
    c, b = _fixture_batch(fx)
    ref = LC.step_reference(c, b, fixture_params(fx), LC.WFS[1])
    for n in fx["live_names"]:
        g = ref["grads"][n][0, :c["S"]] if n == "pos_embedding" else ref["grads"][n]
        if n == LC.ZERO_GRAD:                                       # (true gradient 0: the reference's float32 holds rounding noise)
            assert abs(float(fx["grad_wf1::" + n][0])) <= 64 * LC.EPS32 * float(ref["grads"]["fc.bias"].abs().max())
            continue
        assert LC.rel_err(g, fx["grad_wf1::" + n]) <= 5e-5, n


def test_admission_and_refusal_table():
    from r3d_amd import build
    build.build(verbose=False)
    from r3d_amd import engine_l3 as E
    ok = [(128, 8, 8, 49, 17), (16, 2, 8, 49, 7), (136, 4, 8, 49, 17), (1024, 8, 8, 256, 1023)]
    for row in ok:
        E.check_l3_shape(*row)
    bad = [((132, 8, 8, 49, 17), "hidden % 8"), ((120, 7, 8, 49, 17), "n_head"), ((2056, 8, 8, 49, 17), "2048"),
           ((1032, 8, 8, 49, 17), "128"), ((1024, 8, 16, 49, 17), "1024"), ((128, 8, 8, 257, 17), "256"),
           ((128, 8, 8, 0, 17), "query_num"), ((128, 8, 8, 49, 1024), "1023")]
    for row, pat in bad:
        with pytest.raises(ValueError, match=pat):
            E.check_l3_shape(*row)
    longest = E.max_clip_len(128, 8, 8, 2000, True)
    assert longest >= 256
    E.check_l3_batch(1, 1, 128, 8, 8, 2000, True)
    E.check_l3_batch(64, longest, 128, 8, 8, 2000, True)
    for (B, S, mp), pat in (((0, 4, 2000), "1 to 64"), ((65, 4, 2000), "1 to 64"), ((8, 0, 2000), "at least one frame"),
                            ((8, 33, 32), "max_pos_len"), ((8, longest + 1, 10 ** 6), "scores")):
        with pytest.raises(ValueError, match=pat):
            E.check_l3_batch(B, S, 128, 8, 8, mp, True)
    from r3d_amd import train_unsupervised as TU
    import argparse
    for kw in (dict(seg=False), dict(anticipate=False), dict(erank_weight=0.5), dict(measure_rank=True), dict(erank_report=True),
               dict(supcon_weight=0.1)):
        with pytest.raises(ValueError):
            TU.check_args(argparse.Namespace(**dict(dict(seg=True, anticipate=True), **kw)))
    TU.check_args(argparse.Namespace(seg=True, anticipate=True))
    assert [TU.get_warmup_factor(e, 0, 30, 60) for e in (0, 1, 2, 30, 45, 60, 99)] == [0.0, 1 / 30, 2 / 30, 1.0, 0.5, 0.0, 0.0]


def test_host_helpers_restate_the_reference_functions():
    from r3d_amd import train_unsupervised as TU
    lab = torch.tensor([[1, 2, 9, 9], [9, 9, 9, 9], [3, 9, 4, 5]])
    assert TU.get_last_non_padding_labels(lab, 9).tolist() == [2, 9, 5]
    pred = torch.tensor([[0.1, 0.9], [0.8, 0.2], [0.3, 0.7]])
    assert TU.weighted_accuracy(pred, torch.tensor([1, 1, 9]), 9, torch.tensor([0])) == 0.5
    assert TU.weighted_accuracy(pred, torch.tensor([9, 9, 9]), 9, torch.tensor([0])) == 0


DROPIN = r'''
import argparse, json, torch
from opts import parser                                              # main_darai.py:12
from pl_bolts.optimizers.lr_scheduler import LinearWarmupCosineAnnealingLR   # :13
from loss.spc import SupConLoss                                      # :15
from utils import read_mapping_dict                                  # :16
import model.futr_proposed, model.futr_safuser_tokenfusion, model.futr_safuser_batchnormalization, model.futr_unsupervised_depth
from model.futr_unsupervised_temp3 import FUTR                       # :36
from train_proposed_depth import train as _t39                       # :39
from train_unsupervised import train                                 # :40
import train_unsupervised as TU, r3d_amd.train_unsupervised as R, r3d_amd.model.futr_unsupervised_temp3 as RM
assert train is R.train and FUTR is RM.FUTR
for n in ("validate", "get_warmup_factor", "get_cluster_intervals", "weighted_accuracy", "get_last_non_padding_labels"):
    assert getattr(TU, n) is getattr(R, n), n
import r3d_amd.loss.temporal as T
assert TU.get_cluster_intervals is T.get_cluster_intervals
a = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
m = FUTR(int(__import__("sys").argv[2]), int(__import__("sys").argv[1]), 9, torch.device("cpu"), a, n_query=8, n_head=2,
         num_encoder_layers=2, num_decoder_layers=1, query_num=49)
print(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()]))
'''


def test_dropin_imports_resolve_and_state_dict_matches_the_reference(tmp_path):
    fx = load_fixture("l3_tiny")
    m = fx["meta"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", DROPIN, str(m["H"]), str(m["n_class"])], env=env, capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().split("\n")[-1])
    keys = json.loads(str(fx["state_keys"]))
    shapes = json.loads(str(fx["state_shapes"]))
    assert [k for k, _ in got] == keys                                  # the reference's keys, in its order (strict=True loads)
    assert [s for _, s in got] == shapes
    assert [k for k in keys if "pos_table" not in k] == fx["param_names"]
