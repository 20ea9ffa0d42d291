"""The three-modality (RGB + depth + gaze) model without a GPU: its parameter tree against the two-modality model's, the float64
restatement (tests/m3_oracle.py) against autograd, the case table's coverage, the selection margins of the validation cases,
every refusal of the engine's admission checks, the loop's batch arity and --gaze_dim."""
import argparse

import pytest
import torch

from r3d_amd import engine_m3  # noqa: F401  (the feature under test: without it nothing here is collected)
from r3d_amd.engine_m3 import check_m3_args, check_m3_batch, check_m3_shape
from tests import m3_cases as MC
from tests import m3_oracle as MO


def _args(**kw):
    return MC.make_args(None, **kw)


def _two_and_three(seed, H=64, heads=4, K=17, pixels=256, gaze_dim=2):
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR as F2
    from r3d_amd.model.futr_safuser_tokenfusion3 import FUTR as F3
    kw = dict(n_query=8, n_head=heads, num_encoder_layers=1, num_decoder_layers=1, query_num=49, depth_pixels=pixels)
    torch.manual_seed(seed)
    m2 = F2(K, H, K + 1, torch.device("cpu"), _args(), **kw)
    torch.manual_seed(seed)
    m3 = F3(K, H, K + 1, torch.device("cpu"), _args(), gaze_dim=gaze_dim, **kw)
    return m2, m3


# ---------------------------------------------------------------------------------------------------------------------
# the parameter tree
# ---------------------------------------------------------------------------------------------------------------------
def test_state_dict_is_the_two_modality_models_plus_four():
    m2, m3 = _two_and_three(3, gaze_dim=5)
    s2, s3 = m2.state_dict(), m3.state_dict()
    extra = {"gaze_projection.weight": (64, 5), "gaze_projection.bias": (64,), "gaze_layernorm.weight": (64,),
             "gaze_layernorm.bias": (64,)}
    assert set(s3) == set(s2) | set(extra)
    assert list(s3)[:len(s2)] == list(s2)                       # (the two-modality model's keys first, in its order)
    for k, v in s2.items():
        assert tuple(s3[k].shape) == tuple(v.shape), k
    for k, shp in extra.items():
        assert tuple(s3[k].shape) == shp, k
    assert tuple(MO.GAZE_KEYS) == tuple(extra)


def test_same_seed_gives_the_two_modality_models_initial_values():
    m2, m3 = _two_and_three(7)
    s3 = m3.state_dict()
    for k, v in m2.state_dict().items():
        assert torch.equal(s3[k], v), k
    w = s3["gaze_projection.weight"]
    bound = (6.0 / (w.shape[0] + w.shape[1])) ** 0.5            # xavier_uniform_
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.5 * bound
    assert torch.equal(s3["gaze_layernorm.weight"], torch.ones(64)) and torch.equal(s3["gaze_layernorm.bias"], torch.zeros(64))


def test_a_two_modality_checkpoint_loads_with_exactly_the_gaze_keys_missing():
    m2, m3 = _two_and_three(9)
    res = m3.load_state_dict(m2.state_dict(), strict=False)
    assert sorted(res.missing_keys) == sorted(MO.GAZE_KEYS) and not res.unexpected_keys


def test_live_and_dead_parameters():
    from r3d_amd.engine import is_live
    _, m3 = _two_and_three(1)
    live = lambda n: is_live(n) or n.startswith(engine_m3.M3_LIVE_EXTRA)     # noqa: E731
    names = [n for n, _ in m3.named_parameters()]
    assert [n for n in names if n.startswith(("gaze_projection.", "gaze_layernorm."))] == list(MO.GAZE_KEYS)
    assert all(live(n) for n in MO.GAZE_KEYS)
    assert sorted(n for n in names if live(n)) == sorted(n for n in names if n.startswith(MO.LIVE_PREFIXES))
    dead = [n for n in names if not live(n)]
    assert dead and all(n.startswith(("transformer.encoder.", "l3_attention.", "query_attention.", "fc_l3.",
                                      "fuser.modality_token", "fuser.projection.", "fuser.fusion_conv.")) for n in dead)


def test_the_model_needs_a_gpu_and_a_gaze_track():
    _, m3 = _two_and_three(1)
    with pytest.raises(RuntimeError, match="MI355X"):
        m3((torch.zeros(1, 2, 2048), torch.zeros(1, 2, dtype=torch.long)), torch.zeros(1, 2, 256), torch.zeros(1, 2, 2))
    with pytest.raises(TypeError):
        m3((torch.zeros(1, 2, 2048), None), torch.zeros(1, 2, 256))          # forward(inputs, depth_features, gaze, ...)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_zero_gaze_with_zero_beta_gives_a_zero_gaze_row():
    c = MC.STEP_BY_TAG["m3_tiny"]
    _, p0 = MC.build_model(c)
    p = {n: v.double() for n, v in p0.items()}
    p["gaze_layernorm.bias"] = torch.zeros_like(p["gaze_layernorm.bias"])
    p["gaze_projection.bias"] = torch.full_like(p["gaze_projection.bias"], 0.25)       # a constant row: x - mean = 0 exactly
    gz = MO.gaze_embed(p, torch.zeros(2, 5, c["gaze_dim"], dtype=torch.float64))
    assert float(gz.abs().max()) == 0.0
    b = MC.batch(c)
    with torch.no_grad():
        _, aux = MO.forward(p, (b[0], b[2]), b[1], torch.zeros_like(b[5]), "val", MC.pad_idx(c), c["n_head"], c["n_dec"])
    assert float(aux["gaze_embed"].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["H8_N5", "H72_N67", "H136_N5", "saturated", "saturated_H8"])
def test_oracle_seam_backward_equals_float64_autograd(name):
    case = MC.SEAM_BY_NAME[name]
    d = MC._cast(MC.seam_inputs(name), torch.float64)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("rgb_src", "dep_src", "w_g", "b_g", "lnd_g", "lnd_b", "lng_g",
                                                              "lng_b", "ln1_g", "ln1_b")}
    if case["ns_r"] == 0:
        pre = leaves["rgb_src"]                                  # the finished embedding stands for relu(pre): gate by it
        dd = dict(d, **leaves)
        dd["rgb_src"] = torch.relu(pre + 0)                      # (inputs are already >= 0: relu is the identity's gate)
    else:
        dd = dict(d, **leaves)
    fw = MC.seam_fwd_of(dd, case, torch.float64)
    x0 = fw["x0"]
    extra = d["add1"] if d["add2"] is None else d["add1"] + d["add2"]
    ((fw["h1"] * d["d_h1"]).sum() + (x0 * extra).sum()).backward()
    fw0 = MC.seam_fwd_of(d, case, torch.float64)
    bw = MC.seam_bwd_of(d, fw0, torch.float64)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))      # noqa: E731
    if case["ns_r"] > 0:
        for s in range(case["ns_r"]):
            assert close(bw["d_rgb_pre"], leaves["rgb_src"].grad[s])
    else:
        assert close(bw["d_rgb_pre"], leaves["rgb_src"].grad)
    for s in range(case["ns_d"]):
        assert close(bw["d_dep_pre"], leaves["dep_src"].grad[s])
    assert close(bw["d_w_g"], leaves["w_g"].grad) and close(bw["d_b_g"], leaves["b_g"].grad)
    for tag, g, b in (("n1", "ln1_g", "ln1_b"), ("dep", "lnd_g", "lnd_b"), ("gz", "lng_g", "lng_b")):
        s = bw["p_" + tag].sum(dim=0)
        assert close(s[0], leaves[g].grad) and close(s[1], leaves[b].grad), tag


def test_oracle_step_uses_the_pinned_pieces_and_has_the_gaze_gradients():
    c = MC.STEP_BY_TAG["m3_odd"]
    _, p0 = MC.build_model(c)
    ref = MC.step_reference(c, p0)
    assert sorted(ref["live"]) == sorted(n for n in p0 if n.startswith(MO.LIVE_PREFIXES))
    for n in MO.GAZE_KEYS:
        assert float(ref["grads"][n].abs().max()) > 0.0
    for n, g in ref["grads"].items():
        assert (g is None) == (not n.startswith(MO.LIVE_PREFIXES)), n
    # with the gaze stream removed the fuser piece is the reference-pinned two-modality fuser (tests/test_fuser3_cpu.py ties
    # fuser3_oracle to oracle.cm_fuser); here: the step's fused tokens are that piece's on the step's own embeddings
    from tests import fuser3_oracle as F3
    aux = ref["aux"]
    p64 = {n: v.double() for n, v in p0.items()}
    fused, _ = F3.cm_fuser3(p64, [aux["rgb_embed"].detach(), aux["depth_embed"].detach(), aux["gaze_embed"].detach()], "train",
                            c["n_head"])
    assert torch.equal(fused, aux["fused"].detach())
    # Q and K rows of the fuser's qkv weight are live with a NON-zero gradient (two logits per softmax), unlike the two-token swap
    gq = ref["grads"]["fuser.blocks.0.attn.qkv.weight"]
    assert float(gq[:c["H"]].abs().max()) > 0.0 and float(gq[c["H"]:2 * c["H"]].abs().max()) > 0.0


def test_the_all_padding_clip_is_nan_in_the_oracle_and_nowhere_else():
    c = MC.STEP_BY_TAG["m3_tiny"]
    _, p0 = MC.build_model(c)
    ref = MC.step_reference(c, p0)
    b = ref["batch"]
    assert bool((b[2][1] == MC.pad_idx(c)).all()) and int((b[2][0] == MC.pad_idx(c)).sum()) == 2
    out = ref["out"]
    assert bool(torch.isnan(out["action"][1]).all()) and bool(torch.isfinite(out["action"][0]).all())
    assert bool(torch.isfinite(out["seg"]).all())
    assert bool(torch.isfinite(ref["res"]["loss_seg"])) and bool(torch.isnan(ref["res"]["loss_action"]))


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def test_every_factor_value_meets_every_width_instance():
    for epl in (2, 8, 16):
        rows = [c for c in MC.SEAM if MC.epl_of(c["H"]) == epl]
        assert {c["N"] for c in rows} >= set(MC.FRAMES)
        assert {c["G"] for c in rows} == set(MC.GAZES), epl
        assert {c["mask"] for c in rows} == set(MC.MASKS), epl
        assert {c["keep"] for c in rows} == {True, False}, epl
        assert {c["ns_r"] for c in rows} == {0, 1, 3}, epl
        assert {c["ns_d"] for c in rows} == {1, 4}, epl
        assert {c["add2"] for c in rows} == {True, False}, epl
        assert any(c["H"] % 64 == 0 for c in rows) and any(c["H"] % 64 for c in rows), epl
    assert {(c["H"], c["N"]) for c in MC.SEAM} >= {(H, N) for H in MC.WIDTHS for N in MC.FRAMES}
    assert any(c["N"] > 1024 for c in MC.SEAM)                   # the forward's frame loop takes a second turn


def test_seam_cases_keep_their_relus_clear_of_zero_and_saturate_where_they_say():
    for c in MC.SEAM:
        d = MC.seam_inputs(c["name"])
        fw = MC.seam_reference(c["name"])["fw"]
        assert MO.relu_margin(fw, d["lnd_g"].double(), d["lnd_b"].double(), d["lng_g"].double(), d["lng_b"].double(),
                              c["ns_r"]) >= MC.RELU_GUARD, c["name"]
        if c["flavour"] == "saturated":
            eps_rstd = 1.0 / MO.LN_EPS ** 0.5
            assert float(fw["rstd_d"][1]) == pytest.approx(eps_rstd, rel=1e-12)      # variance exactly 0
            assert float(fw["rstd_g"][1]) == pytest.approx(eps_rstd, rel=1e-12)
            assert float(fw["r1"][3]) == pytest.approx(eps_rstd, rel=1e-12) and float(fw["x0"][3].abs().max()) == 0.0
        tol = MC.seam_reference(c["name"])["tol"]
        assert all(0.0 <= v < 1e-4 for v in tol.values()), (c["name"], tol)


@pytest.mark.parametrize("tag", MC.VAL_TAGS)
def test_validation_cases_select_away_from_ties(tag):
    c = MC.STEP_BY_TAG[tag]
    _, p0 = MC.build_model(c)
    ref = MC.validation_reference(c, p0)
    gap = MC.selection_gap(ref, c["H"])
    print(tag, "selection gap / (4 x score tolerance):", gap)
    assert gap > 1.0, (tag, gap)


# ---------------------------------------------------------------------------------------------------------------------
# admission
# ---------------------------------------------------------------------------------------------------------------------
def test_check_m3_shape_refusals():
    check_m3_shape(128, 8, 8, 17, 2)
    check_m3_shape(1024, 8, 8, 1023, 8)
    check_m3_shape(8, 8, 8, 1, 1)
    for kw, pat in ((dict(H=132), "hidden % 8"), (dict(H=136, n_head=16), "n_head"), (dict(H=1032), "1024"),
                    (dict(H=1024, n_head=4), "head width 256"), (dict(H=1024, n_head=8, n_query=9), "n_query"),
                    (dict(gaze_dim=0), "gaze_dim"), (dict(gaze_dim=9), "gaze_dim"), (dict(n_class=1024), "n_class"),
                    (dict(n_class=0), "n_class"), (dict(erank_route="wide"), "erank_route")):
        a = dict(H=128, n_head=8, n_query=8, n_class=17, gaze_dim=2)
        a.update(kw)
        with pytest.raises(ValueError, match=pat):
            check_m3_shape(**a)


def test_check_m3_batch_refusals():
    check_m3_batch(8, 16, 128, 8, 8, 2000, True)
    check_m3_batch(16, 16, 1024, 8, 8, 2000, True, erank_weight=0.05)         # configuration five's per-GPU shape
    with pytest.raises(ValueError, match="at least one"):
        check_m3_batch(0, 16, 128, 8, 8, 2000, True)
    with pytest.raises(ValueError, match="max_pos_len"):
        check_m3_batch(8, 2001, 128, 8, 8, 2000, True)
    with pytest.raises(ValueError, match="2\\^31"):
        check_m3_batch(512, 1366, 1024, 8, 8, 2000, False)
    assert 3 * 512 * 1366 * 1024 >= 2 ** 31 > 3 * 512 * 1365 * 1024
    from r3d_amd.engine import max_clip_len
    longest = max_clip_len(1024, 8, 8, 100000, True)
    with pytest.raises(ValueError, match="cross-attention core"):
        check_m3_batch(1, longest + 1, 1024, 8, 8, 100000, True)
    check_m3_batch(1, longest, 1024, 8, 8, 100000, True)
    with pytest.raises(ValueError, match="rank penalty"):                     # past the blocked Jacobi's LDS on either side
        check_m3_batch(100, 900, 1024, 8, 8, 2000, True, erank_weight=0.1)
    check_m3_batch(100, 900, 1024, 8, 8, 2000, True, erank_weight=0.1, erank_route="tall")
    check_m3_batch(100, 900, 1024, 8, 8, 2000, False, erank_weight=0.1)        # (a forward without gradients runs no penalty)
    with pytest.raises(ValueError, match="rank penalty"):
        check_m3_batch(2, 4, 128, 8, 8, 2000, True, erank_weight=0.1, erank_route="tall")      # N < H


def test_check_m3_args_refusals():
    check_m3_args()
    for kw, pat in ((dict(seg=False), "seg"), (dict(anticipate=False), "anticipate"), (dict(input_type="gt"), "gt"),
                    (dict(parallel=True), "one GPU"), (dict(pixel_shard=True), "pixel_shard")):
        with pytest.raises(ValueError, match=pat):
            check_m3_args(**kw)


# ---------------------------------------------------------------------------------------------------------------------
# the loop's batch arity, the refusals that need no GPU, --gaze_dim
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_arity_errors():
    from r3d_amd.train_proposed_depth import _is_m3, _to_dev
    m2, m3 = _two_and_three(2)
    assert _is_m3(m3) and not _is_m3(m2)
    c = MC.STEP_BY_TAG["m3_tiny"]
    b = MC.batch(c)
    six = _to_dev(b, "cpu", gaze=True)
    assert len(six) == 6 and six[5].dtype == torch.float32 and torch.equal(six[5], b[5])
    five = _to_dev(b[:5], "cpu")
    assert len(five) == 5 and all(torch.equal(x, y) for x, y in zip(five, six[:5]))       # today's tuple, unchanged
    with pytest.raises(ValueError, match="6-element"):
        _to_dev(b[:5], "cpu", gaze=True)
    with pytest.raises(ValueError, match="only the three-modality model"):
        _to_dev(b, "cpu", gaze=False)


def test_predict_and_supcon_refuse_before_anything_runs():
    from r3d_amd.predict import predict, predict_clip
    from r3d_amd.train_proposed_depth import train
    _, m3 = _two_and_three(2)
    with pytest.raises(ValueError, match="gaze"):
        predict_clip(m3, torch.zeros(4, 2048), torch.zeros(4, 256), 8)
    with pytest.raises(ValueError, match="gaze"):
        predict(torch.nn.DataParallel(m3), [], argparse.Namespace(dataset="darai", sample_rate=1), 0.3, 17, {}, "cpu")
    with pytest.raises(ValueError, match="supcon_weight"):
        train(argparse.Namespace(supcon_weight=0.5), m3, [], None, None, None, ".", 18, "cpu", [], 0)
    with pytest.raises(ValueError, match="pixel_shard"):
        train(argparse.Namespace(supcon_weight=0.0, pixel_shard=True), m3, [], None, None, None, ".", 18, "cpu", [], 0)


def test_report_line_names_four_representations():
    from r3d_amd.rankstream import report_line
    r = lambda e: dict(erank=e, rows=40, sigma=None)     # noqa: E731
    assert report_line(dict(rgb=r(1.0), depth=r(2.0), gaze=r(3.0), fused=r(4.0))) == \
        "Effective rank over 40 frames: rgb 1.000, depth 2.000, gaze 3.000, fused 4.000"
    assert report_line(dict(rgb=r(1.0), depth=r(2.0), fused=r(4.0))) == \
        "Effective rank over 40 frames: rgb 1.000, depth 2.000, fused 4.000"


def test_gaze_dim_parses():
    from r3d_amd.opts import parser
    assert parser.parse_args([]).gaze_dim == 2
    assert parser.parse_args(["--gaze_dim", "5"]).gaze_dim == 5
    with pytest.raises(SystemExit):
        parser.parse_args(["--gaze_dim", "two"])


def test_seam_pays_follows_the_measurement_file():
    """seam_pays is a rule read off profiles/m3_step_speed.json: True exactly where the seam was measured ahead (forward +
    backward, replayed as a graph); every shape that was not timed keeps the composed route"""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "m3_step_speed.json")
    assert not engine_m3.seam_pays(3, 8) and not engine_m3.seam_pays(77, 264)          # never timed
    assert os.path.exists(path), "profiles/m3_step_speed.json: written by tools/m3_step_speed.py"
    rec = json.load(open(path))
    for row in rec["seam_vs_composed"]:
        N, H = row["B"] * row["S"], row["H"]
        ahead = row["seam_fwd_bwd_us"] < row["composed_fwd_bwd_us"]
        assert engine_m3.seam_pays(N, H) == ahead, row
