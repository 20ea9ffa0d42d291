"""The three-modality (RGB + depth + gaze) model on the GPU against the float64 restatement (tests/m3_oracle.py) over
tests/m3_cases.py: the two seam entry points of csrc/fuse3_seam.hip on their own, the engine's seam route against its composed
route, whole training steps, validation forwards with exact selected indices, the rank penalty against float64 autograd through
svdvals, dropout (keep rates, eager against graphed, the offset) and the loop.  Needs an MI355X.  Tolerances: tests/m3_cases.py
(8 x the float32 restatement's error per case and quantity); the penalty's bounds are tests/test_erank_tall_gpu.py's and
test_effective_rank_penalty_baseline_shapes's."""
import argparse
import contextlib
import io
import re

import pytest
import torch

from r3d_amd import engine_m3  # noqa: F401  (the feature under test: without it nothing here is collected)
from tests import m3_cases as MC
from tests import m3_oracle as MO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# the two seam entry points on their own
# ---------------------------------------------------------------------------------------------------------------------
def _run_seam(ops, case, d):
    """(forward outputs, backward outputs) of the case through the C ABI; every output buffer starts as NaN"""
    N, H, G, ns_r = case["N"], case["H"], case["G"], case["ns_r"]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)     # noqa: E731
    g = {k: _dev(v) for k, v in d.items()}
    dsc = MC.DROP_SCALE if d["keep"] is not None else 1.0
    f = dict(rgb=nan(N, H) if ns_r > 0 else g["rgb_src"], dep_pre=nan(N, H), mean_d=nan(N), rstd_d=nan(N), dep=nan(N, H),
             gz_pre=nan(N, H), mean_g=nan(N), rstd_g=nan(N), gz=nan(N, H), x0=nan(3 * N, H), h1=nan(3 * N, H), m1=nan(3 * N),
             r1=nan(3 * N))
    ops.embed_fuse3_fwd(g["rgb_src"], ns_r, g["bias_r"], g["dep_src"], case["ns_d"], g["bias_d"], g["lnd_g"], g["lnd_b"],
                        g["gaze"], g["w_g"], g["b_g"], g["lng_g"], g["lng_b"], g["mask"], g["keep"], dsc, g["ln1_g"], g["ln1_b"],
                        f["rgb"], f["dep_pre"], f["mean_d"], f["rstd_d"], f["dep"], f["gz_pre"], f["mean_g"], f["rstd_g"], f["gz"],
                        f["x0"], f["h1"], f["m1"], f["r1"])
    b = dict(d_rgb_pre=nan(N, H), d_dep_pre=nan(N, H), d_gz_pre=nan(N, H), p_n1=nan(N, 2, H), p_dep=nan(N, 2, H),
             p_gz=nan(N, 2, H))
    ops.embed_fuse3_bwd(g["d_h1"], f["x0"], f["m1"], f["r1"], g["ln1_g"], g["add1"], g["add2"], g["keep"], dsc, g["mask"],
                        f["rgb"], f["dep_pre"], f["mean_d"], f["rstd_d"], g["lnd_g"], g["lnd_b"], f["gz_pre"], f["mean_g"],
                        f["rstd_g"], g["lng_g"], g["lng_b"], b["d_rgb_pre"], b["d_dep_pre"], b["d_gz_pre"], b["p_n1"],
                        b["p_dep"], b["p_gz"])
    # the partials in the layout r3d_layernorm_bwd_finalize_batched reduces (rows = -N), and the gaze projection's gradient
    # as the engine forms it: the existing GEMM with its column-sum epilogue, output gaze_dim wide
    sums = {k: nan(2, H) for k in ("n1", "dep", "gz")}
    ops.LnFinalizeGroup([(b["p_" + k], -N, H, sums[k][0], sums[k][1]) for k in ("n1", "dep", "gz")]).launch()
    b["d_w_g"], b["d_b_g"] = nan(H, G), nan(H)
    from r3d_amd._lib import GEMM_TN
    ops.gemm(GEMM_TN, b["d_gz_pre"], g["gaze"], b["d_w_g"], bias_grad=b["d_b_g"], ws=ops.GemmWorkspace(DEV))
    for k in sums:
        b["dg_" + k] = sums[k]
    torch.cuda.synchronize()
    return f, b, g, dsc


def _quantities(f, b):
    q = {k: f[k] for k in ("rgb", "dep_pre", "dep", "gz_pre", "gz", "x0", "h1")}
    q["mean"] = torch.cat([f["mean_d"], f["mean_g"], f["m1"]])
    q["rstd"] = torch.cat([f["rstd_d"], f["rstd_g"], f["r1"]])
    q.update({k: b[k] for k in MC.BWD_KEYS})
    return q


@pytest.mark.parametrize("name", [c["name"] for c in MC.SEAM])
def test_seam_matches_float64(ops, name):
    case = MC.SEAM_BY_NAME[name]
    d = MC.seam_inputs(name)
    ref = MC.seam_reference(name)
    f, b, g, dsc = _run_seam(ops, case, d)
    q = _quantities(f, b)
    fails = []
    for k in MC.FWD_KEYS + MC.BWD_KEYS:
        assert not torch.isnan(q[k]).any(), (name, k, "an element was not written")
        err = MC.rel_err(q[k], ref["q"][k])
        print(f"{name}/{k}: err {err:.3e} tol {ref['tol'][k]:.3e}")
        if err > ref["tol"][k]:
            fails.append((k, err, ref["tol"][k]))
    assert not fails, (name, fails)
    # x0 is the existing exchange launch on the seam's own finished embeddings, bit for bit
    x0 = torch.full_like(f["x0"], float("nan"))
    ops.token_exchange3_fwd(f["rgb"], f["dep"], f["gz"], g["mask"], x0, drop_mask=g["keep"], drop_scale=dsc)
    assert torch.equal(x0, f["x0"])
    # two calls give the same bits
    f2, b2, _, _ = _run_seam(ops, case, d)
    for k in f:
        assert torch.equal(f[k], f2[k]), (name, k)
    for k in b:
        assert torch.equal(b[k], b2[k]), (name, k)


def test_seam_refusals(ops):
    lib = ops._lib.load()
    x = torch.full((4, 8), 3.0, device=DEV)
    p = x.data_ptr()
    base = [p, 0, None, p, 1, None, p, p, p, p, p, p, p]
    tail = [p, None, 1.0, p, p] + [p] * 13
    assert lib.r3d_embed_fuse3_fwd(*base, 9, *tail, 1, 8, None) == -1            # gaze_dim past 8
    assert lib.r3d_embed_fuse3_fwd(*base, 0, *tail, 1, 8, None) == -1
    assert lib.r3d_embed_fuse3_fwd(*base, 2, *tail, 1, 1032, None) == -1         # hidden past the seam's registers
    assert lib.r3d_embed_fuse3_fwd(*base, 2, *tail, 0, 8, None) == -1            # no frames
    b2 = list(base)
    b2[1] = 2                                                                     # RGB slabs without their bias
    assert lib.r3d_embed_fuse3_fwd(*b2, 2, *tail, 1, 8, None) == -1
    assert lib.r3d_embed_fuse3_bwd(*([p] * 8), 1.0, *([p] * 18), 1, 1032, None) == -1
    assert lib.r3d_embed_fuse3_bwd(*([p] * 8), 1.0, *([p] * 17), None, 1, 8, None) == -1
    torch.cuda.synchronize()
    assert bool((x == 3.0).all())
    with pytest.raises(ValueError, match="gaze_dim"):
        v, r = torch.zeros(8, device=DEV), torch.zeros(2, 8, device=DEV)
        ops.embed_fuse3_fwd(r, 0, None, r, 1, None, v, v, torch.zeros(2, 9, device=DEV), torch.zeros(8, 9, device=DEV), v, v, v,
                            torch.zeros(3, 8, device=DEV), None, 1.0, v, v, r, r, v[:2], v[:2], r, r, v[:2], v[:2], r,
                            torch.zeros(6, 8, device=DEV), torch.zeros(6, 8, device=DEV), v[:6], v[:6])


# ---------------------------------------------------------------------------------------------------------------------
# the engine: helpers
# ---------------------------------------------------------------------------------------------------------------------
def _engine(c, dropout=False, use_seam=None):
    model, p0 = MC.build_model(c, "cuda", dropout=dropout)
    eng = model.engine()
    eng.use_seam = use_seam
    return model, eng, p0


def _fwd_bwd(eng, d, training=False):
    out = eng.forward(d[0], d[1], d[2], "train", training=training, gaze=d[5])
    loss, counts = eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()
    return out, loss, counts


def _same_nan(got, ref, what):
    got, ref = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach()
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), (what, "NaN where the reference is finite, or the reverse", int(gn.sum()), int(rn.sum()))


def _undefined(ref, what, skipped):
    """The all-padding clip (m3_tiny only; m3_ragged is the same shape with every quantity finite and compared): every key of its cross-attention is masked, and the softmax over an empty set is NaN in the
    reference's arithmetic and in the attention kernels alike (compared: the outputs' and the losses' NaN patterns are equal).
    The total loss is then NaN, so its gradient is not a number the two sides can be compared on: float64 autograd and the
    float32 kernels spread the NaN differently through operations that select (masked_fill's backward writes 0 over a NaN,
    torch's relu passes one on; the GEMM epilogues' fmaxf(x, 0) and the attention backward do the opposite).  A gradient or a
    stepped parameter is compared where the reference holds no NaN at all."""
    if bool(torch.isnan(torch.as_tensor(ref)).any()):
        skipped.append(what)
        return True
    return False


def _rel(got, ref, tol, what, fails):
    _same_nan(got, ref, what)
    err = MC.rel_err(got, ref)
    print(f"  {what}: err {err:.3e} tol {tol:.3e}")
    if err > tol:
        fails.append((what, err, tol))


# ---------------------------------------------------------------------------------------------------------------------
# seam route against composed route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,H", MC.SEAM_VS_COMPOSED)
def test_seam_route_against_composed_route(B, S, H):
    c = MC._step(f"sc_{H}", B, S, H, 8, 17, 1, 256, 40 + H)
    ref = MC.step_reference(c, MC.build_model(c)[1])
    d = [t.cuda() for t in ref["batch"]]
    grads = {}
    for seam in (True, False):
        model, eng, _ = _engine(c, use_seam=seam)
        model.eval()
        out, loss, _ = _fwd_bwd(eng, d)
        assert eng.last["seam"] is seam
        grads[seam] = (eng.arena.grads.clone(), {k: v.clone() for k, v in out.items()}, loss.clone(), eng)
    fails = []
    for k in ("action", "duration", "seg"):
        _rel(grads[True][1][k], grads[False][1][k].cpu(), 2 * ref["tol"][k], f"seam vs composed {k}", fails)
    for n in ref["live"]:
        gs, gc = (grads[s][3].arena.g(n) for s in (True, False))
        if n == "pos_embedding":
            gs, gc = gs[:, :S], gc[:, :S]
        # both routes are float32 evaluations of the same arithmetic: each within the case's tolerance of float64
        if n == MC.ZERO_GRAD:           # (a true gradient of 0: rounding noise on both sides, held to its absolute bound)
            assert float((gs - gc).abs().max()) <= 2 * ref["tol_abs"][n], n
            continue
        _rel(gs, gc.cpu(), 2 * ref["tol"]["grad::" + n], f"seam vs composed grad {n}", fails)
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------
# whole training steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [True, False], ids=["seam", "composed"])
@pytest.mark.parametrize("tag", [c["tag"] for c in MC.STEP_CASES])
def test_step_matches_float64(tag, seam):
    c = MC.STEP_BY_TAG[tag]
    model, eng, p0 = _engine(c, use_seam=seam)
    model.eval()
    ref = MC.step_reference(c, p0)
    tol, res = ref["tol"], ref["res"]
    d = [t.cuda() for t in ref["batch"]]
    B, S = c["B"], c["S"]
    out, loss, counts = _fwd_bwd(eng, d)
    fails, skipped = [], []
    nan_case = c["ragged"] == "all"
    if not nan_case:        # (every other case, the ragged one included: nothing of the step is NaN, so nothing is left out)
        assert all(bool(torch.isfinite(g).all()) for g in ref["grads"].values() if g is not None)
        assert all(bool(torch.isfinite(v).all()) for v in ref["out"].values())
    for k in ("action", "duration", "seg"):
        _rel(out[k], ref["out"][k], tol[k], f"{tag}/{k}", fails)
    for i, k in enumerate(MC.LOSS_KEYS):
        _rel(loss[i], res[k], tol[k], f"{tag}/{k}", fails)
    cnt = counts.cpu().tolist()
    want = [res["seg_correct"], res["seg_total"], res["act_correct"], res["act_total"]]
    # (the arg-max of a NaN row -- the all-padding clip -- is no class: its "correct" count is compared on the finite cases)
    assert cnt[:2] == want[:2] and cnt[3] == want[3] and (nan_case or cnt[2] == want[2]), (cnt, want)
    live = ref["live"]
    assert sorted(live) == sorted(n for n, _ in model.named_parameters() if eng.arena.is_live(n))
    for n in live:
        g, gref = eng.arena.g(n), ref["grads"][n]
        if n == "pos_embedding":
            assert float(g[:, S:].abs().max()) == 0.0
            g, gref = g[:, :S], gref[:, :S]
        if not _undefined(gref, f"grad {n}", skipped):
            _rel(g, gref, tol["grad::" + n], f"{tag}/grad {n}", fails)
    assert not fails, fails
    # ---- one AdamW step: live parameters against torch's rule on the float64 gradients; dead parameters unchanged
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    eng.adamw(c["lr"], c["wd"])
    torch.cuda.synchronize()
    for n in live:
        p = eng.arena.p(n)
        if n == "pos_embedding":
            p = p[:, :S]
        got, want_p = p.detach().cpu().double(), ref["post"][n]
        if _undefined(want_p, f"post {n}", skipped):
            continue
        over = (got - want_p).abs() - tol["post::" + n]
        assert float(over.max()) <= 0.0, (n, float(over.max()))
    for n, p in model.named_parameters():
        if not eng.arena.is_live(n):
            assert torch.equal(p.detach(), before[n]), f"dead parameter {n} moved"
    assert int(eng.step_t.item()) == 1
    assert nan_case or not skipped, skipped
    if skipped:
        print(f"  {tag}: {len(skipped)} gradients / stepped parameters whose reference is NaN (a NaN loss) were not compared")


@pytest.mark.parametrize("tag", MC.VAL_TAGS)
def test_validation_forward_selects_the_oracles_channels(tag):
    c = MC.STEP_BY_TAG[tag]
    model, eng, p0 = _engine(c)
    model.eval()
    ref = MC.validation_reference(c, p0)
    assert MC.selection_gap(ref, c["H"]) > 1.0
    b = ref["batch"]
    with torch.no_grad():
        out = model((b[0], b[2]), b[1], b[5], mode="val")
    torch.cuda.synchronize()
    idx = eng.last_idx.cpu()
    for m in range(3):
        assert torch.equal(torch.sort(idx[m])[0], ref["aux"]["idx"][m]), (tag, m)
    fails = []
    for k in ("action", "duration", "seg"):
        _rel(out[k], ref["out"][k], ref["tol"][k], f"{tag}/val {k}", fails)
    assert not fails, fails
    assert eng.last["seam"] is False                       # (validation scores need the embeddings first: composed launches)


# ---------------------------------------------------------------------------------------------------------------------
# the rank penalty
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,H,route", [(8, 16, 128, "jacobi"), (4, 8, 512, "jacobi"), (4, 10, 1024, "jacobi"),
                                         (8, 20, 128, "tall")])
def test_rank_penalty_against_float64_autograd(ops, B, S, H, route):
    lam = 0.05
    c = MC._step(f"er_{B}_{S}_{H}", B, S, H, 8, 17, 1, 256, 60 + S)
    model, eng, p0 = _engine(c)
    model.eval()
    eng.erank_weight, eng.erank_route = lam, route
    b = MC.batch(c)
    out, res, grads, aux = MO.step(p0, b, MC.pad_idx(c), c["n_head"], c["n_dec"], torch.float64, erank_weight=lam)
    from oracle import futr_oracle as O
    er = O.effective_rank(aux["fused"].detach().reshape(-1, H))
    d = [t.cuda() for t in b]
    _fwd_bwd(eng, d)
    w = eng.last["w"]
    N = B * S
    if route == "tall":
        assert getattr(w, "er_tall", None) is not None
    else:
        # [32, 512] still fits one CU's LDS (the in-LDS Jacobi takes a wide matrix as it is); [40, 1024] does not: the blocked
        # Jacobi on fused^T, the branch configuration five's per-GPU shape [256, 1024] takes
        assert (w.er_blk is None) == ops.erank_fits(N, H) == ((N, H) != (40, 1024))
        if w.er_blk is not None:
            assert w.er_flip == (N < H) and float(w.er_stats[0, 3]) < eng.erank_max_sweeps
    got = float(eng.erank_value())
    assert abs(got - er) < 5e-3 * max(1.0, er / 50), (got, er)
    worst = (0.0, "")
    for n, r in grads.items():
        if r is not None:
            g = eng.arena.g(n).double().cpu()
            worst = max(worst, (float((g - r).abs().max()) / max(float(r.abs().max()), 1e-5), n))
    print(f"[m3 penalty B{B} S{S} H{H} {route}] erank {got:.4f} vs svdvals {er:.4f}, worst gradient error / scale {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 1e-2, worst


# ---------------------------------------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------------------------------------
def test_dropout_keep_rates_graph_and_offset():
    c = MC._step("drop", 8, 16, 128, 8, 17, 1, 256, 70)
    b = [t.cuda() for t in MC.batch(c)]
    runs = {}
    for how in ("eager", "graphed"):
        model, eng, _ = _engine(c, dropout=True, use_seam=True)
        model.train()
        for step in range(2):
            if how == "eager":
                eng.train_step(b[0], b[1], b[2], b[3], b[4], 1e-3, 5e-3, training=True, gaze=b[5])
            else:
                eng.train_step_graphed(b[0], b[1], b[2], b[3], b[4], 1e-3, 5e-3, training=True, gaze=b[5])
            torch.cuda.synchronize()
            assert int(eng.drop_offset.item()) == step + 1 and int(eng.step_t.item()) == step + 1      # once per step
        w = eng.shapes[(c["B"], c["S"], True)]
        runs[how] = (eng.arena.params.clone(), w.drop_pool.clone(), w.loss.clone())
        assert eng.last["drop"] and eng.last["seam"]
        for k, m in w.drop.items():
            rate = float(m.float().mean())
            n = m.numel()
            assert set(m.unique().tolist()) <= {0, 1}
            # keep probability 0.9: five standard deviations of a binomial of n draws
            assert abs(rate - 0.9) <= 5 * (0.09 / n) ** 0.5, (k, rate, n)
        x0 = w.x0.view(-1)
        assert bool((x0[w.drop["x0"] == 0] == 0).all())                   # embd_drop's mask is the one the seam applied
    assert torch.equal(runs["eager"][1], runs["graphed"][1])              # the same masks at the same seed and offset
    assert torch.equal(runs["eager"][0], runs["graphed"][0]) and torch.equal(runs["eager"][2], runs["graphed"][2])


def test_graphed_steps_of_alternating_clip_lengths_equal_eager_steps():
    """A captured step clears the pos_embedding gradient rows [S, mark) as the high-water mark stood at its capture.  A short
    clip captured BEFORE a longer one was seen must not be replayed after it: rows [S, longer) would keep the longer step's
    gradient and AdamW would apply it again.  The mark's value is in the capture key; here S = 5, 8, 5, 8, 5, 12, 5."""
    c = MC._step("alt", 2, 5, 64, 4, 17, 1, 256, 95)
    seq = [5, 8, 5, 8, 5, 12, 5]
    batches = [[t.cuda() for t in MC.batch(c, seed=95 + i, S=S)] for i, S in enumerate(seq)]
    finals = {}
    for how in ("eager", "graphed"):
        model, eng, _ = _engine(c, use_seam=True)
        model.train()
        step = eng.train_step if how == "eager" else eng.train_step_graphed
        for b in batches:
            step(b[0], b[1], b[2], b[3], b[4], 1e-3, 5e-3, training=True, gaze=b[5])
        torch.cuda.synchronize()
        g = eng.arena.g("pos_embedding")
        assert float(g[0, 5:].abs().max()) == 0.0 and float(g[0, :5].abs().max()) > 0.0      # (the last step had 5 frames)
        assert int(eng.step_t.item()) == len(seq) and eng.pos_grad_rows == 12
        finals[how] = (eng.arena.params.clone(), eng.arena.exp_avg.clone(), eng.arena.p("pos_embedding")[0, :12].clone())
        if how == "graphed":
            assert len(eng.graphs) == 5          # S = 5 at marks 5, 8 and 12; S = 8 at mark 8; S = 12
    assert torch.equal(finals["eager"][2], finals["graphed"][2])
    assert torch.equal(finals["eager"][0], finals["graphed"][0]) and torch.equal(finals["eager"][1], finals["graphed"][1])


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
class _NoSched:
    def step(self):
        pass


def _train(c, tmp_path, extra, batches, val):
    from r3d_amd.optim import FlatAdamW
    from r3d_amd.opts import parser
    from r3d_amd.train_proposed_depth import train
    model, eng, _ = _engine(c, dropout=False)
    opt = parser.parse_args(extra)
    args = argparse.Namespace(epochs=2, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=8,
                              graph_steps=opt.graph_steps, erank_report=opt.erank_report, erank_weight=opt.erank_weight,
                              erank_route=opt.erank_route, erank_every=0, restore_train_mode=False, supcon_weight=0.0,
                              pixel_shard=False)
    tmp_path.mkdir(parents=True, exist_ok=True)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train(args, model, batches, FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3), _NoSched(), None, str(tmp_path),
              MC.pad_idx(c), torch.device("cuda"), val, seed=0)
    torch.cuda.synchronize()
    return model, buf.getvalue()


def test_train_graphed_equals_eager_and_reports_four_ranks(tmp_path):
    c = MC._step("loop", 8, 6, 64, 4, 17, 1, 256, 80)
    batches = [MC.batch(c, seed=80), MC.batch(c, seed=81, B=3), MC.batch(c, seed=82)]       # (the middle one is skipped: 3 < 8)
    val = [MC.batch(c, seed=90, B=2, S=7)]
    m_g, text_g = _train(c, tmp_path / "g", ["--erank_report"], batches, val)
    m_e, text_e = _train(c, tmp_path / "e", ["--erank_report", "--no_graph_steps"], batches, val)
    for (n, p), (_, q) in zip(m_g.named_parameters(), m_e.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    assert text_g == text_e
    lines = [ln for ln in text_g.splitlines() if ln.startswith("Effective rank over")]
    rows = int((val[0][2] != MC.pad_idx(c)).sum())                     # unpadded validation frames
    assert len(lines) == 2 and all(re.fullmatch(rf"Effective rank over {rows} frames: rgb [0-9.]+, depth [0-9.]+, gaze [0-9.]+, "
                                                rf"fused [0-9.]+", ln) for ln in lines), text_g
    assert len(re.findall(r"Loss : [0-9.]+", text_g)) == 2 and "Training Acc" in text_g
    assert int(m_g.engine().step_t.item()) == 4
    # a 5-element batch to this model, and a 6-element batch to the two-modality model, are refused
    from r3d_amd.train_proposed_depth import validate
    with pytest.raises(ValueError, match="6-element"):
        validate(m_g, [val[0][:5]], None, MC.pad_idx(c), torch.device("cuda"))
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR as F2
    m2 = F2(17, 64, 18, torch.device("cuda"), MC.make_args(c), n_query=8, n_head=4, num_encoder_layers=1, num_decoder_layers=1,
            depth_pixels=256).to("cuda")
    with pytest.raises(ValueError, match="only the three-modality model"):
        validate(m2, val, None, 18, torch.device("cuda"))
    from r3d_amd.parallel import DataParallelStep
    with pytest.raises(ValueError, match="one GPU"):
        DataParallelStep(m_g.engine())                     # (asked of the engine before anything is hooked into it)
    assert m_g.engine().grad_hook is None
    from r3d_amd.rankstream import measure_rank
    r = measure_rank(m_g, val, torch.device("cuda"))
    assert sorted(r) == ["depth", "fused", "gaze", "rgb"] and all(v["rows"] == rows for v in r.values())
