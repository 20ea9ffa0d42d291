"""The decoder chain's one-launch route (csrc/decoder_chain.hip, phases 7: forward half, tail + losses, backward half, with
the hand-offs between them on chip) against the same step as three launches (forward half / tail_losses_kernel / backward
half, every hand-off through global memory): hidden 128, Q = 8, 8 heads, depth frames of 16 x 16 pixels.

Two references.  THREE LAUNCHES -- phases 1, then tail_losses_kernel alone, then phases 4 -- run the same device code as the
one launch on the same values in the same order (tail_losses_kernel is tail_clip_body in its global form, the loss workgroups
are the same function), only with every hand-off through global memory: all 44 tensors must be EQUAL bit for bit.  A stale
LDS tile, a missing barrier, garbage in rows 8..15 of an operand image, or a value handed over unrounded where the memory
route rounds it (an FMA contracted across the hand-off) shows as a bit difference -- in ca_o's planes, in the d_ff2 planes,
in the d_t3pre and d_cao tiles alike.

DEFER_TAIL=FALSE, the engine's own split route.  Its forward half is again the same code, so what that stores (p_ca, ca_o,
t2_pre, t2, m2, r2, ff1, t3_pre, and seg from the launch before it) and the counters must be EQUAL.  From the tail on it is
NOT the same arithmetic: its tail forward is decoder_tail_fwd (tail.hip), whose head products and LayerNorm sums run in
another order than tail_clip_body's.  Run on the commit before the hand-offs moved on chip, ALL EIGHT cases (B2-S1-K17-none,
B3-S7-K23-tail, B2-S64-K17-ragged, B8-S16-K17-tail, each with dropout off and on) differed from the tail on: 16 to 18 of the
44 tensors, actdur by up to 4.8e-7, the loss by up to 1.9e-6 absolute, the decoder layer's gradients by 7e-9 .. 3e-8.  What
the tail and the backward half store is therefore compared at 1e-6 of each tensor's scale in every case.  With one key per
clip d_caq and d_caqin have no scale of their own (they are zero in exact arithmetic); they are held to an exact zero without
dropout and to 1e-6 of the scale of the operands they derive from with it (the comment at the comparison).

Then the fuser chain's query role (the other caller of the small attention units inside a chain) against the composed
launches: at the kernel's arguments B = 2, S = 1 and S = 7 by a direct launch of the engine's argument block (a batch of two
such clips is below the fuser role's 16-row granularity, so the engine itself never makes that launch), and through the
engine, backward included, at the two-clip shapes it admits, (B=2, S=4) and (B=2, S=8)."""
import argparse
import collections
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import synth  # noqa: E402
from tests import chain_cases as CC  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

ARGS = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
HW = (16, 16)

Handoff = collections.namedtuple("Handoff", "B S K pad why")
CASES = [
    Handoff(2, 1, 17, "none", "one key per clip"),
    Handoff(3, 7, 23, "tail", "odd B and S; largest head count whose tail stays in the chain"),
    Handoff(2, 64, 17, (1, 64), "largest S; a clip with one valid key"),
    Handoff(8, 16, 17, "tail", "the headline shape"),
]


def _id(c):
    return f"B{c.B}-S{c.S}-K{c.K}-{c.pad if isinstance(c.pad, str) else 'ragged'}"


@functools.lru_cache(maxsize=None)
def _params(K):
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    m = FUTR(K, CC.H, K + 1, torch.device("cpu"), ARGS, n_query=CC.Q, n_head=CC.HEADS, num_encoder_layers=2,
             num_decoder_layers=1, depth_pixels=HW[0] * HW[1])
    names = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    return {n: torch.from_numpy(v) for n, v in synth.fill_state(names).items()}


def build_model(K):
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    model = FUTR(K, CC.H, K + 1, torch.device("cuda"), ARGS, n_query=CC.Q, n_head=CC.HEADS, num_encoder_layers=2,
                 num_decoder_layers=1, depth_pixels=HW[0] * HW[1])
    model.load_state_dict({n: v.clone() for n, v in _params(K).items()}, strict=False)
    return model.to("cuda")


def _batch(c):
    return [t.cuda() for t in CC.make_batch(CC.Case(c.B, c.S, c.K, c.pad, None, None, None, None, c.why), depth_hw=HW)]


def _step(eng, d, training, route):
    """One training step, its decoder chain run by `route`:
    "one"    defer_tail=True: forward half, tail + losses and backward half in ONE launch (phases 7), hand-offs on chip;
    "three"  the same device code as three launches -- phases 1, tail_losses_kernel on its own (tail_clip_body in its global
             form), phases 4 -- with every hand-off through global memory;
    "split"  defer_tail=False: phases 1, decoder_tail_fwd (tail.hip), the loss launch, the tail's backward, phases 4."""
    eng.defer_tail = route != "split"
    for w in eng.shapes.values():
        w.tables.clear()
    eng.forward(d[0], d[1], d[2], "train", training=training)           # no tick between the runs: the same dropout masks
    w = eng.last["w"]
    deferred = bool(getattr(w, "_dec_deferred", False))
    assert deferred == (route != "split"), (route, deferred)
    if route == "three":
        # the forward half as a launch of its own: losses() then finds no decoder chain pending and launches the tail and
        # the losses alone, and backward() the backward half
        eng._dec_chain(w, eng.last["drop"]).launch(1, key_label=w._dec_key_labels)
        w._dec_deferred = False
    loss, counts = eng.losses(d[2], d[4], d[3])
    in_one = bool(getattr(w, "_dec_bwd_done", False))                   # the backward half ran inside losses()'s launch
    assert in_one == (route == "one"), (route, in_one)
    eng.backward()
    torch.cuda.synchronize()
    assert ("dec_chain", bool(training), True) in w.tables, sorted(map(str, w.tables))
    snap = dict(loss=loss.clone(), counts=counts.clone(), seg=w.seg.clone(), actdur=w.actdur.clone(), tgtF=w.tgtF.clone(),
                d_seg=w.d_seg.clone(), d_actdur=w.d_actdur.clone(), grads=eng.arena.grads.clone())
    snap.update({"l0_" + k: v.clone() for k, v in w.layers[0].items() if torch.is_tensor(v)})
    snap.update({"g0_" + k: v.clone() for k, v in w.glayers[0].items() if torch.is_tensor(v)})
    return snap


NAMED = ("g0_caq", "g0_cakv", "g0_t3pre", "g0_ff2", "g0_ff1", "g0_t2pre", "g0_cap", "g0_cao", "l0_ca_o", "l0_t2_pre",
         "l0_m2", "l0_r2", "l0_ff1", "l0_t3_pre", "l0_t3", "l0_p_ca")
FORWARD_HALF = ("seg", "counts", "l0_p_ca", "l0_ca_o", "l0_t2_pre", "l0_t2", "l0_m2", "l0_r2", "l0_ff1", "l0_t3_pre")


@pytest.mark.parametrize("training", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_one_launch_equals_split_launches(c, training):
    """Losses, counters, seg, actdur, every stored activation and gradient of the decoder layer (d_caq and d_cakv among
    them) and the whole gradient arena of the one-launch route: EQUAL to the three-launch route's in every tensor, and
    against defer_tail=False equal in the forward half's tensors and the counters, within 1e-6 in the rest (module
    docstring)."""
    model = build_model(c.K)
    model.train(training)
    eng = model.engine()
    d = _batch(c)
    split = _step(eng, d, training, "split")
    three = _step(eng, d, training, "three")
    one = _step(eng, d, training, "one")
    eng.defer_tail = False
    for k in NAMED:
        assert k in one, (k, sorted(one))
    assert sorted(one) == sorted(three) == sorted(split)
    bad = []
    # ---- the same device code with the hand-offs through global memory: bit for bit, every tensor
    for k in three:
        if not bool(torch.isfinite(one[k].double()).all()):
            bad.append(f"{k}: not finite")
        if not torch.equal(one[k], three[k]):
            diff = (one[k].double() - three[k].double()).abs()
            bad.append(f"{k}: {int((diff != 0).sum())} of {diff.numel()} differ from the three-launch route, "
                       f"max |diff| {float(diff.max()):.3e} at scale {float(three[k].double().abs().max()):.3e}")
    # ---- defer_tail=False
    H, dh = CC.H, CC.H // CC.HEADS
    eps = 2.0 ** -24
    for k in split:
        diff = (one[k].double() - split[k].double()).abs()
        scale = max(float(split[k].double().abs().max()), 1e-5)
        n, err = int((diff != 0).sum()), float(diff.max()) if diff.numel() else 0.0
        if c.S == 1 and k in ("g0_caq", "g0_caqin"):
            # One key per clip: the softmax over it is exactly 1, so dS = P (dP - sum P dP) is dP - dP.  Without dropout
            # that is an exact zero on every route.  With dropout dP = (dO . V) * keep may be contracted into the
            # subtraction, which leaves the product's rounding error: |dS| <= 2^-24 |dP| / sqrt(dh) with
            # |dP| <= dh max|dO| max|V| drop_scale, d_caq = dS K, d_caqin = d_caq . Wq (H terms).  The two routes' d_cao
            # differ (below), so their residues are unrelated: the difference is bounded by twice that, which stays below
            # 1e-6 of the scale the values derive from, max|d_cao| max|V| max|K| (2 * 2^-24 * 16 * 1.12 / 4 = 5.3e-7).
            if not training:
                lim = 0.0
            else:
                kv = split["l0_cakv"].double().abs()
                lim = 1e-6 * float(split["g0_cao"].double().abs().max()) * float(kv[:, H:].max()) * float(kv[:, :H].max())
                assert 2 * eps * dh * (1.0 / 0.9 + 1e-3) / dh ** 0.5 < 1e-6
                if k == "g0_caqin":
                    wq = eng.arena.p("transformer.decoder.layers.0.multihead_attn.in_proj_weight")[:H]
                    lim *= H * float(wq.double().abs().max())
            print(f"{_id(c)} training={training} {k}: zero up to the product's rounding, max |diff| {err:.3e}, "
                  f"max |value| {float(one[k].abs().max()):.3e} / {float(split[k].abs().max()):.3e}, bound {lim:.3e}")
            if not err <= lim or (not training and bool(one[k].abs().max() > 0)):
                bad.append(f"{k}: max |diff| {err:.3e} above {lim:.3e}")
            continue
        if n:
            print(f"{_id(c)} training={training} {k}: {n} of {diff.numel()} differ, max |diff| {err:.3e}, rel {err / scale:.2e}")
        if (k in FORWARD_HALF and n) or err > 1e-6 * scale:
            bad.append(f"{k}: {n} of {diff.numel()} differ, max |diff| {err:.3e} at scale {scale:.3e}")
    assert not bad, (_id(c), training, bad)
    assert bool(split["grads"].abs().max() > 0) and bool(torch.isfinite(split["grads"]).all())


SA_NAMES = ("sa_qkv", "p_sa", "sa_o", "t1_pre", "t1", "m1", "r1", "caq", "cakv")
SA_GRADS = ("caqin", "sap", "sao", "saqkv", "sain")


def _query_role_against_composed(B, S, training):
    c = Handoff(B, S, 17, "none", "")
    model = build_model(c.K)
    model.train(training)
    eng = model.engine()
    d = _batch(c)
    res = []
    for chain in (False, True):
        eng.use_fuser_chain = chain
        for w in eng.shapes.values():
            w.tables.clear()
        eng.forward(d[0], d[1], d[2], "train", training=training)          # same drop_offset -> same masks
        w = eng.last["w"]
        assert eng._chain_ok(w) == chain, f"B={B} S={S}: the fuser chain {'did not run' if chain else 'ran'}"
        assert (("fwd_chain", bool(training), True) in w.tables) == chain, sorted(map(str, w.tables))
        eng.losses(d[2], d[4], d[3])
        eng.backward()
        torch.cuda.synchronize()
        acts = {k: w.layers[0][k].clone() for k in SA_NAMES}
        acts.update({"g_" + k: w.glayers[0][k].clone() for k in SA_GRADS})
        acts.update(fused=w.fused.clone(), seg=w.seg.clone())
        res.append(dict(acts=acts, grads=eng.arena.grads.clone(), loss=w.loss.clone()))
    for k in res[0]["acts"]:
        close_rel(res[1]["acts"][k], res[0]["acts"][k], f"B{B} S{S}/chain {k}", rtol=5e-5)
    close_rel(res[1]["loss"], res[0]["loss"], "loss", rtol=1e-5)
    a = eng.arena
    for n in a.live_names:
        o, k, _ = a.offsets[n]
        close_rel(res[1]["grads"][o:o + k], res[0]["grads"][o:o + k], f"B{B} S{S}/chain grad {n}", rtol=5e-4)


QUERY_ROLE = ("sa_qkv", "p_sa", "sa_o", "t1_pre", "t1", "m1", "r1", "caq")


@pytest.mark.parametrize("B,S", [(2, 1), (2, 7)], ids=["B2-S1", "B2-S7"])
def test_fuser_chain_query_role_equals_composed(B, S):
    """r3d_fuser_chain_fwd launched with B = 2 clips for its query role and S = 1 / S = 7, against the composed launches.
    The engine cannot make that launch from a batch of two such clips (2*B*S = 4 / 28 frame rows are no whole 16-row
    workgroups for the fuser role), but the entry point takes N apart from B: the frame rows here are those of eight clips
    (N = 8 S, a shape the engine admits, whose argument block it builds), and the launch is repeated with the block's B set
    to 2.  The query sub-layer reads parameters and its dropout masks only, row by row and clip by clip, so its rows of
    the first two clips must equal the composed path's at the tolerance of
    test_fuser_chain_kernel_equals_composed_launches, and the rows of the other six clips must stay untouched."""
    c = Handoff(8, S, 17, "none", "")
    model = build_model(c.K)
    model.train(True)
    eng = model.engine()
    d = _batch(c)
    eng.use_fuser_chain = False
    eng.forward(d[0], d[1], d[2], "train", training=True)                # same drop_offset below -> the same masks
    w = eng.last["w"]
    assert not eng._chain_ok(w)
    torch.cuda.synchronize()
    ref = {k: w.layers[0][k].clone() for k in QUERY_ROLE}
    eng.use_fuser_chain = True
    for ws in eng.shapes.values():
        ws.tables.clear()
    eng.forward(d[0], d[1], d[2], "train", training=True)                # builds the block, refreshes the weight planes
    w = eng.last["w"]
    assert eng._chain_ok(w)
    torch.cuda.synchronize()
    blk = w.tables[("fwd_chain", True, True)]
    assert (blk.args.B, blk.args.S, blk.args.N) == (8, S, 8 * S)
    for k in QUERY_ROLE:
        w.layers[0][k].zero_()
    blk.args.B = B
    try:
        blk.launch()
        torch.cuda.synchronize()
    finally:
        blk.args.B = 8
    for k in QUERY_ROLE:
        got, want = w.layers[0][k], ref[k]
        n = got.shape[0] * B // 8                                         # leading dimension: rows (or clips) of B of 8 clips
        assert got.shape[0] % 8 == 0 and n > 0, (k, got.shape)
        assert bool(want[:n].abs().max() > 0), k
        close_rel(got[:n], want[:n], f"B{B} S{S}/query role {k}", rtol=5e-5)
        assert not bool(got[n:].any()), f"{k}: rows of clips >= {B} were written by a launch with B = {B}"


@pytest.mark.parametrize("B,S", [(2, 4), (2, 8)], ids=["B2-S4", "B2-S8"])
def test_fuser_chain_query_role_equals_composed_admitted(B, S):
    """The nearest two-clip shapes the fuser chain admits: the query self-attention units (Lq = Lk = 8) and their backward
    inside fuser_chain_fwd / _bwd against mha_fwd_small_kernel / the gemm_ln rider, at the tolerances of
    test_fuser_chain_kernel_equals_composed_launches."""
    _query_role_against_composed(B, S, training=True)
