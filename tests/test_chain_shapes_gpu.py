"""The hidden-128 chain kernels (csrc/fuser_chain.hip, csrc/decoder_chain.hip with mha_small.h / losses_dev.h) over every
batch shape tests/chain_cases.py lists: the K boundaries of the segmentation head, the bf16x3 / fp32 backward and the tail
in or out of the decoder chain, key counts Lk = S from 1 to 65, ragged key padding, B != 8 and the NTU head (K = 122).

Each row must (a) take the path its row states -- a quiet fall-back to the composed launches fails --, (b) match the
oracle run in float64 (eval mode), (c) agree with the composed launches, the fp32 chain and the undeferred tail under
dropout.  Then: validation forwards at B = 1, the rank penalty at the NTU shape, and one engine (and train()) switching
between chain and composed paths as the batch shape changes from step to step."""
import argparse
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import futr_oracle as O, synth  # noqa: E402
from tests import chain_cases as CC  # noqa: E402
from tests.helpers import assert_close, ffn_kink_units, without_kink_units  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

ARGS = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")


@functools.lru_cache(maxsize=None)
def _params(K):
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    m = FUTR(K, CC.H, K + 1, torch.device("cpu"), ARGS, n_query=CC.Q, n_head=CC.HEADS, num_encoder_layers=2,
             num_decoder_layers=1)
    names = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    return {n: torch.from_numpy(v) for n, v in synth.fill_state(names).items()}


def params(K):
    return {n: v.clone() for n, v in _params(K).items()}


def build_model(K):
    from r3d_amd.model.futr_safuser_tokenfusion import FUTR
    model = FUTR(K, CC.H, K + 1, torch.device("cuda"), ARGS, n_query=CC.Q, n_head=CC.HEADS, num_encoder_layers=2,
                 num_decoder_layers=1)
    model.load_state_dict(params(K), strict=False)
    return model.to("cuda")


def f64(batch):
    return [t.double() if t.is_floating_point() else t for t in batch]


def oracle_step64(K, batch):
    """fp64 oracle: outputs, losses and every parameter gradient; plus the fp32 oracle's selected channels, which the
    kernel must reproduce bit for bit -- and which the fp64 run must share, or the fp64 comparison would be meaningless."""
    tr = O.CpuTrainer({n: v.double() for n, v in params(K).items()}, K + 1, CC.HEADS, 1)
    res, out, aux = tr.step(f64(batch), apply=False)
    with torch.no_grad():
        _, aux32 = O.forward(params(K), (batch[0], batch[2]), batch[1], "train", K + 1, CC.HEADS, 1)
    for k in ("idx_rgb", "idx_dep"):
        assert torch.equal(aux32[k], aux[k]), f"fp32 and fp64 oracles select different {k}"
    return tr, res, out, aux, aux32


def run_step(eng, d, training):
    eng.forward(d[0], d[1], d[2], "train", training=training)
    w = eng.last["w"]
    deferred = bool(getattr(w, "_dec_deferred", False))
    loss, counts = eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()
    return w, deferred, loss, counts


def assert_path(eng, w, c, deferred, drop, er=False):
    """The launches the engine made for this workspace: the argument blocks it built are cached in w.tables, which must be
    fresh (a new engine, or cleared before the step) -- exactly the chain blocks of the row's path, nothing else."""
    bf3 = bool(eng.chain_bf3)
    assert eng._chain_ok(w) == c.fuser and eng._dec_chain_ok(w) == c.dec, (c, eng._chain_ok(w), eng._dec_chain_ok(w))
    want = set()
    if c.fuser:
        want |= {("fwd_chain", drop, bf3), ("bwd_chain", drop, er, c.bwd == "bf3" and bf3)}
    if c.dec:
        want.add(("dec_chain", drop, bf3))
    got = {k for k in w.tables if k[0] in ("fwd_chain", "bwd_chain", "dec_chain")}
    assert got == want, (c, sorted(map(str, got)), sorted(map(str, want)))
    assert deferred == (c.defer and bool(eng.defer_tail)), (c, deferred)


# ------------------------------------------------------------------------------------------------------------------
# (a) + (b): path and fp64 oracle, eval mode
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CC.CASES, ids=CC.case_id)
def test_chain_shape_against_fp64_oracle(c, oracle_lib):
    B, S, K, H = c.B, c.S, c.K, CC.H
    batch = CC.make_batch(c)
    tr, res, oout, oaux, aux32 = oracle_step64(K, batch)
    model = build_model(K).eval()
    eng = model.engine()
    eng.defer_tail = True                 # the training flow's routing (train(), train_step())
    d = [t.cuda() for t in batch]
    w, deferred, loss, counts = run_step(eng, d, training=False)
    assert_path(eng, w, c, deferred, drop=False)
    assert torch.equal(eng.last["idx"][0].cpu(), aux32["idx_rgb"]) and torch.equal(eng.last["idx"][1].cpu(), aux32["idx_dep"])
    out = dict(seg=w.seg.view(B, S, K), action=w.actdur[:, :K].reshape(B, CC.Q, K), duration=w.actdur[:, K].reshape(B, CC.Q))
    for k in ("action", "duration", "seg"):
        close_rel(out[k], oout[k].detach(), f"{CC.case_id(c)}/{k}")
    close_rel(w.fused.view(B, S, H), oaux["fused"].detach(), f"{CC.case_id(c)}/fused")
    want = torch.stack([res[k].detach() for k in ("loss_seg", "loss_action", "loss_dur", "loss")])
    assert_close(loss.cpu(), want, 1e-3, 1e-6, f"{CC.case_id(c)}/losses")
    kink = ffn_kink_units(oaux["ffn_pre"])
    assert len(kink) <= 4, f"{CC.case_id(c)}: {len(kink)} FFN units on the ReLU kink"
    rtol = 2e-3 if not kink else 4e-3
    n_grads = 0
    for n, p in tr.p.items():
        if p.grad is None:
            continue
        g, r = without_kink_units(n, eng.arena.g(n).cpu(), p.grad, kink)
        close_rel(g, r, f"{CC.case_id(c)}/grad {n}" + (f" (kink units {sorted(kink)} excluded)" if kink else ""), rtol=rtol)
        n_grads += 1
    assert n_grads == len(eng.arena.live_names)


# ------------------------------------------------------------------------------------------------------------------
# (c): chain vs composed, fp32 vs bf16x3 chain, deferred vs separate tail -- dropout on, same masks
# ------------------------------------------------------------------------------------------------------------------
FUSER_ACTS = ("x1", "h2", "u", "x3", "fused", "seg")
DEC_ACTS = ("p_ca", "ca_o", "t2", "ff1", "t3_pre", "t3")
OUT_ACTS = ("tgtF", "actdur", "d_seg", "d_actdur", "d_fused")


def _snapshot(eng, d, flags):
    for k, v in flags.items():
        setattr(eng, k, v)
    for w in eng.shapes.values():
        w.tables.clear()                  # (argument blocks are rebuilt on use: what w.tables then holds, THIS run built)
    w, deferred, loss, counts = run_step(eng, d, training=True)     # no tick: the same drop_offset -> the same masks
    acts = {k: getattr(w, k).clone() for k in FUSER_ACTS + OUT_ACTS}
    acts.update({"l0_" + k: w.layers[0][k].clone() for k in DEC_ACTS})
    return dict(w=w, deferred=deferred, acts=acts, loss=loss.clone(), counts=counts.clone(), grads=eng.arena.grads.clone())


def _agree(eng, a, b, what):
    for k in a["acts"]:
        close_rel(b["acts"][k], a["acts"][k], f"{what}: {k}", rtol=5e-5)
    close_rel(b["loss"], a["loss"], f"{what}: loss", rtol=1e-5)
    assert torch.equal(b["counts"], a["counts"]), (what, a["counts"], b["counts"])
    g = lambda r, n: r["grads"][eng.arena.offsets[n][0]:eng.arena.offsets[n][0] + eng.arena.offsets[n][1]]   # noqa: E731
    for n in eng.arena.live_names:
        if n == "fc_len.bias":
            # exactly zero: the duration loss L1-normalises exp(duration) over each clip's queries, which a shift of
            # every duration cancels -- both sides are rounding noise, bounded by the chain bound of fc_len.weight's scale
            lim = 5e-4 * float(g(a, "fc_len.weight").abs().max())
            assert max(float(g(a, n).abs().max()), float(g(b, n).abs().max())) <= lim, (what, g(a, n), g(b, n), lim)
            continue
        close_rel(g(b, n), g(a, n), f"{what}: grad {n}", rtol=5e-4)


@pytest.mark.parametrize("c", CC.CASES, ids=CC.case_id)
def test_chain_shape_paths_agree(c):
    model = build_model(c.K).train()
    eng = model.engine()
    d = [t.cuda() for t in CC.make_batch(c)]
    off = dict(use_fuser_chain=False, use_decoder_chain=False, chain_bf3=True, defer_tail=False)
    on = dict(use_fuser_chain=True, use_decoder_chain=True, chain_bf3=True, defer_tail=False)
    composed = _snapshot(eng, d, off)
    assert not [k for k in composed["w"].tables if "chain" in str(k[0])], "chains switched off, yet a chain launch ran"
    chain = _snapshot(eng, d, on)
    assert_path(eng, chain["w"], c, chain["deferred"], drop=True)
    _agree(eng, composed, chain, f"{CC.case_id(c)} chain vs composed")
    fp32 = _snapshot(eng, d, dict(on, chain_bf3=False))
    assert_path(eng, fp32["w"], c, fp32["deferred"], drop=True)
    _agree(eng, chain, fp32, f"{CC.case_id(c)} fp32 chain vs bf16x3 chain")
    if c.defer:
        deferred = _snapshot(eng, d, dict(on, defer_tail=True))
        assert_path(eng, deferred["w"], c, deferred["deferred"], drop=True)
        _agree(eng, chain, deferred, f"{CC.case_id(c)} tail in the decoder chain vs separate")
    for k, v in on.items():
        setattr(eng, k, v)


# ------------------------------------------------------------------------------------------------------------------
# (e): validation forwards at B = 1
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,K,dec", CC.VAL_CASES, ids=[f"B{b}-S{s}-K{k}" for b, s, k, _ in CC.VAL_CASES])
def test_val_mode_shapes_against_fp64_oracle(B, S, K, dec, oracle_lib):
    c = CC.Case(B, S, K, "none", False, None, dec, False, "val")
    feats, depth, lab, dur, tgt = CC.make_batch(c)
    oout, oaux = O.forward({n: v.double() for n, v in params(K).items()}, (feats.double(), lab), depth.double(), "val",
                           K + 1, CC.HEADS, 1)
    _, aux32 = O.forward(params(K), (feats, lab), depth, "val", K + 1, CC.HEADS, 1)
    for k in ("idx_rgb", "idx_dep"):
        assert torch.equal(aux32[k], oaux[k]), f"fp32 and fp64 oracles select different {k}"
    model = build_model(K).eval()
    with torch.no_grad():
        out = model((feats.cuda(), lab.cuda()), depth.cuda(), mode="val")
    torch.cuda.synchronize()
    eng = model.engine()
    w = eng.last["w"]
    assert not eng._chain_ok(w) and eng._dec_chain_ok(w) == dec
    assert (("dec_chain", False, bool(eng.chain_bf3)) in w.tables) == dec, sorted(map(str, w.tables))
    assert torch.equal(eng.last["idx"][0].cpu(), aux32["idx_rgb"]) and torch.equal(eng.last["idx"][1].cpu(), aux32["idx_dep"])
    for k in ("action", "duration", "seg"):
        close_rel(out[k], oout[k], f"val B{B} S{S}/{k}")


# ------------------------------------------------------------------------------------------------------------------
# (f): the rank penalty at the NTU shape (fp32 backward chain with d_extra)
# ------------------------------------------------------------------------------------------------------------------
def test_effective_rank_penalty_at_the_ntu_head(oracle_lib):
    lam = 0.05
    c = next(c for c in CC.CASES if (c.B, c.S, c.K) == (8, 32, 122))
    batch = CC.make_batch(c)
    K, H = c.K, CC.H
    tr = O.CpuTrainer({n: v.double() for n, v in params(K).items()}, K + 1, CC.HEADS, 1)
    b64 = f64(batch)
    out, aux = O.forward(tr.p, (b64[0], b64[2]), b64[1], "train", K + 1, CC.HEADS, 1)
    res = O.losses(out, b64[2], b64[3], b64[4], K + 1)
    er = O.effective_rank_torch(aux["fused"].reshape(-1, H))
    (res["loss"] - lam * er).backward()
    model = build_model(K).eval()
    eng = model.engine()
    eng.erank_weight = lam
    d = [t.cuda() for t in batch]
    w, deferred, loss, counts = run_step(eng, d, training=False)
    assert_path(eng, w, c, deferred, drop=False, er=True)
    assert ("bwd_chain", False, True, False) in w.tables
    got = float(eng.erank_value())
    assert abs(got - float(er)) < 5e-3 * max(1.0, float(er) / 50), (got, float(er))
    for n, p in tr.p.items():
        if p.grad is not None:
            close_rel(eng.arena.g(n), p.grad, f"NTU head erank-penalised grad {n}", rtol=1e-2)


# ------------------------------------------------------------------------------------------------------------------
# (g): one engine across changing batch shapes
# ------------------------------------------------------------------------------------------------------------------
ALTERNATION = [(8, 16), (9, 16), (8, 7), (10, 33), (8, 65), (8, 16)]


def _alt_batch(i, B, S, K=17):
    return CC.make_batch(CC.Case(B, S, K, "tail", None, None, None, None, ""), seed=CC.BATCH_SEED + i)


def test_one_engine_switching_shapes_equals_fresh_engines():
    """Each step's losses, counters and gradients bit for bit those of a freshly built engine at that shape: nothing of
    one shape's workspace, argument blocks (w.tables) or weight planes leaks into another's (dropout on, same masks)."""
    model = build_model(17).train()
    eng = model.engine()
    for i, (B, S) in enumerate(ALTERNATION):
        d = [t.cuda() for t in _alt_batch(i, B, S)]
        _, _, loss, counts = run_step(eng, d, training=True)
        got = (loss.clone(), counts.clone(), eng.arena.grads.clone())
        fresh = build_model(17).train().engine()
        _, _, loss, counts = run_step(fresh, d, training=True)
        assert torch.equal(got[0], loss), (i, B, S, got[0], loss)
        assert torch.equal(got[1], counts), (i, B, S)
        assert torch.equal(got[2], fresh.arena.grads), (i, B, S, float((got[2] - fresh.arena.grads).abs().max()))


# short shapes are captured before the longest clip length (65) appears, then replayed after it: a replay must clear the
# pos_embedding gradient rows the longer batches wrote, as the eager step does
TRAIN_ORDER = [(8, 7), (8, 7), (8, 7), (8, 16), (8, 16), (9, 16), (9, 16), (8, 65), (8, 7), (8, 16), (10, 33), (9, 16),
               (8, 65), (8, 7), (8, 7), (8, 16), (10, 33), (8, 16)]


def test_train_over_mixed_shapes_graphed_equals_eager(tmp_path):
    """train() over batches whose shape changes from step to step (each shape eager, then captured, then replayed; short
    shapes captured before the longest one appears) with and without hipGraph replay: bitwise-identical final
    parameters."""
    from r3d_amd.train_proposed_depth import train
    from r3d_amd.optim import FlatAdamW, LinearWarmupCosineAnnealingLR
    assert set(TRAIN_ORDER) == set(ALTERNATION)
    batches = [_alt_batch(i, B, S) for i, (B, S) in enumerate(TRAIN_ORDER)]
    val = [[t[:1] for t in batches[0]]]
    finals = []
    for graph_steps in (False, True):
        model = build_model(17)
        p0 = model.engine().arena.params.clone()
        args = argparse.Namespace(epochs=1, input_type="i3d_transcript", seg=True, anticipate=True, task="long",
                                  min_batch=1, graph_steps=graph_steps)
        opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)
        sch = LinearWarmupCosineAnnealingLR(opt, warmup_epochs=2, max_epochs=4)
        sch.step()
        sch.step()                                        # (epoch 0 of the schedule runs at lr 0: start where lr > 0)
        train(args, model, batches, opt, sch, None, str(tmp_path), 18, torch.device("cuda"), val, seed=1)
        torch.cuda.synchronize()
        finals.append(model.engine().arena.params.clone())
    assert not torch.equal(finals[0], p0), "the steps changed no parameter"
    assert torch.equal(finals[0], finals[1]), float((finals[0] - finals[1]).abs().max())
