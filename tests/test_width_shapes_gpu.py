"""The composed path over the (hidden, heads, clip length) shapes of tests/width_cases.py, against the oracle run in float64.

Admitted rows: the step must take the path its row states (embedding seam or not, tail + losses in one launch or three,
side stream; the cross-attention core must be launched with the row's (Lq, Lk, dh) -- whether attention.hip then takes its
small or general kernel is decided inside the library, so the row's `attn` column is checked against the restated rule of
mha_small_ok, not observed), select the fp32 oracle's channels bit for bit, and match the fp64 oracle's
outputs, fused tokens and losses within 1e-3 of scale and every gradient within 2e-3 (4e-3 with kink units excluded).
Refused rows: the engine raises a ValueError naming the limit before anything is enqueued, and stays usable; train() with
graph replay over a dataset holding a refused clip length raises before that shape is captured.
Validation rows (VAL_CASES, VAL_CLIP_BOUNDS): validate()'s forward against the fp64 oracle's val forward, the channels that
token fusion and the activation-magnitude fuser select from |x| column sums bit for bit against the fp32 oracle, the
BN-blend fuser on running statistics far from the fresh state, and the longest forward-only clip and one frame past it."""
import argparse
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import futr_oracle as O, synth  # noqa: E402
from tests import plain_oracle as PO  # noqa: E402
from tests import vary_oracle as V  # noqa: E402
from tests import width_cases as WC  # noqa: E402
from tests.helpers import assert_close, ffn_kink_units, without_kink_units  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

ARGS = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
MODELS = {"tf": "futr_safuser_tokenfusion", "vary": "futr_safuser_tokenfusion_vary", "bn": "futr_safuser_batchnormalization",
          "plain": "futr_safuser_depth"}


def _cls(variant):
    import importlib
    return importlib.import_module(f"r3d_amd.model.{MODELS[variant]}").FUTR


def _new(variant, H, heads, K, device):
    kw = dict(depth_pixels=224 * 224) if variant == "bn" else {}       # synth.make_batch's depth frames
    return _cls(variant)(K, H, K + 1, torch.device(device), ARGS, n_query=WC.Q, n_head=heads, num_encoder_layers=2,
                         num_decoder_layers=1, **kw)


def params(variant, H, heads, K):
    names = [(n, tuple(p.shape)) for n, p in _new(variant, H, heads, K, "cpu").named_parameters()]
    return {n: torch.from_numpy(synth.fill_value(n, s, j)) for j, (n, s) in enumerate(names)}


def build_model(variant, H, heads, K, p):
    model = _new(variant, H, heads, K, "cuda")
    missing = model.load_state_dict(p, strict=False)
    assert not missing.unexpected_keys
    return model.to("cuda")


def bn_state(H, seed=None):
    """The BatchNorm buffers: the fresh state (mean 0, var 1), or with a seed a state far from it (per-channel means and
    variances that differ between the two BatchNorms, so a wrong buffer or channel index shows)."""
    st = {}
    for j, pre in enumerate(("fuser.bn_rgb.", "fuser.bn_depth.")):
        if seed is None:
            st[pre + "running_mean"], st[pre + "running_var"] = torch.zeros(H, dtype=torch.float64), torch.ones(H, dtype=torch.float64)
        else:
            g = torch.Generator().manual_seed(seed + j)
            st[pre + "running_mean"] = (0.5 * torch.randn(H, generator=g)).float().double()
            st[pre + "running_var"] = (0.25 + 2.0 * torch.rand(H, generator=g)).float().double()
        st[pre + "num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    return st


def f64(batch):
    return [t.double() if t.is_floating_point() else t for t in batch]


class Recorder:
    """Records the path-deciding launches of a step (the engine calls them as r3d_amd.ops attributes)."""
    NAMES = ("embed_fuse_fwd", "token_exchange_fwd", "bn_blend_fwd", "scaled_exchange_fwd", "plain_fuse_fwd", "colabssum",
             "token_select", "decoder_tail_losses", "decoder_tail_fwd", "mha_core_fwd", "check")

    def __init__(self, monkeypatch):
        from r3d_amd import ops
        self.calls = []
        for nm in self.NAMES:
            fn = getattr(ops, nm)

            def wrap(*a, _fn=fn, _nm=nm, **k):
                self.calls.append((_nm, a))
                return _fn(*a, **k)
            monkeypatch.setattr(ops, nm, wrap)

    def names(self):
        return [n for n, _ in self.calls]


def oracle64(c, batch, p):
    """fp64 oracle (outputs, losses, gradients) and the fp32 oracle's channel selection."""
    b64 = f64(batch)
    K, heads = c.K, c.heads
    if c.variant == "plain":                # (no selection: nothing for the fp32 oracle to decide)
        t64 = PO.Trainer(p, K + 1, heads, 1, dtype=torch.float64, erank_weight=c.erank)
        res, out, aux = t64.step(batch, apply=False)
        if c.erank:
            res["erank"] = aux["erank"]
        return t64, res, out, aux, None
    if c.variant == "vary":
        t64 = V.Trainer(p, K + 1, heads, 1, dtype=torch.float64)
        if c.erank:                         # (as tests/test_vary_gpu.py's rank-penalty test)
            out, aux = V.forward(t64.p, (b64[0], b64[2]), b64[1], "train", K + 1, heads, 1)
            res = O.losses(out, b64[2], b64[3], b64[4], K + 1)
            res["erank"] = O.effective_rank_torch(aux["fused"].reshape(-1, c.H))
            (res["loss"] - c.erank * res["erank"]).backward()
        else:
            res, out, aux = t64.step(batch, apply=False)
        aux32 = V.Trainer(p, K + 1, heads, 1, dtype=torch.float32).step(batch, apply=False)[2]
        return t64, res, out, aux, aux32
    kw = dict(bn_state=bn_state(c.H), bn_training=True) if c.variant == "bn" else {}
    tr = O.CpuTrainer({n: v.double() for n, v in p.items()}, K + 1, heads, 1, **kw)
    if c.erank:
        out, aux = O.forward(tr.p, (b64[0], b64[2]), b64[1], "train", K + 1, heads, 1, **kw)
        res = O.losses(out, b64[2], b64[3], b64[4], K + 1)
        res["erank"] = O.effective_rank_torch(aux["fused"].reshape(-1, c.H))
        (res["loss"] - c.erank * res["erank"]).backward()
    else:
        res, out, aux = tr.step(b64, apply=False)
    kw32 = dict(bn_state={k: v.float() if v.is_floating_point() else v for k, v in bn_state(c.H).items()},
                bn_training=True) if c.variant == "bn" else {}
    with torch.no_grad():
        _, aux32 = O.forward(p, (batch[0], batch[2]), batch[1], "train", K + 1, heads, 1, **kw32)
    return tr, res, out, aux, aux32


ADMITTED = [c for c in WC.CASES if c.refuse is None]
REFUSED = [c for c in WC.CASES if c.refuse is not None]


@pytest.mark.parametrize("c", ADMITTED, ids=WC.case_id)
def test_width_shape_against_fp64_oracle(c, oracle_lib, monkeypatch):
    t0 = time.time()
    B, S, H, K, heads = c.B, c.S, c.H, c.K, c.heads
    cid = WC.case_id(c)
    batch = WC.make_batch(c)
    p = params(c.variant, H, heads, K)
    tr, res, oout, oaux, aux32 = oracle64(c, batch, p)
    for k in ("idx_rgb", "idx_dep") if aux32 is not None else ():
        assert np.array_equal(np.sort(np.asarray(aux32[k])), np.sort(np.asarray(oaux[k]))), \
            f"{cid}: fp32 and fp64 oracles select different {k}"
    t_oracle = time.time() - t0
    model = build_model(c.variant, H, heads, K, p).eval()
    eng = model.engine()
    eng.defer_tail = True                 # the training flow's routing (train(), train_step())
    if c.erank:
        eng.erank_weight = c.erank
    d = [t.cuda() for t in batch]
    rec = Recorder(monkeypatch)
    fw = dict(bn_training=True) if c.variant == "bn" else {}
    eng.forward(d[0], d[1], d[2], "train", training=False, **fw)
    w = eng.last["w"]
    tail_deferred = bool(getattr(w, "_tail_deferred", False))
    loss, _ = eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    # ---- the path the row states
    names = rec.names()
    assert not eng._chain_ok(w) and not eng._dec_chain_ok(w), cid
    seams = {n for n in names if n in WC.SEAMS.values()}
    assert seams == ({WC.SEAMS[c.variant]} if c.seam else set()), (cid, names)          # exactly the row's own seam
    assert ("token_exchange_fwd" in names) == (c.variant == "tf" and not c.seam), (cid, names)
    assert ("colabssum" in names) == (c.variant == "vary"), (cid, names)     # train mode: only vary scores from |x|
    assert tail_deferred == c.tail1 and ("decoder_tail_losses" in names) == c.tail1, (cid, tail_deferred)
    assert ("decoder_tail_fwd" in names) == (not c.tail1), cid
    ca = [a for n, a in rec.calls if n == "mha_core_fwd" and a[7] == WC.Q and a[8] == S]
    assert ca, (cid, "no cross-attention core launch with Lk = S")
    dh = ca[0][9]
    assert dh == H // heads
    assert c.attn == ("small" if S <= 64 and dh in (16, 32, 64, 128) else "general"), cid
    assert eng._multi_stream() == c.side, cid
    # ---- selection, outputs, losses, gradients
    idx = eng.last["idx"]
    if c.variant == "plain":
        assert idx is None, cid
    else:
        assert np.array_equal(np.sort(idx[0].cpu().numpy()), np.sort(np.asarray(aux32["idx_rgb"]))), cid
        assert np.array_equal(np.sort(idx[1].cpu().numpy()), np.sort(np.asarray(aux32["idx_dep"]))), cid
    out = dict(seg=w.seg.view(B, S, K), action=w.actdur[:, :K].reshape(B, WC.Q, K),
               duration=w.actdur[:, K].reshape(B, WC.Q))
    for k in ("action", "duration", "seg"):
        close_rel(out[k], oout[k].detach(), f"{cid}/{k}")
    close_rel(w.fused.view(B, S, H), oaux["fused"].detach(), f"{cid}/fused")
    want = torch.stack([torch.as_tensor(res[k]).detach() for k in ("loss_seg", "loss_action", "loss_dur", "loss")])
    assert_close(loss.cpu(), want, 1e-3, 1e-6, f"{cid}/losses")
    if c.erank:
        er = float(res["erank"])
        assert abs(float(eng.erank_value()) - er) < 5e-3 * max(1.0, er / 50), (cid, float(eng.erank_value()), er)
    kink = ffn_kink_units(oaux["ffn_pre"]) if "ffn_pre" in oaux else set()
    assert len(kink) <= 4, f"{cid}: {len(kink)} FFN units on the ReLU kink"
    rtol = 2e-3 if not kink else 4e-3
    n_grads = 0
    for n, q in tr.p.items():
        if q.grad is None:
            continue
        g, r = without_kink_units(n, eng.arena.g(n).cpu(), q.grad, kink)
        if n == "fc_len.bias":
            # exactly zero (a shift of every duration cancels in the L1 normalisation): rounding noise on both sides
            assert float(g.abs().max()) <= 5e-4 * float(eng.arena.g("fc_len.weight").abs().max()), cid
        else:
            close_rel(g, r, f"{cid}/grad {n}" + (f" (kink units {sorted(kink)} excluded)" if kink else ""), rtol=rtol)
        n_grads += 1
    assert n_grads == len(eng.arena.live_names)
    if c.variant == "plain":
        assert "fuser.modality_token" in eng.arena.live_names, cid
    print(f"[width] {cid}: oracle {t_oracle:.1f} s, total {time.time() - t0:.1f} s")


def val_oracle(variant, p, batch, K, heads, st, dtype):
    """The oracle's validation forward (dropout off, no key padding mask) in `dtype`: (outputs, aux)."""
    q = {n: v.to(dtype) for n, v in p.items()}
    feats, depth, lab = batch[0].to(dtype), batch[1].to(dtype), batch[2]
    with torch.no_grad():
        if variant == "plain":
            return PO.forward(q, feats, depth, "val", K + 1, heads, 1)               # the bare tensor, as validate() passes
        if variant == "vary":
            return V.forward(q, (feats, lab), depth, "val", K + 1, heads, 1)
        kw = {}
        if variant == "bn":
            kw = dict(bn_state={k: v.to(dtype) if v.is_floating_point() else v.clone() for k, v in st.items()},
                      bn_training=False)
        return O.forward(q, (feats, lab), depth, "val", K + 1, heads, 1, **kw)


def _val_model(variant, H, heads, K, p, st):
    model = build_model(variant, H, heads, K, p).eval()
    if st is not None:                      # running statistics far from the fresh state
        sd = {k: v.float() if v.is_floating_point() else v for k, v in st.items()}
        model.load_state_dict(sd, strict=False)
        assert torch.equal(model.fuser.bn_depth.running_var.cpu(), sd["fuser.bn_depth.running_var"])
    return model


def _check_val(variant, c, batch, p, st, model, rec, tag):
    """validate()'s own forward against the fp64 oracle; for the selecting variants the fp32 oracle's channels, bit for bit."""
    B, S, K = c.B, c.S, c.K
    oout, oaux = val_oracle(variant, p, batch, K, c.heads, st, torch.float64)
    eng = model.engine()
    d = [t.cuda() for t in batch]
    out = eng.forward(d[0], d[1], d[2], "val", training=False, need_grad=False)
    out = {k: v.clone() for k, v in out.items()}
    torch.cuda.synchronize()
    names = rec.names()
    assert not eng._chain_ok(eng.last["w"]), tag
    if variant in ("tf", "vary"):           # the seam is train mode only: |x| column sums, then the selection from them
        assert "colabssum" in names and "embed_fuse_fwd" not in names, (tag, names)
        _, aux32 = val_oracle(variant, p, batch, K, c.heads, st, torch.float32)
        for j, k in enumerate(("idx_rgb", "idx_dep")):
            assert np.array_equal(np.sort(np.asarray(aux32[k])), np.sort(np.asarray(oaux[k]))), \
                f"{tag}: fp32 and fp64 oracles select different {k} (reseed the row)"
            assert np.array_equal(eng.last["idx"][j].cpu().numpy(), np.sort(np.asarray(aux32[k]))), (tag, k)
    else:
        assert "colabssum" not in names, (tag, names)
        assert ({n for n in names if n in WC.SEAMS.values()} == {WC.SEAMS[variant]}), (tag, names)
    for k in ("action", "duration", "seg"):
        close_rel(out[k], oout[k], f"{tag}/val {k}")
    return out


@pytest.mark.parametrize("v", WC.VAL_CASES, ids=WC.val_id)
def test_val_forward_against_fp64_oracle(v, oracle_lib, monkeypatch):
    t0 = time.time()
    variant, H, heads = v
    c = WC._c(2, 16, H, heads, variant=variant, pad="none")
    tag = WC.val_id(v)
    batch = WC.make_batch(c)
    p = params(variant, H, heads, c.K)
    st = bn_state(H, seed=H) if variant == "bn" else None
    model = _val_model(variant, H, heads, c.K, p, st)
    rec = Recorder(monkeypatch)
    out = _check_val(variant, c, batch, p, st, model, rec, tag)
    monkeypatch.undo()
    if variant == "plain":                  # the bare features and the (features, labels) tuple: the same forward
        d = [t.cuda() for t in batch]
        with torch.no_grad():
            bare = model(d[0], d[1], mode="val")
            tup = model((d[0], d[2]), d[1], mode="val")
        torch.cuda.synchronize()
        for k in ("action", "duration", "seg"):
            assert torch.equal(bare[k], tup[k]), (tag, k)
            assert torch.equal(bare[k], out[k]), (tag, k)
    if variant == "bn":                     # the eval state reads the running statistics and leaves them as they were
        assert torch.equal(model.fuser.bn_rgb.running_mean.cpu(), st["fuser.bn_rgb.running_mean"].float())
    print(f"[width] val {tag}: total {time.time() - t0:.1f} s")


@pytest.mark.parametrize("H,heads,last,first,limit", WC.VAL_CLIP_BOUNDS)
def test_val_forward_at_the_longest_forward_only_clip(H, heads, last, first, limit, oracle_lib, monkeypatch):
    """The longest clip a forward alone admits runs against the fp64 oracle; one frame more raises a ValueError naming the
    limit before anything is enqueued, and the engine is still usable."""
    from r3d_amd import engine as E
    t0 = time.time()
    assert min(E.max_clip_len(H, heads, WC.Q, ARGS.max_pos_len, False), ARGS.max_pos_len) == last
    c = WC._c(1, last, H, heads, pad="none")
    batch = WC.make_batch(c)
    p = params("tf", H, heads, c.K)
    model = _val_model("tf", H, heads, c.K, p, None)
    eng = model.engine()
    big = [t.cuda() for t in WC.make_batch(WC._c(1, first, H, heads, pad="none"))]
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match=limit):
        eng.forward(big[0], big[1], big[2], "val", training=False, need_grad=False)
    assert not rec.calls and not eng.shapes, rec.names()
    del big
    _check_val("tf", c, batch, p, None, model, rec, f"H{H}x{heads}-S{last}")
    print(f"[width] val H{H}x{heads} S{last}: total {time.time() - t0:.1f} s")


@pytest.mark.parametrize("c", [c for c in REFUSED if WC.engine_refused(c)], ids=WC.case_id)
def test_refused_engine_shapes_raise_at_construction(c, monkeypatch):
    model = build_model(c.variant, c.H, c.heads, c.K, params(c.variant, c.H, c.heads, c.K))
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match=c.refuse):
        model.engine()
    assert not rec.calls, rec.names()


def _admitted_batch(S, K=17, B=1, seed=5):
    return WC.make_batch(WC._c(B, S, 128, 8, K=K, pad="none"), seed=seed)


@pytest.mark.parametrize("c", [c for c in REFUSED if not WC.engine_refused(c)], ids=WC.case_id)
def test_refused_clip_lengths_raise_before_any_launch(c, monkeypatch):
    """The step raises before it enqueues anything; the same engine then runs an admitted shape exactly as a fresh one."""
    p = params(c.variant, c.H, c.heads, c.K)
    model = build_model(c.variant, c.H, c.heads, c.K, p).train()
    eng = model.engine()
    big = [t.cuda() for t in WC.make_batch(c)]
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match="clip length"):
        eng.train_step(big[0], big[1], big[2], big[3], big[4], 1e-3, 5e-3)
    assert not rec.calls, rec.names()
    assert not eng.shapes
    monkeypatch.undo()
    small = [t.cuda() for t in WC.make_batch(WC._c(1, 24, c.H, c.heads, variant=c.variant, pad="none"))]
    got = [x.clone() for x in eng.train_step(*small, 1e-3, 5e-3)] + [eng.arena.params.clone()]
    fresh = build_model(c.variant, c.H, c.heads, c.K, p).train().engine()
    want = [x.clone() for x in fresh.train_step(*small, 1e-3, 5e-3)] + [fresh.arena.params.clone()]
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_train_with_graph_replay_refuses_a_long_clip_before_capture(tmp_path, monkeypatch):
    """The refused clip length's step raises before it launches anything (a check that came from a kernel would come after
    the step's first launches) and before that shape is captured; the admitted shape before it was captured and replayed."""
    from r3d_amd.engine import FusionEngine
    from r3d_amd.train_proposed_depth import train
    from r3d_amd.optim import FlatAdamW, LinearWarmupCosineAnnealingLR
    K = 17
    p = params("tf", 128, 8, K)
    model = build_model("tf", 128, 8, K, p)
    batches = [_admitted_batch(16, seed=i) for i in range(3)] + [_admitted_batch(1606, seed=9)]
    rec = Recorder(monkeypatch)
    real_fb, real_graph = FusionEngine.forward_begin, torch.cuda.graph

    def forward_begin(self, feats, *a, **k):
        rec.calls.append(("forward_begin", (feats.shape[1],)))
        return real_fb(self, feats, *a, **k)

    def graph(*a, **k):
        rec.calls.append(("capture", ()))
        return real_graph(*a, **k)
    monkeypatch.setattr(FusionEngine, "forward_begin", forward_begin)
    monkeypatch.setattr(torch.cuda, "graph", graph)
    args = argparse.Namespace(epochs=1, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=1,
                              graph_steps=True)
    opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)
    sch = LinearWarmupCosineAnnealingLR(opt, warmup_epochs=2, max_epochs=4)
    sch.step()
    sch.step()
    with pytest.raises(ValueError, match="clip length 1606"):
        train(args, model, batches, opt, sch, None, str(tmp_path), K + 1, torch.device("cuda"), [batches[0]], seed=1)
    torch.cuda.synchronize()
    monkeypatch.undo()
    names = rec.names()
    assert names.count("capture") == 1, "only the admitted shape was captured"
    last = max(i for i, (n, a) in enumerate(rec.calls) if n == "forward_begin" and a[0] == 1606)
    assert names[last + 1:] == [], f"launched after the refused step began: {names[last + 1:]}"
    assert names.index("capture") < last
    assert all(k[1] == 16 for k in model.engine().shapes)


def test_rank_penalty_refuses_a_token_matrix_past_the_blocked_jacobi(monkeypatch):
    """B * S = 9600 fused tokens at hidden 128: admitted by the attention core (S = 1200), refused by the rank penalty's
    blocked Jacobi before anything is enqueued; without the penalty the same batch shape is admitted."""
    from r3d_amd import engine as E
    B, S, K = 8, 1200, 17
    E.check_clip_shape(S, 128, 8, WC.Q, 2000, True)
    model = build_model("tf", 128, 8, K, params("tf", 128, 8, K)).eval()
    eng = model.engine()
    eng.erank_weight = 0.05
    feats = torch.zeros(B, S, 2048, device="cuda")
    depth = torch.zeros(B, S, 224 * 224, device="cuda")
    lab = torch.full((B, S), K + 1, dtype=torch.int64, device="cuda")
    rec = Recorder(monkeypatch)
    with pytest.raises(ValueError, match="rank penalty"):
        eng.forward(feats, depth, lab, "train", training=False)
    assert not rec.calls and not eng.shapes, rec.names()


def test_side_stream_adamw_sees_this_steps_learning_rate():
    """H >= 512 with a depth AdamW that cannot be fused (B * S < 64): the small bucket's AdamW runs on the parameter-gradient
    stream.  A learning rate set in adamw() itself (as a torch optimiser wrapper does) must reach that stream: two steps
    with different rates equal, bit for bit, the same steps on one stream."""
    K = 17
    p = params("tf", 512, 8, K)
    d = [t.cuda() for t in WC.make_batch(WC._c(1, 24, 512, 8, pad="none"))]
    finals = []
    for side in (True, False):
        eng = build_model("tf", 512, 8, K, p).eval().engine()
        eng.auto_side_stream = side
        for lr in (1e-3, 3e-4):
            eng.forward(d[0], d[1], d[2], "train", training=False)
            eng.losses(d[2], d[4], d[3], tick=True)
            eng.backward(adamw_next=True)
            assert eng._tail_pending == side
            eng.adamw(lr, 5e-3, ticked=True)
        torch.cuda.synchronize()
        finals.append(eng.arena.params.clone())
    assert torch.equal(finals[0], finals[1]), float((finals[0] - finals[1]).abs().max())
