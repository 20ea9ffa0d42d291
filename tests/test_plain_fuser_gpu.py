"""The plain SA-Fuser model (model/futr_safuser_depth.py) through the HIP engine: step parity against the fixtures from the
imported reference and the CPU restatement (tests/plain_oracle.py), d modality_token against a float64 restatement and
from run to run, the validation forward, the hidden-128 chains against the composed path, the composed path at hidden
512, the shape refusals, graph replay, the rank penalty, train() with --erank_every, and two data-parallel ranks
(replicated, pixel-sharded, and the one-graph RCCL step flow)."""
import argparse
import contextlib
import io
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import futr_oracle as O, synth  # noqa: E402
from tests import plain_oracle as PO  # noqa: E402
from tests.helpers import load_fixture  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

TAGS = ["plain_tiny", "plain_cfg2", "plain_k122"]
HW = (120, 160)                     # the module's 160 * 120 depth projection


def _args():
    return argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")


def _model(params, H, K, pad_idx, n_dec=1, n_head=8):
    from r3d_amd.model.futr_safuser_depth import FUTR
    model = FUTR(K, H, pad_idx, torch.device("cuda"), _args(), n_query=8, n_head=n_head, num_encoder_layers=2,
                 num_decoder_layers=n_dec)
    missing = model.load_state_dict(params, strict=False)
    assert not missing.unexpected_keys and all("pos_table" in k for k in missing.missing_keys), missing
    return model.to("cuda")


def _batch(B, S, K, seed):
    return [torch.from_numpy(x) for x in synth.make_batch(B, S, K, K + 1, seed, depth_hw=HW)]


def _params(H, K, n_dec=1):
    """The analytic fill of the plain model's parameters at any shape."""
    from r3d_amd.model.futr_safuser_depth import FUTR
    m = FUTR(K, H, K + 1, torch.device("cpu"), _args(), n_query=8, n_head=8, num_encoder_layers=2, num_decoder_layers=n_dec)
    ns = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    return {n: torch.from_numpy(synth.fill_value(n, s, j)) for j, (n, s) in enumerate(ns)}


def _step(eng, d, mode="train"):
    out = eng.forward(d[0], d[1], d[2], mode, training=False)
    out = {k: v.clone() for k, v in out.items()}
    loss, counts = eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()
    return out, loss.clone(), counts.clone()


def _against_fp64(eng, t64, out, out64, what, rtol=2e-3):
    for k in ("action", "duration", "seg"):
        close_rel(out[k], out64[k].detach(), f"{what} {k}", rtol=1e-3)
    for n, q in t64.p.items():
        if q.grad is not None and n != "fc_len.bias":         # (fc_len.bias: exactly zero in exact arithmetic)
            close_rel(eng.arena.g(n), q.grad, f"{what} grad {n}", rtol=rtol)


@pytest.mark.parametrize("tag", TAGS)
def test_plain_step_parity(tag, oracle_lib):
    fx = load_fixture(tag)
    m = fx["meta"]
    H, K, L = m["H"], m["n_class"], m["n_dec"]
    batch = _batch(m["B"], m["S"], K, m["seed"])
    p = PO.plain_params(fx)
    tr = PO.Trainer(p, m["pad_idx"], 8, L)
    ores, oout, oaux = tr.step(batch, apply=False)
    t64 = PO.Trainer(p, m["pad_idx"], 8, L, dtype=torch.float64)
    t64.step(batch, apply=False)
    model = _model(p, H, K, m["pad_idx"], L).eval()
    eng = model.engine()
    assert eng.plain and not eng.bn and not eng.vary
    assert eng.arena.is_live("fuser.modality_token") and not eng.arena.is_live("fuser.projection.weight")
    d = [t.cuda() for t in batch]
    out, loss, counts = _step(eng, d)
    w = eng.last["w"]
    for k in ("action", "duration", "seg"):
        close_rel(out[k], oout[k].detach(), f"{tag}/{k} vs restatement", rtol=1e-3)
        close_rel(out[k], fx["out_" + k], f"{tag}/{k} vs reference fixture", rtol=1e-3)
    close_rel(w.fused.view(m["B"], m["S"], H), fx["fused"], f"{tag}/fused", rtol=1e-3)
    np.testing.assert_allclose(loss.cpu().numpy(), fx["losses"], rtol=1e-3, atol=1e-6)
    assert counts.cpu().tolist() == fx["counts"].tolist()
    for n in fx["live_names"]:
        close_rel(eng.arena.g(n), tr.p[n].grad, f"{tag}/grad {n}", rtol=2e-3)
    g_tok = eng.arena.g("fuser.modality_token").clone()
    close_rel(g_tok, fx["grad::fuser.modality_token"], f"{tag}/d token vs reference", rtol=2e-3)
    close_rel(g_tok, t64.p["fuser.modality_token"].grad, f"{tag}/d token vs fp64", rtol=2e-3)
    _step(eng, d)                                           # the same step again: d modality_token bit for bit
    assert torch.equal(eng.arena.g("fuser.modality_token"), g_tok)
    if (m["B"], m["S"], H) == (8, 16, 128):                 # the headline shape: both hidden-128 chains ran
        bf3 = bool(eng.chain_bf3)
        got = {k for k in w.tables if k[0] in ("fwd_chain", "bwd_chain", "dec_chain")}
        assert got == {("fwd_chain", False, bf3), ("bwd_chain", False, False, bf3), ("dec_chain", False, bf3)}, got


def test_plain_adamw_updates_the_token(oracle_lib):
    fx = load_fixture("plain_cfg2")
    m = fx["meta"]
    p = PO.plain_params(fx)
    model = _model(p, m["H"], m["n_class"], m["pad_idx"]).eval()
    eng = model.engine()
    d = [t.cuda() for t in _batch(m["B"], m["S"], m["n_class"], m["seed"])]
    before = eng.arena.p("fuser.modality_token").clone()
    proj = eng.arena.p("fuser.projection.weight").clone()
    _step(eng, d)
    eng.adamw(m["lr"], m["wd"])
    torch.cuda.synchronize()
    tr = PO.Trainer(p, m["pad_idx"], 8, 1, lr=m["lr"], wd=m["wd"], dtype=torch.float64)
    tr.step([t for t in _batch(m["B"], m["S"], m["n_class"], m["seed"])], apply=True)
    after = eng.arena.p("fuser.modality_token")
    assert not torch.equal(after, before)
    g64 = tr.p["fuser.modality_token"].grad
    keep = (g64.abs() > 1e-3 * float(g64.abs().max())).cpu()         # (AdamW's first step is ~ lr sign(g))
    close_rel((after - before).cpu()[keep], (tr.p["fuser.modality_token"] - p["fuser.modality_token"].double()).detach()[keep],
              "AdamW step of the token", rtol=2e-2)
    assert torch.equal(eng.arena.p("fuser.projection.weight"), proj)        # still dead


def test_plain_val_forward_bare_tensor_tuple_and_predict(oracle_lib):
    from r3d_amd.predict import predict_clip
    fx = load_fixture("plain_cfg2")
    m = fx["meta"]
    batch = _batch(m["B"], m["S"], m["n_class"], m["seed"])
    model = _model(PO.plain_params(fx), m["H"], m["n_class"], m["pad_idx"]).eval()
    d = [t.cuda() for t in batch]
    with torch.no_grad():
        bare = model(d[0], d[1], mode="val")
        tup = model((d[0], d[2]), d[1], mode="val")
    torch.cuda.synchronize()
    for k in ("action", "duration", "seg"):
        close_rel(bare[k], fx["val_" + k], f"val {k} (bare tensor)", rtol=1e-3)
        assert torch.equal(bare[k], tup[k]), k
    r = predict_clip(model, d[0][1], d[1][1], 20)
    for k in ("action", "duration", "seg"):
        close_rel(r["outputs"][k][0], fx["val_" + k][1], f"predict_clip {k}", rtol=1e-3)


def _snapshot(eng, d, flags):
    for k, v in flags.items():
        setattr(eng, k, v)
    eng.drop_offset.zero_()
    for w in eng.shapes.values():
        w.tables.clear()
    eng.forward(d[0], d[1], d[2], "train", training=True)
    loss, counts = eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()
    w = eng.last["w"]
    return dict(w=w, loss=loss.clone(), fused=w.fused.clone(), grads=eng.arena.grads.clone(),
                chains={k for k in w.tables if k[0] in ("fwd_chain", "bwd_chain", "dec_chain")})


@pytest.mark.parametrize("B,S,K", [(8, 16, 17), (8, 32, 122), (5, 16, 17)])
def test_plain_chain_vs_composed_and_bf3_vs_fp32(B, S, K):
    """Dropout on: the chains (bf16x3 and fp32) against the composed path, every gradient."""
    batch = _batch(B, S, K, 21 + B + S)
    model = _model(_params(128, K), 128, K, K + 1).train()
    eng = model.engine()
    d = [t.cuda() for t in batch]
    off = dict(use_fuser_chain=False, use_decoder_chain=False, chain_bf3=True, defer_tail=False)
    on = dict(off, use_fuser_chain=True, use_decoder_chain=True)
    a = _snapshot(eng, d, off)
    assert not a["chains"]
    b = _snapshot(eng, d, on)
    fc = eng._chain_ok(b["w"])
    assert fc == (B == 8)                            # (B = 5: 40 query rows, not whole 16-row tiles: composed fuser)
    if fc:
        assert ("fwd_chain", True, True) in b["chains"] and any(k[0] == "bwd_chain" for k in b["chains"]), b["chains"]
    assert (("dec_chain", True, True) in b["chains"]) == eng._dec_chain_ok(b["w"]), b["chains"]
    c = _snapshot(eng, d, dict(on, chain_bf3=False))
    if fc:
        assert ("bwd_chain", True, False, False) in c["chains"], c["chains"]
    for name, x, y in (("chain vs composed", a, b), ("fp32 vs bf16x3 chain", b, c)):
        close_rel(y["fused"], x["fused"], f"{name}: fused", rtol=5e-5)
        close_rel(y["loss"], x["loss"], f"{name}: loss", rtol=1e-5)
        for n in eng.arena.live_names:
            o, k, _ = eng.arena.offsets[n]
            if n == "fc_len.bias":
                continue                  # exactly zero in exact arithmetic (see test_chain_shapes_gpu)
            close_rel(y["grads"][o:o + k], x["grads"][o:o + k], f"{name}: grad {n}", rtol=5e-4)


def test_plain_ragged_odd_clip_length_against_restatement(oracle_lib):
    """Clips of different lengths (padding frames with pad_idx labels), an odd clip length."""
    K = 17
    batch = _batch(8, 15, K, 77)
    lab = batch[2]
    for b, n in enumerate((15, 1, 2, 14, 9, 15, 4, 12)):
        lab[b, n:] = K + 1
        batch[0][b, n:] = 0
        batch[1][b, n:] = 0
    p = _params(128, K)
    t64 = PO.Trainer(p, K + 1, 8, 1, dtype=torch.float64)
    res, out64, aux = t64.step(batch, apply=False)
    model = _model(p, 128, K, K + 1).eval()
    eng = model.engine()
    out, loss, _ = _step(eng, [t.cuda() for t in batch])
    _against_fp64(eng, t64, out, out64, "ragged")


def test_plain_composed_path_at_hidden_512(oracle_lib):
    K = 17
    batch = _batch(4, 8, K, 31)
    p = _params(512, K)
    t64 = PO.Trainer(p, K + 1, 8, 1, dtype=torch.float64)
    res, out64, aux = t64.step(batch, apply=False)
    model = _model(p, 512, K, K + 1).eval()
    eng = model.engine()
    out, loss, _ = _step(eng, [t.cuda() for t in batch])
    assert not eng._chain_ok(eng.last["w"])
    _against_fp64(eng, t64, out, out64, "H512")


def test_plain_refuses_hidden_past_the_seam_without_launching(monkeypatch):
    from r3d_amd import ops
    from r3d_amd.model.futr_safuser_depth import FUTR
    calls = []
    real = ops.check
    monkeypatch.setattr(ops, "check", lambda *a, **k: (calls.append(a), real(*a, **k))[1])
    model = FUTR(17, 1040, 18, torch.device("cuda"), _args(), n_query=8, n_head=16, num_encoder_layers=2,
                 num_decoder_layers=1).to("cuda")
    with pytest.raises(ValueError, match="plain SA-Fuser"):
        model.engine()
    assert model._engine is None and not calls


def test_plain_graph_replay_equals_eager():
    """train()'s graphed step (r3d_amd.train_proposed_depth._GraphedSteps) over several batches, constant lr, dropout on,
    against the same steps enqueued eagerly on a second engine: parameters bitwise equal, the token trained."""
    from r3d_amd.train_proposed_depth import _GraphedSteps
    K = 17
    p = _params(128, K)
    batches = [[t.cuda() for t in _batch(8, 16, K, 100 + i)] for i in range(4)]
    engs = []
    for graphed in (True, False):
        model = _model(p, 128, K, K + 1).train()
        eng = model.engine()
        eng.defer_tail = True
        acc_l = torch.zeros(4, dtype=torch.float64, device="cuda")
        acc_c = torch.zeros(4, dtype=torch.int64, device="cuda")
        gs = _GraphedSteps(eng, acc_l, acc_c, None, K + 1)
        hyper = (5e-3, (0.9, 0.999), 1e-8)
        for b in batches:
            if graphed:
                gs.step(b, 1e-3, hyper, True)
            else:
                eng._drop_ready = None
                gs._enqueue(b, 1e-3, hyper, True)
            torch.cuda.synchronize()
        if graphed:
            assert all(st["graph"] is not None for st in gs.shapes.values())      # steps 2.. replayed a capture
        engs.append(eng)
    a, b = engs
    assert torch.equal(a.arena.params, b.arena.params)
    tok0 = p["fuser.modality_token"].cuda()
    assert float((a.arena.p("fuser.modality_token") - tok0).abs().max()) > 1e-4        # the token trained


def test_plain_erank_penalty_gradients(oracle_lib):
    lam = 0.05
    K = 17
    batch = _batch(8, 16, K, 55)
    p = _params(128, K)
    t64 = PO.Trainer(p, K + 1, 8, 1, dtype=torch.float64, erank_weight=lam)
    res, out64, aux = t64.step(batch, apply=False)
    model = _model(p, 128, K, K + 1).eval()
    eng = model.engine()
    eng.erank_weight = lam
    _step(eng, [t.cuda() for t in batch])
    er = float(aux["erank"])
    assert abs(float(eng.erank_value()) - er) < 5e-3 * max(1.0, er / 50)
    for n, q in t64.p.items():
        if q.grad is not None and n != "fc_len.bias":
            close_rel(eng.arena.g(n), q.grad, f"erank grad {n}", rtol=1e-2)


def test_plain_train_loop_prints_the_effective_rank(tmp_path):
    from r3d_amd.train_proposed_depth import train
    from r3d_amd.optim import FlatAdamW
    K = 17
    model = _model(_params(128, K), 128, K, K + 1)
    batches = [_batch(8, 16, K, 400 + i) for i in range(3)]
    val = [[t[:1] for t in _batch(2, 16, K, 999)]]
    args = argparse.Namespace(epochs=1, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=1,
                              erank_every=1)

    class NoSched:
        def step(self):
            pass
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train(args, model, batches, FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3), NoSched(), None, str(tmp_path),
              K + 1, torch.device("cuda"), val, seed=0)
    torch.cuda.synchronize()
    printed = [float(x) for x in re.findall(r"effective rank of fused tokens: ([0-9.]+)", buf.getvalue())]
    assert len(printed) == 3, buf.getvalue()
    fused = model.engine().shapes[(8, 16, True)].fused
    ref = O.effective_rank(fused.cpu())
    assert abs(printed[-1] - ref) <= 0.5, (printed, ref)


# ---- two data-parallel ranks on one GPU (gloo) ----------------------------------------------------------------------------
def _dp_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import datetime
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        torch.cuda.set_device(0)
        from r3d_amd.parallel import DataParallelStep, RcclStep
        from tests.test_parallel_gpu import _DistAsRccl
        K, B, S = 17, 4, 16
        gb = _batch(world * B, S, K, 91)
        p = _params(128, K)
        tr = PO.Trainer(p, K + 1, 8, 1)
        tr.step(gb, apply=False)                                 # one process on the concatenated batch
        mine = [t[rank * B:(rank + 1) * B].cuda() for t in gb]
        losses = {}
        for shard in (False, True):
            model = _model(p, 128, K, K + 1).eval()
            eng = model.engine()
            dp = DataParallelStep(eng, pixel_shard=shard)
            dp.prepare_duration_denominator(mine[3], K + 1)
            eng.forward(mine[0], mine[1], mine[2], "train", training=False)
            loss, _ = eng.losses(mine[2], mine[4], mine[3])
            eng.backward()
            dp.wait_grads()
            torch.cuda.synchronize()
            losses[shard] = loss.clone()
            for n, g in tr.p.items():
                if g.grad is None or n == "fc_len.bias":
                    continue
                if shard and n == "depth_projection.weight":
                    got = dp.tp.g * dp.grad_scale                 # this rank's pixel columns
                    close_rel(got, g.grad[:, dp.tp.p0:dp.tp.p0 + dp.tp.Pr], "pixel-sharded grad depth_projection.weight",
                              rtol=2e-3)
                    continue
                close_rel(eng.arena.g(n) * dp.grad_scale, g.grad, f"dp (shard={shard}) grad {n}", rtol=2e-3)
        # the one-graph RCCL step flow (a torch.distributed stand-in for the RCCL binding), replicated and pixel-sharded
        for shard in (False, True):
            model = _model(p, 128, K, K + 1).eval()
            eng = model.engine()
            dp = DataParallelStep(eng, pixel_shard=shard)
            dp.broadcast_parameters()
            rs = RcclStep(dp, _DistAsRccl(), _DistAsRccl(), 1e-3, 5e-3)
            rs.stage(mine[1].reshape(B * S, -1), mine[3], K + 1, 0)
            rs.run(mine[0], mine[1], mine[2], mine[3], mine[4], K + 1, False, slot=0)
            torch.cuda.synchronize()
            close_rel(eng.last["w"].loss, losses[False], f"RcclStep (shard={shard}) loss", rtol=1e-4)
            tok = eng.arena.p("fuser.modality_token")
            assert not torch.equal(tok, p["fuser.modality_token"].cuda())           # the AdamW inside the step moved it
            t = tok.clone()
            dist.broadcast(t, src=0)
            assert torch.equal(t, tok)                                             # the ranks agree bit for bit
        q.put((rank, "ok", ""))
    except Exception as e:          # noqa: BLE001
        import traceback
        q.put((rank, "fail", traceback.format_exc() + repr(e)))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_plain_data_parallel_two_ranks(oracle_lib):
    """2 ranks on one GPU (gloo): the averaged gradients (replicated and pixel-sharded) equal the restatement's on the
    concatenated batch; the RcclStep flow runs both ways and keeps the ranks' tokens equal."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=600) for _ in procs]
    for pr in procs:
        pr.join(timeout=60)
    for rank, status, info in res:
        assert status == "ok", f"rank {rank}: {info}"
