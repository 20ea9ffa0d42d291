"""The activation-magnitude fuser variant (model/futr_safuser_tokenfusion_vary.py) through the HIP engine: step parity
against the fixtures from the imported reference and the CPU restatement (tests/vary_oracle.py), d alpha against a
float64 restatement, the hidden-128 chains on the variant, the composed path at hidden 512, graph replay of the training
step with per-batch selection, the validation forward, the rank penalty and two data-parallel ranks."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import futr_oracle as O, synth  # noqa: E402
from tests import vary_oracle as V  # noqa: E402
from tests.helpers import load_fixture  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

TAGS = ["vary_tiny", "vary_cfg2", "vary_k122"]


def _args():
    return argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")


def _model(params, H, K, pad_idx):
    from r3d_amd.model.futr_safuser_tokenfusion_vary import FUTR
    model = FUTR(K, H, pad_idx, torch.device("cuda"), _args(), n_query=8, n_head=8, num_encoder_layers=2,
                 num_decoder_layers=1)
    missing = model.load_state_dict(params, strict=False)
    assert not missing.unexpected_keys and all("pos_table" in k for k in missing.missing_keys), missing
    return model.to("cuda")


def _batch(B, S, K, seed, **kw):
    return [torch.from_numpy(x) for x in synth.make_batch(B, S, K, K + 1, seed, **kw)]


def _params(H, K):
    """The analytic fill of the variant's parameters at any shape (fuser.alpha in [0.5, 0.95])."""
    from r3d_amd.model.futr_safuser_tokenfusion_vary import FUTR
    m = FUTR(K, H, K + 1, torch.device("cpu"), _args(), n_query=8, n_head=8, num_encoder_layers=2, num_decoder_layers=1)
    ns = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    return {n: torch.from_numpy(synth.fill_value(n, s, j)) for j, (n, s) in enumerate(ns)}


def _step(eng, d, mode="train"):
    out = eng.forward(d[0], d[1], d[2], mode, training=False)
    out = {k: v.clone() for k, v in out.items()}
    loss, counts = eng.losses(d[2], d[4], d[3])
    eng.backward()
    torch.cuda.synchronize()
    return out, loss.clone(), counts.clone()


@pytest.mark.parametrize("tag", TAGS)
def test_vary_step_parity(tag, oracle_lib):
    fx = load_fixture(tag)
    m = fx["meta"]
    H, K = m["H"], m["n_class"]
    batch = _batch(m["B"], m["S"], K, m["seed"])
    p = V.vary_params(fx)
    tr = V.Trainer(p, m["pad_idx"], 8, 1)
    ores, oout, oaux = tr.step(batch, apply=False)
    t64 = V.Trainer(p, m["pad_idx"], 8, 1, dtype=torch.float64)
    t64.step(batch, apply=False)
    model = _model(p, H, K, m["pad_idx"]).eval()
    eng = model.engine()
    assert eng.vary and not eng.bn and not eng.use_fused_embed
    d = [t.cuda() for t in batch]
    out, loss, counts = _step(eng, d)
    w = eng.last["w"]
    assert np.array_equal(np.sort(eng.last["idx"][0].cpu().numpy()), fx["idx_rgb"])      # bit-exact, ties included
    assert np.array_equal(np.sort(eng.last["idx"][1].cpu().numpy()), fx["idx_dep"])
    for k in ("action", "duration", "seg"):
        close_rel(out[k], oout[k].detach(), f"{tag}/{k} vs restatement")
        close_rel(out[k], fx["out_" + k], f"{tag}/{k} vs reference fixture")
    close_rel(w.fused.view(m["B"], m["S"], H), fx["fused"], f"{tag}/fused")
    np.testing.assert_allclose(loss.cpu().numpy(), fx["losses"], rtol=1e-3, atol=1e-6)
    assert counts.cpu().tolist() == fx["counts"].tolist()
    for n in fx["live_names"]:
        close_rel(eng.arena.g(n), tr.p[n].grad, f"{tag}/grad {n}", rtol=2e-3)
    close_rel(eng.arena.g("fuser.alpha"), fx["grad::fuser.alpha"], f"{tag}/d alpha vs reference", rtol=2e-3)
    close_rel(eng.arena.g("fuser.alpha"), t64.p["fuser.alpha"].grad, f"{tag}/d alpha vs fp64", rtol=2e-3)
    if (m["B"], m["S"], H) == (8, 16, 128):            # the headline shape: both hidden-128 chains ran
        bf3 = bool(eng.chain_bf3)
        got = {k for k in w.tables if k[0] in ("fwd_chain", "bwd_chain", "dec_chain")}
        assert got == {("fwd_chain", False, bf3), ("bwd_chain", False, False, bf3), ("dec_chain", False, bf3)}, got


def test_vary_val_mode_forward(oracle_lib):
    fx = load_fixture("vary_cfg2")
    m = fx["meta"]
    batch = _batch(m["B"], m["S"], m["n_class"], m["seed"])
    model = _model(V.vary_params(fx), m["H"], m["n_class"], m["pad_idx"]).eval()
    d = [t.cuda() for t in batch]
    with torch.no_grad():
        out = model((d[0], d[2]), d[1], mode="val")
    torch.cuda.synchronize()
    eng = model.engine()
    assert np.array_equal(np.sort(eng.last["idx"][0].cpu().numpy()), fx["val_idx_rgb"])
    assert np.array_equal(np.sort(eng.last["idx"][1].cpu().numpy()), fx["val_idx_dep"])
    for k in ("action", "duration", "seg"):
        close_rel(out[k], fx["val_" + k], f"val {k}")


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
def test_vary_chain_vs_composed_and_bf3_vs_fp32(B, S, K):
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


def test_vary_ragged_batch_against_restatement(oracle_lib):
    """Clips of different lengths (padding frames with pad_idx labels) at the headline shape."""
    K = 17
    batch = _batch(8, 16, K, 77)
    lab = batch[2]
    for b, n in enumerate((16, 1, 2, 15, 9, 16, 4, 12)):
        lab[b, n:] = K + 1
        batch[0][b, n:] = 0
        batch[1][b, n:] = 0
    p = _params(128, K)
    t64 = V.Trainer(p, K + 1, 8, 1, dtype=torch.float64)
    res, out64, aux = t64.step(batch, apply=False)
    model = _model(p, 128, K, K + 1).eval()
    eng = model.engine()
    out, loss, _ = _step(eng, [t.cuda() for t in batch])
    assert np.array_equal(np.sort(eng.last["idx"][0].cpu().numpy()), aux["idx_rgb"].numpy())
    for k in ("action", "duration", "seg"):
        close_rel(out[k], out64[k].detach(), f"ragged {k}", rtol=1e-3)
    for n, q in t64.p.items():
        if q.grad is not None and n != "fc_len.bias":
            close_rel(eng.arena.g(n), q.grad, f"ragged grad {n}", rtol=2e-3)


def test_vary_composed_path_at_hidden_512(oracle_lib):
    K = 17
    batch = _batch(4, 8, K, 31)
    p = _params(512, K)
    t64 = V.Trainer(p, K + 1, 8, 1, dtype=torch.float64)
    res, out64, aux = t64.step(batch, apply=False)
    model = _model(p, 512, K, K + 1).eval()
    eng = model.engine()
    out, loss, _ = _step(eng, [t.cuda() for t in batch])
    assert not eng._chain_ok(eng.last["w"])
    assert np.array_equal(np.sort(eng.last["idx"][0].cpu().numpy()), aux["idx_rgb"].numpy())
    assert np.array_equal(np.sort(eng.last["idx"][1].cpu().numpy()), aux["idx_dep"].numpy())
    for k in ("action", "duration", "seg"):
        close_rel(out[k], out64[k].detach(), f"H512 {k}", rtol=1e-3)
    for n, q in t64.p.items():
        if q.grad is not None and n != "fc_len.bias":
            close_rel(eng.arena.g(n), q.grad, f"H512 grad {n}", rtol=2e-3)


def test_vary_graph_replay_equals_eager_and_masks_follow_the_batch():
    """train()'s graphed step (r3d_amd.train_proposed_depth._GraphedSteps) over several batches, constant lr, dropout on,
    against the same steps enqueued eagerly on a second engine: parameters bitwise equal; the selection changes between
    batches, so a mask frozen at capture time would fail."""
    from r3d_amd.train_proposed_depth import _GraphedSteps
    K = 17
    p = _params(128, K)
    batches = [[t.cuda() for t in _batch(8, 16, K, 100 + i)] for i in range(5)]
    for i, b in enumerate(batches):              # a different set of weak RGB channels per batch
        b[0][..., :] *= 1.0 + 0.5 * torch.sin(torch.arange(2048, device="cuda", dtype=torch.float32) * (0.37 + 0.11 * i))
    engs, masks = [], []
    for graphed in (True, False):
        model = _model(p, 128, K, K + 1).train()
        eng = model.engine()
        eng.defer_tail = True
        acc_l = torch.zeros(4, dtype=torch.float64, device="cuda")
        acc_c = torch.zeros(4, dtype=torch.int64, device="cuda")
        gs = _GraphedSteps(eng, acc_l, acc_c, None, K + 1)
        hyper = (5e-3, (0.9, 0.999), 1e-8)
        ms = []
        for b in batches:
            if graphed:
                gs.step(b, 1e-3, hyper, True)
            else:
                eng._drop_ready = None
                gs._enqueue(b, 1e-3, hyper, True)
            torch.cuda.synchronize()
            ms.append(eng.last["w"].mask.clone())
        if graphed:
            assert all(st["graph"] is not None for st in gs.shapes.values())      # steps 2.. replayed a capture
        engs.append(eng)
        masks.append(ms)
    a, b = engs
    assert torch.equal(a.arena.params, b.arena.params)
    assert all(torch.equal(x, y) for x, y in zip(masks[0], masks[1]))
    assert sum(not torch.equal(masks[0][i], masks[0][i + 1]) for i in range(len(batches) - 1)) >= 2
    assert float((a.arena.p("fuser.alpha") - 1).abs().max()) > 0


def test_vary_erank_penalty_gradients(oracle_lib):
    lam = 0.05
    K = 17
    batch = _batch(8, 16, K, 55)
    p = _params(128, K)
    t64 = V.Trainer(p, K + 1, 8, 1, dtype=torch.float64)
    b = [t.double() if t.is_floating_point() else t for t in batch]
    out, aux = V.forward(t64.p, (b[0], b[2]), b[1], "train", K + 1, 8, 1)
    res = O.losses(out, b[2], b[3], b[4], K + 1)
    er = O.effective_rank_torch(aux["fused"].reshape(-1, 128))
    (res["loss"] - lam * er).backward()
    model = _model(p, 128, K, K + 1).eval()
    eng = model.engine()
    eng.erank_weight = lam
    _step(eng, [t.cuda() for t in batch])
    assert abs(float(eng.erank_value()) - float(er)) < 5e-3 * max(1.0, float(er) / 50)
    for n, q in t64.p.items():
        if q.grad is not None and n != "fc_len.bias":
            close_rel(eng.arena.g(n), q.grad, f"erank grad {n}", rtol=1e-2)


def _dp_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        from r3d_amd.parallel import DataParallelStep
        K, B = 17, 4
        gb = _batch(world * B, 16, K, 91)
        p = _params(128, K)
        tr = V.Trainer(p, K + 1, 8, 1)
        res, out, aux = tr.step(gb, apply=False)                 # one process on the concatenated batch
        model = _model(p, 128, K, K + 1).eval()
        eng = model.engine()
        dp = DataParallelStep(eng)
        with pytest.raises(NotImplementedError):
            DataParallelStep(_model(p, 128, K, K + 1).engine(), pixel_shard=True)
        mine = [t[rank * B:(rank + 1) * B].cuda() for t in gb]
        dp.prepare_duration_denominator(mine[3], K + 1)
        eng.forward(mine[0], mine[1], mine[2], "train", training=False)
        eng.losses(mine[2], mine[4], mine[3])
        eng.backward()
        dp.wait_grads()
        torch.cuda.synchronize()
        assert np.array_equal(np.sort(eng.last["idx"][0].cpu().numpy()), aux["idx_rgb"].numpy())
        assert np.array_equal(np.sort(eng.last["idx"][1].cpu().numpy()), aux["idx_dep"].numpy())
        for n, g in tr.p.items():
            if g.grad is not None and n != "fc_len.bias":
                close_rel(eng.arena.g(n) * dp.grad_scale, g.grad, f"dp grad {n}", rtol=2e-3)
        q.put((rank, "ok", ""))
    except Exception as e:          # noqa: BLE001
        import traceback
        q.put((rank, "fail", traceback.format_exc() + repr(e)))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_vary_data_parallel_two_ranks(oracle_lib):
    """2 ranks on one GPU (gloo): global-batch scores through score_allreduce; the averaged gradients equal the
    restatement's on the concatenated batch."""
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
