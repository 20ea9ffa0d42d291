"""The streaming effective-rank measurement on the device, against float64.

Kernel rows (tests/rank_cases.py): the rows go through StreamingRank.update() in the row's chunks and lanes; R is merged on
the device, read back, and its singular values -- taken on the CPU in float64 -- are held against float64 svdvals of the
valid rows at the project's tolerances (rtol 1e-4, atol 1e-4 sigma_max; surplus sigma <= 1e-5 sigma_max when N < H);
finalize()["erank"] (the device Jacobi on the merged R) within 5e-3 max(1, er / 50) of the float64 effective rank; rows
equals the count of valid rows; the strictly lower triangle of every lane's R is exactly zero.
Further: empty lanes, n = 0, padded rows (NaN behind the padding labels), an all-padding chunk, bit reproducibility,
refusals.  Model level: measure_rank over a ragged three-batch loader against float64 svdvals of the engine's own
w.rgb / w.dep / w.fused (copied out per batch), on the hidden-128 chain route, the composed route and the BN-blend,
activation-magnitude and plain models; the query models and data-parallel runs are refused; train() with --erank_report prints the lines of the run without it plus one rank line per
epoch, whose numbers are measure_rank's."""
import argparse
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import rank_cases as RC  # noqa: E402
from tests import rank_oracle as RO  # noqa: E402
from tests import width_cases as WC  # noqa: E402

ARGS = argparse.Namespace(input_dim=2048, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")
K = 17
PAD = K + 1


@pytest.fixture(scope="module")
def ops():
    from r3d_amd import ops
    return ops


def _merged(ops, acc):
    """The merged triangle of an accumulator (on a copy), and every lane's R, on the host."""
    R = acc.R.clone()
    ops.qr_merge(R)
    torch.cuda.synchronize()
    return R[0].cpu().numpy(), acc.R.cpu().numpy()


def _feed(acc, xd, chunk, labels=None, pad_idx=None):
    n = xd.shape[0]
    chunk = n if chunk is None else chunk
    for c0 in range(0, n, chunk):
        acc.update(xd[c0:c0 + chunk], None if labels is None else labels[c0:c0 + chunk], pad_idx)


@pytest.mark.parametrize("c", RC.CASES, ids=RC.case_id)
def test_kernel_row_against_fp64(ops, c):
    from r3d_amd.rankstream import StreamingRank
    t0 = time.time()
    T = ops.qr_append_tile_rows(c.H)
    N = RC.resolve_n(c, T)
    x = RO.make_input(c.input, N, c.H, seed=N + 7 * c.H).astype(np.float32)
    if c.ldx:                                            # a column slice of a wider matrix, NaN around it
        big = torch.full((N, c.ldx), float("nan"), device="cuda")
        big[:, 9:9 + c.H] = torch.from_numpy(x).cuda()
        xd = big[:, 9:9 + c.H]
        assert xd.stride(0) == c.ldx
    else:
        xd = torch.from_numpy(x).cuda()
    acc = StreamingRank(c.H, "cuda", lanes=c.lanes)
    _feed(acc, xd, c.chunk)
    res = acc.finalize()
    R, lanes_R = _merged(ops, acc)
    assert np.isfinite(lanes_R).all()
    assert not np.tril(lanes_R, -1).any(), "a lane's strictly lower triangle is not zero"
    worst, er_ref = RO.check_against_fp64(R, x, RC.case_id(c))
    print(f"[rank row {RC.case_id(c)} N {N} T {T}] sigma err/max {worst:.2e}, erank {res['erank']:.5f} vs {er_ref:.5f} "
          f"({time.time() - t0:.1f} s)")
    assert res["rows"] == N
    assert res["sigma"].shape == (c.H,)
    assert abs(res["erank"] - er_ref) <= RC.erank_tol(er_ref), (res["erank"], er_ref)
    # finalize() merged a scratch copy: accumulation can go on, and a second finalize() says the same
    assert np.array_equal(acc.R.cpu().numpy(), lanes_R)
    assert acc.finalize()["erank"] == res["erank"]


def test_empty_lanes_and_empty_calls(ops):
    from r3d_amd.rankstream import StreamingRank
    H = 16
    x = torch.from_numpy(RO.make_input("gauss", 3, H, seed=3).astype(np.float32)).cuda()
    acc = StreamingRank(H, "cuda", lanes=8)
    acc.update(x)
    torch.cuda.synchronize()
    assert acc.rows.cpu().tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert not acc.R[3:].any(), "a lane without rows must leave its R zero"
    before = acc.R.clone()
    acc.update(x[:0])                                    # n = 0: a no-op
    acc.update(torch.empty(0, 4, H, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(acc.R, before) and int(acc.rows.sum()) == 3
    res = acc.finalize()
    assert res["rows"] == 3
    R, _ = _merged(ops, acc)
    _, er_ref = RO.check_against_fp64(R, x.cpu().numpy(), "3 rows over 8 lanes")
    assert abs(res["erank"] - er_ref) <= RC.erank_tol(er_ref)
    acc.reset()
    assert not acc.R.any() and not acc.rows.any()
    empty = acc.finalize()
    assert empty["rows"] == 0 and empty["erank"] == 0.0 and empty["sigma"].shape == (H,) and not empty["sigma"].any()


def test_padded_rows_are_left_out(ops):
    from r3d_amd.rankstream import StreamingRank
    B, S, H, lens = 3, 40, 128, (40, 17, 1)
    x = RO.make_input("gauss", B * S, H, seed=58).astype(np.float32).reshape(B, S, H)
    lab = np.zeros((B, S), dtype=np.int64)
    for b, n in enumerate(lens):
        lab[b, :n] = np.arange(n) % K
        lab[b, n:] = PAD
        x[b, n:] = np.nan                                # a padded row is never read: staged as zeros
    valid = x[lab != PAD]
    assert valid.shape == (58, H)
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    acc = StreamingRank(H, "cuda", lanes=4)
    acc.update(xd, ld, PAD)                              # [B, S, H] with [B, S] labels
    res = acc.finalize()
    R, lanes_R = _merged(ops, acc)
    assert np.isfinite(lanes_R).all()
    _, er_ref = RO.check_against_fp64(R, valid, "masked [3, 40, 128]")
    assert res["rows"] == 58
    assert abs(res["erank"] - er_ref) <= RC.erank_tol(er_ref), (res["erank"], er_ref)
    # a chunk whose rows are all padding leaves R bit-identical (and counts nothing)
    before, rows_before = acc.R.clone(), acc.rows.clone()
    acc.update(xd[2, 1:], ld[2, 1:], PAD)
    acc.update(torch.full((600, H), float("nan"), device="cuda"), torch.full((600,), PAD, dtype=torch.int64, device="cuda"), PAD)
    torch.cuda.synchronize()
    assert torch.equal(acc.R, before) and torch.equal(acc.rows, rows_before)
    # the same rows, flat and without labels, give the same singular values
    acc2 = StreamingRank(H, "cuda", lanes=4)
    acc2.update(torch.from_numpy(valid).cuda())
    R2, _ = _merged(ops, acc2)
    RO.check_against_fp64(R2, valid, "the 58 valid rows")


def test_same_calls_same_bits(ops):
    from r3d_amd.rankstream import StreamingRank
    x = torch.from_numpy(RO.make_input("relu", 500, 136, seed=11).astype(np.float32)).cuda()
    outs = []
    for _ in range(2):
        acc = StreamingRank(136, "cuda", lanes=3)
        _feed(acc, x, 77)
        R = acc.R.clone()
        ops.qr_merge(R)
        res = acc.finalize()
        torch.cuda.synchronize()
        outs.append((acc.R.clone(), R, res))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2]["erank"] == outs[1][2]["erank"] and torch.equal(outs[0][2]["sigma"], outs[1][2]["sigma"])


def test_update_replayed_from_a_graph_equals_eager():
    """update() only enqueues: captured once and replayed, it accumulates what the same calls do eagerly, bit for bit."""
    from r3d_amd.rankstream import StreamingRank
    x = torch.from_numpy(RO.make_input("gauss", 200, 128, seed=5).astype(np.float32)).cuda()
    lab = torch.zeros(200, dtype=torch.int64, device="cuda")
    lab[150:] = PAD
    eager, graphed = StreamingRank(128, "cuda", lanes=4), StreamingRank(128, "cuda", lanes=4)
    for _ in range(3):
        eager.update(x, lab, PAD)
    graphed.update(x, lab, PAD)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        graphed.update(x, lab, PAD)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager.R, graphed.R) and torch.equal(eager.rows, graphed.rows)
    assert int(graphed.rows.sum()) == 450


def test_refusals_before_any_launch(ops):
    from r3d_amd import _lib
    from r3d_amd.rankstream import StreamingRank
    for H in (0, 2049):
        with pytest.raises(ValueError, match="width"):
            StreamingRank(H, "cuda")
    for lanes in (0, 65):
        with pytest.raises(ValueError, match="lanes"):
            StreamingRank(128, "cuda", lanes=lanes)
    x = torch.ones(4, 128, device="cuda")
    for lanes in (65,):
        with pytest.raises(_lib.R3DHipError, match="R3D_EINVAL"):
            ops.qr_append(x, torch.zeros(lanes, 128, 128, device="cuda"))
    with pytest.raises(_lib.R3DHipError, match="R3D_EINVAL"):
        ops.qr_append(torch.ones(4, 2049, device="cuda"), torch.zeros(1, 2049, 2049, device="cuda"))
    R = torch.zeros(2, 128, 128, device="cuda")
    lib = _lib.load()
    assert lib.r3d_qr_append(x.data_ptr(), 127, 4, 128, None, 0, R.data_ptr(), None, 2, None) == -1       # ldx < H
    assert lib.r3d_qr_append(x.data_ptr(), 128, 4, 128, None, 0, R.data_ptr(), None, 0, None) == -1       # lanes 0
    assert lib.r3d_qr_append(x.data_ptr(), 128, 4, 0, None, 0, R.data_ptr(), None, 2, None) == -1         # H 0
    with pytest.raises(ValueError, match="float32"):
        ops.qr_append(x.double(), R)
    with pytest.raises(ValueError, match="row_label"):
        ops.qr_append(x, R, row_label=torch.zeros(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="lanes, H, H"):
        ops.qr_append(x, R[0])
    acc = StreamingRank(128, "cuda")
    with pytest.raises(ValueError):
        acc.update(torch.ones(4, 64, device="cuda"))
    with pytest.raises(ValueError, match="pad_idx"):
        acc.update(x, torch.zeros(4, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    assert not R.any() and not acc.R.any()


# ------------------------------------------------------------------------------------------------------------------
# models and the loop
# ------------------------------------------------------------------------------------------------------------------
LENS = [(16, 1, 9, 16, 16, 2, 15, 7), (3, 16, 16, 16, 11, 16, 1, 5), (16, 16, 16, 16, 16, 16, 16, 8)]
# (variant, H, heads, chain route -- None: not asserted); the plain model runs its embedding seam in validation too
MODEL_CASES = [("tf", 128, 8, True), ("tf", 136, 4, False), ("bn", 128, 8, None), ("vary", 128, 8, None),
               ("plain", 128, 8, None), ("plain", 136, 8, False)]


def _loader(H, heads, variant, B=8, S=16):
    return [WC.make_batch(WC._c(B, S, H, heads, variant=variant, pad=lens), seed=70 + i) for i, lens in enumerate(LENS)]


def _build(variant, H, heads):
    from tests.test_width_shapes_gpu import build_model, params
    return build_model(variant, H, heads, K, params(variant, H, heads, K))


@pytest.mark.parametrize("variant,H,heads,chain", MODEL_CASES, ids=lambda v: str(v))
def test_measure_rank_against_fp64_of_the_engines_buffers(variant, H, heads, chain, monkeypatch):
    from r3d_amd.engine import FusionEngine
    from r3d_amd.rankstream import BUFFERS, measure_rank
    model = _build(variant, H, heads).eval()
    loader = _loader(H, heads, variant)
    kept = {name: [] for name in BUFFERS}
    routes = []
    real = FusionEngine.forward

    def forward(self, feats, depth, labels, mode="train", **kw):
        out = real(self, feats, depth, labels, mode, **kw)
        assert mode == "val" and kw.get("need_grad") is False
        w = self.last["w"]
        ok = (labels != PAD).reshape(-1)
        for name, attr in BUFFERS.items():
            kept[name].append(getattr(w, attr)[ok].cpu())
        routes.append(any(isinstance(k, tuple) and k[0] == "fwd_chain" for k in w.tables))
        return out
    monkeypatch.setattr(FusionEngine, "forward", forward)
    res = measure_rank(model, loader, torch.device("cuda"))
    monkeypatch.undo()
    assert len(routes) == 3 and (chain is None or all(r == chain for r in routes)), routes
    assert model.engine().rank_stream is None
    n_valid = sum(sum(l) for l in LENS)
    for name in ("rgb", "depth", "fused"):
        x = torch.cat(kept[name]).numpy()
        assert x.shape == (n_valid, H) and np.isfinite(x).all()
        er_ref = RO.erank64(x)
        print(f"[rank model {variant} H{H}x{heads} {name}] erank {res[name]['erank']:.5f} vs {er_ref:.5f} over {n_valid} frames")
        assert res[name]["rows"] == n_valid
        assert abs(res[name]["erank"] - er_ref) <= RC.erank_tol(er_ref), (name, res[name]["erank"], er_ref)
    only = measure_rank(model, loader, torch.device("cuda"), which=("fused",))
    assert list(only) == ["fused"] and only["fused"]["erank"] == res["fused"]["erank"]


def test_measure_rank_refuses_a_query_model(ops, monkeypatch):
    from r3d_amd.model.futr_unsupervised_depth import FUTR
    from r3d_amd.rankstream import measure_rank
    model = FUTR(K, 128, PAD, torch.device("cuda"), ARGS, n_query=8, n_head=8, num_encoder_layers=2, num_decoder_layers=1)
    calls = []
    monkeypatch.setattr(ops, "qr_append", lambda *a, **k: calls.append("qr_append"))

    def loader():
        calls.append("loader")
        yield None
    with pytest.raises(ValueError, match="no fused token matrix"):
        measure_rank(model, loader(), torch.device("cuda"))
    assert not calls


def test_train_refuses_the_report_under_data_parallelism(tmp_path, monkeypatch):
    """An initialised process group of more than one rank: train() raises before it builds the data-parallel wrapper,
    touches the loader or allocates an accumulator."""
    import torch.distributed as dist
    from r3d_amd import train_proposed_depth as T
    model = _build("tf", 128, 8)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)

    def no_dp(*a, **k):
        raise AssertionError("the data-parallel wrapper was built")
    monkeypatch.setattr(T, "DataParallelStep", no_dp)

    def loader():
        raise AssertionError("the loader was touched")
        yield None
    args = argparse.Namespace(epochs=1, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=1,
                              graph_steps=True, erank_report=True)
    with pytest.raises(ValueError, match="data parallelism"):
        T.train(args, model, loader(), None, None, None, str(tmp_path), PAD, torch.device("cuda"), loader(), seed=1)
    assert model.engine().rank_stream is None


def test_train_with_erank_report_adds_one_line_per_epoch(tmp_path, capsys):
    from r3d_amd.optim import FlatAdamW, LinearWarmupCosineAnnealingLR
    from r3d_amd.rankstream import measure_rank, report_line
    from r3d_amd.train_proposed_depth import train
    batches = _loader(128, 8, "tf")
    val = _loader(128, 8, "tf")[1:]
    texts, engines, models = [], [], []
    for flag in (False, True):
        model = _build("tf", 128, 8)
        args = argparse.Namespace(epochs=2, input_type="i3d_transcript", seg=True, anticipate=True, task="long", min_batch=1,
                                  graph_steps=True, erank_report=flag)
        opt = FlatAdamW(model.parameters(), 1e-3, weight_decay=5e-3)
        sch = LinearWarmupCosineAnnealingLR(opt, warmup_epochs=2, max_epochs=4)
        sch.step()
        sch.step()
        capsys.readouterr()
        train(args, model, batches, opt, sch, None, str(tmp_path), PAD, torch.device("cuda"), val, seed=1)
        torch.cuda.synchronize()
        texts.append(capsys.readouterr().out.splitlines())
        engines.append(model.engine())
        models.append(model)
    off, on = texts
    assert engines[0].rank_stream is None and engines[1].rank_stream is None
    assert not any(l.startswith("Effective rank over") for l in off)
    rank_lines = [l for l in on if l.startswith("Effective rank over")]
    assert len(rank_lines) == 2
    assert [l for l in on if not l.startswith("Effective rank over")] == off
    for i, l in enumerate(on):                           # each one directly after a validate() line
        if l.startswith("Effective rank over"):
            assert on[i - 1].startswith("Validation Loss:")
    assert torch.equal(engines[0].arena.params, engines[1].arena.params)
    n_valid = sum(sum(l) for l in LENS[1:])
    assert rank_lines[-1].startswith(f"Effective rank over {n_valid} frames: rgb ")
    assert rank_lines[-1] == report_line(measure_rank(models[1], val, torch.device("cuda")))
    print(rank_lines[-1])
