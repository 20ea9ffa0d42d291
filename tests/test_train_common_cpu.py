"""r3d_amd.train_common without a GPU: the GraphedSteps state machine (eager, capture, replay, re-capture) over a fake engine
and recording stand-ins for torch.cuda's graph API, the checkpoint writes, and unwrap."""
import os
from contextlib import contextmanager

import pytest
import torch
from torch import nn

from r3d_amd.train_common import GraphedSteps, save_best, unwrap

HYPER = (0.01, (0.9, 0.999), 1e-8)


class _Engine:
    erank_weight, erank_route, erank_fold = 0.0, "jacobi", "none"
    pos_grad_rows = 0
    _drop_ready = "stale"

    def __init__(self):
        self.lrs = []

    def set_lr(self, lr):
        self.lrs.append(lr)


class _Steps(GraphedSteps):
    def __init__(self, eng, graph=True):
        super().__init__(eng, torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int64), graph)
        self.calls = []

    def _enqueue(self, buf, lr, hyper, training):
        self.calls.append(([t.data_ptr() for t in buf], [t.clone() for t in buf], lr, hyper, training))


@pytest.fixture
def cuda(monkeypatch):
    """torch.cuda's graph API as recording fakes: log gets ("new", graph id), ("sync",), ("capture", graph id) and ("replay",
    graph id)."""
    log, made = [], []

    class Graph:
        def __init__(self):
            self.id = len(made)
            made.append(self)
            log.append(("new", self.id))

        def replay(self):
            log.append(("replay", self.id))

    @contextmanager
    def graph(g):
        log.append(("capture", g.id))
        yield

    monkeypatch.setattr(torch.cuda, "CUDAGraph", Graph)
    monkeypatch.setattr(torch.cuda, "graph", graph)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: log.append(("sync",)))
    return log


def _batch(B=2, S=3, fill=0.0):
    return [torch.full((B, S, 4), fill), torch.zeros(B, S, dtype=torch.long)]


def test_one_shape_eager_capture_replay(cuda):
    eng = _Engine()
    gs = _Steps(eng)
    for k in range(4):
        gs.step(_batch(fill=float(k)), 0.1 * (k + 1), HYPER, True)
    # step 1 eager, step 2 captured (after a synchronize) and replayed, steps 3 and 4 replayed without an enqueue
    assert cuda == [("new", 0), ("sync",), ("capture", 0), ("replay", 0), ("replay", 0), ("replay", 0)]
    assert len(gs.calls) == 2
    assert eng.lrs == pytest.approx([0.1, 0.2, 0.3, 0.4])               # lr is set on every step, replays included
    assert eng._drop_ready is None
    (st,) = gs.shapes.values()
    assert st["graph"].id == 0 and st["hyper"] == (HYPER, 0)
    # every enqueue ran on the record's static buffers, which held that step's batch; lr / hyper / training pass through
    for (ptrs, vals, lr, hyper, training), k in zip(gs.calls, range(2)):
        assert ptrs == [t.data_ptr() for t in st["buf"]]
        assert float(vals[0][0, 0, 0]) == float(k) and (hyper, training) == (HYPER, True)
    assert float(st["buf"][0][0, 0, 0]) == 3.0                           # a replay's batch is copied in too


def test_changed_hyper_runs_eager_then_recaptures(cuda):
    gs = _Steps(_Engine())
    for _ in range(3):
        gs.step(_batch(), 0.1, HYPER, True)
    other = (0.02,) + HYPER[1:]
    del cuda[:]
    n = len(gs.calls)
    gs.step(_batch(), 0.1, other, True)
    (st,) = gs.shapes.values()
    assert cuda == [] and len(gs.calls) == n + 1 and st["graph"] is None         # one eager step
    gs.step(_batch(), 0.1, other, True)
    assert cuda == [("new", 1), ("sync",), ("capture", 1), ("replay", 1)] and len(gs.calls) == n + 2
    gs.step(_batch(), 0.1, other, True)
    assert cuda[-1] == ("replay", 1) and len(gs.calls) == n + 2
    assert gs.calls[-1][3] == other


def test_grown_pos_grad_rows_recaptures(cuda):
    eng = _Engine()
    gs = _Steps(eng)
    for _ in range(3):
        gs.step(_batch(), 0.1, HYPER, True)
    eng.pos_grad_rows = 7                       # a longer batch has been seen since the capture
    n = len(gs.calls)
    gs.step(_batch(), 0.1, HYPER, True)
    gs.step(_batch(), 0.1, HYPER, True)
    (st,) = gs.shapes.values()
    assert len(gs.calls) == n + 2 and st["graph"].id == 1 and st["hyper"] == (HYPER, 7)
    assert cuda[-4:] == [("new", 1), ("sync",), ("capture", 1), ("replay", 1)]


def test_second_shape_has_its_own_record(cuda):
    gs = _Steps(_Engine())
    for _ in range(3):
        gs.step(_batch(S=3), 0.1, HYPER, True)
    (first,) = gs.shapes.values()
    graph, bufs = first["graph"], [t.data_ptr() for t in first["buf"]]
    gs.step(_batch(S=5), 0.1, HYPER, True)                              # eager
    gs.step(_batch(S=5), 0.1, HYPER, True)                              # captured
    assert len(gs.shapes) == 2 and len(gs.calls) == 4
    assert first["graph"] is graph and [t.data_ptr() for t in first["buf"]] == bufs
    gs.step(_batch(S=3), 0.1, HYPER, True)
    gs.step(_batch(S=3), 0.1, HYPER, False)                             # training is part of the key: a third record
    assert cuda[-1] == ("replay", 0) and len(gs.shapes) == 3 and len(gs.calls) == 5
    key = next(k for k, v in gs.shapes.items() if v is first)
    assert gs.shapes[key]["graph"] is graph


def test_tensor_living_in_its_buffer_is_not_copied(cuda, monkeypatch):
    gs = _Steps(_Engine())
    gs.step(_batch(), 0.1, HYPER, True)
    (st,) = gs.shapes.values()
    copies = []
    real = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, "copy_", lambda dst, src, **kw: (copies.append(dst.data_ptr()), real(dst, src, **kw))[1])
    gs.step([st["buf"][0], torch.ones(2, 3, dtype=torch.long)], 0.1, HYPER, True)
    assert copies == [st["buf"][1].data_ptr()]
    assert int(st["buf"][1].sum()) == 6


def test_no_graph_enqueues_on_the_callers_tensors(cuda):
    eng = _Engine()
    gs = _Steps(eng, graph=False)
    batches = [_batch(S=3), _batch(S=3), _batch(S=5), _batch(S=3)]
    for k, b in enumerate(batches):
        gs.step(b, 0.1 * (k + 1), HYPER, True)
    assert [c[0] for c in gs.calls] == [[t.data_ptr() for t in b] for b in batches]
    assert eng.lrs == pytest.approx([0.1, 0.2, 0.3, 0.4])
    assert gs.shapes == {} and cuda == []


class _Two(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Parameter(torch.zeros(3))
        self.b = nn.Parameter(torch.ones(2))


def test_save_best_writes_both_files_and_replaces_best(tmp_path, capsys):
    model = _Two()
    save_best(model, str(tmp_path), 7, 0, 1.23456)
    assert sorted(os.listdir(tmp_path)) == ["seed_7_best.ckpt", "seed_7_checkpoint0.ckpt"]
    assert capsys.readouterr().out == "Best model saved with validation loss: 1.235\n"
    with torch.no_grad():
        model.a.fill_(5.0)
    save_best(model, str(tmp_path), 7, 3, 0.5)
    assert sorted(os.listdir(tmp_path)) == ["seed_7_best.ckpt", "seed_7_checkpoint0.ckpt", "seed_7_checkpoint3.ckpt"]
    assert capsys.readouterr().out == "Best model saved with validation loss: 0.500\n"
    best = torch.load(tmp_path / "seed_7_best.ckpt")
    assert sorted(best) == ["a", "b"] and torch.equal(best["a"], torch.full((3,), 5.0))         # the old best is replaced
    assert torch.equal(torch.load(tmp_path / "seed_7_checkpoint0.ckpt")["a"], torch.zeros(3))
    assert torch.equal(torch.load(tmp_path / "seed_7_checkpoint3.ckpt")["a"], torch.full((3,), 5.0))


def test_loop_writes_nothing_without_an_improvement(tmp_path, capsys):
    """The comparison stays in the loops: with it false (here the loops' own expression on equal accuracies) no file and
    no line."""
    best_val_acc, best_weight_acc, val_acc, weight_acc = 0.5, 0.5, 0.5, 0.5
    if val_acc > best_val_acc or weight_acc > best_weight_acc:
        save_best(_Two(), str(tmp_path), 7, 1, 0.1)
    assert os.listdir(tmp_path) == [] and capsys.readouterr().out == ""


def test_unwrap_walks_wrappers_and_refuses_foreign_models():
    core = _Two()
    wrapped = nn.Module()
    wrapped.module = nn.Module()
    wrapped.module.module = core
    assert unwrap(wrapped, _Two, "msg") is core
    assert unwrap(core, (_Two, nn.Linear), "msg") is core
    with pytest.raises(TypeError, match="^this loop drives _Two$"):
        unwrap(nn.Linear(2, 2), _Two, "this loop drives _Two")
    foreign = nn.Module()
    foreign.module = nn.Linear(2, 2)
    with pytest.raises(TypeError, match="^this loop drives _Two$"):
        unwrap(foreign, _Two, "this loop drives _Two")
