"""The launch sequence of one training step, dropout on, of every engine that runs the composed post-norm decoder
(r3d_amd/decoder_composed.py: engine_unsup's depth-query and label-query models, engine_l3, engine_m3), against
tests/golden/composed_launches.json -- the library entry points in the order they were called, recorded by
tests/golden/make_golden_composed.py before the three engines' decoder copies became one.  Every r3d_amd.ops wrapper ends in
ops.check(rc, "r3d_<entry point>"), so the second argument of every check call is the list.  Two decoder layers: the smallest
depth at which both sides of every `l == L - 1` / `l == 0` branch run.  Needs an MI355X."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import synth  # noqa: E402
from tests import l3_cases as LC, m3_cases as MC, query_cases as QC  # noqa: E402
from tests import test_query_shapes_gpu as QS  # noqa: E402
from tests.test_proposed_cpu import probe_loss  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composed_launches.json")
LR, WD = 1e-3, 5e-3


class Recorder(QS.Recorder):
    NAMES = ("check",)

    def names(self):
        return [a[1] for _, a in self.calls]


def _query(c, long_clips=False):
    """(engine, step) of a query model row; "label": the autograd bridge's step (the model has no fused loss) + AdamW."""
    from tests.test_long_clips_gpu import build_model
    model = build_model(c, QS.params(c), long_clips=long_clips).train()
    eng = model.engine()
    d = [t.cuda() for t in QC.make_batch(c)]
    if c.variant == "depth":
        return eng, lambda: eng.train_step(d[0], d[1], d[2], d[3], d[4], LR, WD)

    def step():
        loss = probe_loss(model((d[0], d[2]), d[1]))
        loss.backward()
        eng.adamw(LR, WD, tick_dropout=True)
        return loss
    return eng, step


def _l3():
    """the l3_tiny fixture's shape with two decoder layers (the fixture's own parameters hold one: the analytic fill)"""
    from r3d_amd.model.futr_unsupervised_temp3 import FUTR
    c = dict(LC.STEP_BY_TAG["l3_tiny"], n_dec=2)
    model = FUTR(c["n_class"], c["H"], LC.pad_idx(c), torch.device("cuda"), QS.ARGS, n_query=8, n_head=c["n_head"],
                 num_encoder_layers=2, num_decoder_layers=c["n_dec"], query_num=c["query_num"])
    fill = synth.fill_state([(n, tuple(q.shape)) for n, q in model.named_parameters()])
    model.load_state_dict({n: torch.from_numpy(v) for n, v in fill.items()}, strict=False)
    eng = model.to("cuda").train().engine()
    d = [t.cuda() for t in LC.batch(c, c["seed"])]
    return eng, lambda: eng.train_step(d[0], d[1], d[2], d[3], d[4], LR, WD, LC.WFS[1])


def _m3(seam):
    c = MC._step("composed", 2, 5, 128, 8, 17, 2, 256, 21)
    model, _ = MC.build_model(c, "cuda", dropout=True)
    eng = model.train().engine()
    eng.use_seam = seam
    d = [t.cuda() for t in MC.batch(c)]
    return eng, lambda: eng.train_step(d[0], d[1], d[2], d[3], d[4], LR, WD, gaze=d[5])


CASES = {
    "depth_core": lambda: _query(QC._c("depth", 2, 16, 128, 8, n_dec=2)),
    # dh 16: S = 65 is the first length the S x S core refuses -> the tiled route and its delta workspace
    "depth_tiled": lambda: _query(QC._c("depth", 1, 65, 128, 8, n_dec=2, pad="none"), long_clips=True),
    "label": lambda: _query(QC._c("label", 2, 16, 128, 8, n_dec=2)),
    "l3": _l3,
    "m3_composed": lambda: _m3(False),
    "m3_seam": lambda: _m3(True),
}


def record(name, monkeypatch):
    """The entry points of the case's step, in order; the engine's state shows that the step was the one the case names."""
    eng, step = CASES[name]()
    rec = Recorder(monkeypatch)
    step()
    torch.cuda.synchronize()
    monkeypatch.undo()
    w = eng.last["w"]
    assert eng.last["drop"] and eng.L == 2 and len(w.layers) == 2 and len(w.glayers) == 2
    assert int(eng.step_t.item()) == 1 and int(eng.drop_offset.item()) == 1
    assert getattr(w, "route", "core") == ("tiled" if name == "depth_tiled" else "core")
    assert ("lse_sa" in w.layers[0] and w.delta is not None) if name == "depth_tiled" else "p_sa" in w.layers[0]
    if name.startswith("m3"):
        assert eng.last["seam"] is (name == "m3_seam")
    return rec.names()


@pytest.mark.parametrize("name", list(CASES))
def test_step_launches_equal_the_recording(name, monkeypatch):
    with open(GOLDEN) as fh:
        want = json.load(fh)[name]
    got = record(name, monkeypatch)
    assert len(want) > 60 and all(n.startswith("r3d_") for n in want)
    diff = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (name, len(got), len(want), diff, got[diff:diff + 3], want[diff:diff + 3])
