"""The launch sequence of one optimiser step of the five engines tests/test_composed_decoder_gpu.py does not cover (the token-
fusion engine with its BN-blend, activation-magnitude and plain variants, AFFT, CNN, RNN, TCN), against
tests/golden/engine_launches.json -- recorded by tests/golden/make_golden_engine_launches.py while every engine carried its
own step plumbing; the test holds r3d_amd/engine_base.py, which they share now, to it.

Each case uses its engine's smallest committed fixture, built the way that engine's own GPU test builds it, and runs twice:
  train_step   the engine's fused step, dropout on where the engine has dropout (the ticked path: the loss launch advances
               the counters);
  bridge       the model's autograd bridge, probe_loss(...).backward(), optim.FlatAdamW.step() (the un-ticked path: AdamW's
               own tick launch).
A recording is the list of library entry points in call order (the second argument of every ops.check), and in front of the
entry point of a tick or AdamW launch one more item with what the names alone do not show: the element count of its first
tensor, for the tick whether a dropout counter was passed, for AdamW whether no loss reduction rides along.  Needs an MI355X."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_query_shapes_gpu as QS  # noqa: E402
from tests.helpers import fixture_batch, fixture_params, load_fixture  # noqa: E402
from tests.test_proposed_cpu import probe_loss  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_launches.json")
LR, WD = 1e-3, 5e-3
PATHS = ("train_step", "bridge")


class Recorder(QS.Recorder):
    NAMES = ("check",)
    STEP_OPS = ("tick", "adamw_flat", "adamw_flat_dropout", "adamw_2d")

    def __init__(self, monkeypatch):
        from r3d_amd import ops
        super().__init__(monkeypatch)
        for nm in self.STEP_OPS:
            fn = getattr(ops, nm)

            def wrap(*a, _fn=fn, _nm=nm, **k):
                flag = (a[1] if len(a) > 1 else k.get("b")) is not None if _nm == "tick" else k.get("loss_fin") is None
                self.calls.append((_nm, (None, [_nm, a[0].numel(), bool(flag)])))
                return _fn(*a, **k)
            monkeypatch.setattr(ops, nm, wrap)

    def names(self):
        return [a[1] for _, a in self.calls]


# ---- (model, batch on the device, train_step arguments in front of lr, dropout expected, drop_offset after each path) -----
def _fusion(tag):
    fx = load_fixture(tag)
    m = fx["meta"]
    K = m["n_class"]
    if tag == "step_tiny":
        from tests.test_engine_gpu import build_model
        model, batch = build_model(fx), fixture_batch(fx)
    elif tag == "bn_tiny":
        from oracle import synth
        from tests.test_bn_variant_gpu import _model
        model = _model(fx)
        batch = [torch.from_numpy(x) for x in synth.make_batch(m["B"], m["S"], K, m["pad_idx"], m["seed"],
                                                               depth_hw=tuple(m["depth_hw"]))]
    elif tag == "vary_tiny":
        from tests import test_vary_gpu as T, vary_oracle as V
        model, batch = T._model(V.vary_params(fx), m["H"], K, m["pad_idx"]), T._batch(m["B"], m["S"], K, m["seed"])
    elif tag == "plain_tiny":
        from tests import plain_oracle as PO, test_plain_fuser_gpu as T
        model = T._model(PO.plain_params(fx), m["H"], K, m["pad_idx"], m["n_dec"])
        batch = T._batch(m["B"], m["S"], K, m["seed"])
    else:
        from tests import test_afft_gpu as T
        model = T._model(fixture_params(fx), m["H"], K, m["pad_idx"], n_enc=m["n_encoder_layer"])
        batch = T._batch(m["B"], m["S"], K, m["seed"])
    d = [t.cuda() for t in batch]

    def bridge():           # (AFFT has no 'seg' output: probe_loss reads 'action' under that name too)
        out = model((d[0], d[2]), d[1])
        return out if "seg" in out else dict(out, seg=out["action"])
    return model, (d[0], d[1], d[2], d[3], d[4]), bridge, True, (1, 0)


def _unimodal(tag):
    from tests import test_cnn_gpu, test_rnn_gpu
    T = test_cnn_gpu if tag == "cnn_tiny" else test_rnn_gpu
    fx = load_fixture(tag)
    f, lab, dur, tgt = T._dev(T._batch(fx))
    model = T._model(fx)
    return model, (f, None, lab, dur, tgt), lambda: model((f, lab)), False, (0, 0)


def _tcn(tag):
    from tests import test_tcn_gpu as T
    fx = load_fixture(tag)
    model = T._model(fx, p_drop=0.2)
    feats, tgt = T._batch(fx["meta"])

    def bridge():           # one output: probe_loss reads it under its three names
        out = model(feats)
        return dict(seg=out, action=out, duration=out)
    return model, (feats, tgt, fx["meta"]["pad_idx"]), bridge, True, (1, 1)      # (every dropout forward moves the offset)


CASES = {"step_tiny": _fusion, "bn_tiny": _fusion, "vary_tiny": _fusion, "plain_tiny": _fusion, "afft_tiny": _fusion,
         "cnn_tiny": _unimodal, "rnn_tiny": _unimodal, "tcn_tiny": _tcn}


def record(name, path, monkeypatch):
    """The recording of the case's step; the engine's state shows that the step was the one the case names."""
    from r3d_amd.optim import FlatAdamW
    model, step_args, bridge, drop, offsets = CASES[name](name)
    eng = model.train().engine()
    rec = Recorder(monkeypatch)
    if path == "train_step":
        eng.train_step(*step_args, LR, WD)
    else:
        opt = FlatAdamW(model.parameters(), lr=LR, weight_decay=WD)
        probe_loss(bridge()).backward()
        opt.step()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert model.engine() is eng and bool(eng.last["drop"]) is drop
    assert int(eng.step_t.item()) == 1 and int(eng.drop_offset.item()) == offsets[PATHS.index(path)]
    assert bool(torch.isfinite(eng.arena.params).all())
    return rec.names()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(CASES))
def test_step_launches_equal_the_recording(name, path, monkeypatch):
    with open(GOLDEN) as fh:
        want = json.load(fh)[name][path]
    got = record(name, path, monkeypatch)
    assert len(want) > 10 and all(n.startswith("r3d_") if isinstance(n, str) else n[0] in Recorder.STEP_OPS for n in want)
    assert sum(not isinstance(n, str) for n in want) >= 1 + (path == "bridge")       # an AdamW launch; un-ticked: its tick too
    diff = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (name, path, len(got), len(want), diff, got[diff:diff + 3], want[diff:diff + 3])
