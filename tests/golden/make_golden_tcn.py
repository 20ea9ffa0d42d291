#!/usr/bin/env python3
"""Generates tests/golden/tcn_*.npz by IMPORTING THE REFERENCE's TCN baseline (model/tcn.py) and its loop
(train/train_tcn.py) on CPU -- build container only.  Dropout p = 0 (the reference's masks come from torch's generator, the
library's from its Philox pool); parameters: the analytic oracle.synth fill, which the tests regenerate, so no fixture
carries the 24 MB of parameters.  Per case (tests/tcn_cases.STEP_CASES): a train-mode step through the reference's model
and ``cal_performance(output.view(-1, C), target.view(-1), pad_idx)``, the outputs, loss and counters, gradient statistics
of every parameter (full tensors of the biases and weight_g), post-AdamW statistics, an eval() forward, the state_dict keys /
shapes and the init checksums at torch.manual_seed(1).

tcn_train_loop: stdout and checkpoint names of the reference's own train() over two epochs of a tiny batch list.
train/train_tcn.py cannot run as it stands -- cal_performance returns four values and train_tcn.py:27,84 unpack three -- so
this script rebinds THAT MODULE's name ``cal_performance`` to a wrapper that calls the reference's own function and drops
the unused fourth value (l2_correct).  Nothing else of the loop is touched.

Every value is cross-checked against tests/tcn_oracle.py (float64); the script aborts on a mismatch."""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("R3D_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
sys.path[:0] = [REF, os.path.join(REF, "train")]
warnings.filterwarnings("ignore", category=FutureWarning)

from oracle import synth  # noqa: E402
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402   (helpers: stats, check_close, t_batch)
from tests import tcn_oracle as TO  # noqa: E402
from tests import tcn_cases as TC  # noqa: E402

M = importlib.import_module("model.tcn")
T = importlib.import_module("train_tcn")
RU = importlib.import_module("utils")
T.cal_performance = lambda *a, **k: RU.cal_performance(*a, **k)[:3]        # see the docstring
FULL_GRADS = (".bias", ".weight_g")


def build(num_classes):
    model = M.MustafaNet1DTCN(num_classes=num_classes, anticipated_frames=8)
    names_shapes = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    assert names_shapes == TO.names_shapes(num_classes), "tcn_oracle.names_shapes != the reference's named_parameters"
    state = synth.fill_state(names_shapes)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[n]))
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model, names_shapes


def init_checksums(num_classes):
    torch.manual_seed(1)
    model = M.MustafaNet1DTCN(num_classes=num_classes, anticipated_frames=8)
    return np.array([[float(p.detach().double().sum()), float((p.detach().double() ** 2).sum())]
                     for _, p in model.named_parameters()], np.float64)


def loop_batch(B, S, n_class, pad_idx, seed, **kw):
    """oracle.synth.make_batch reordered to the loop's 5-tuple (features, past_label, trans_dur_future, target, _)."""
    feats, _depth, lab, dur, tgt = G.t_batch(synth.make_batch(B, S, n_class, pad_idx, seed, depth_hw=(2, 2), **kw))
    return feats, lab, dur, tgt, torch.zeros(0)


def case(tag, B, S, num_classes, n_class, pad_idx, seed):
    model, names_shapes = build(num_classes)
    feats, _lab, _dur, tgt, _ = loop_batch(B, S, n_class, pad_idx, seed)
    sd = model.state_dict()
    fx = {"meta": json.dumps(dict(tag=tag, B=B, S=S, num_classes=num_classes, n_class=n_class, pad_idx=pad_idx, seed=seed,
                                  lr=TC.LR, wd=TC.WD, torch=torch.__version__)),
          "param_names": json.dumps([n for n, _ in names_shapes]),
          "param_shapes": json.dumps([list(s) for _, s in names_shapes]),
          "state_keys": json.dumps(list(sd.keys())), "state_shapes": json.dumps([list(v.shape) for v in sd.values()]),
          "init_sums": init_checksums(num_classes)}
    model.eval()
    with torch.no_grad():
        eout = model(feats)
    model.train()
    out = model(feats)
    C = out.size(2)
    loss, n_correct, n_total, _ = RU.cal_performance(out.view(-1, C), tgt.contiguous().view(-1), pad_idx)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    assert len(grads) == len(names_shapes)
    torch.optim.AdamW(model.parameters(), lr=TC.LR, weight_decay=TC.WD).step()
    post = {n: p.detach().clone() for n, p in model.named_parameters()}
    fx.update({"out": out.detach().numpy(), "eval_out": eout.numpy(), "loss": np.float64(float(loss)),
               "counts": np.array([n_correct, n_total], np.int64),
               "grad_stats": np.stack([G.stats(grads[n]) for n, _ in names_shapes]),
               "post_stats": np.stack([G.stats(post[n]) for n, _ in names_shapes])})
    for n, _ in names_shapes:
        if n.endswith(FULL_GRADS):
            fx["grad::" + n] = grads[n].numpy()
    # ---- restatement cross-check (float64) ----------------------------------------------------------------------------
    tr = TO.Trainer(TO.fill_params(names_shapes), pad_idx, lr=TC.LR, wd=TC.WD)
    with torch.no_grad():
        G.check_close(f"{tag}/eval", TO.forward(tr.p, feats.double()), eout)
    oloss, onc, ont, oout = tr.step(feats, tgt)
    G.check_close(f"{tag}/out", oout, out)
    G.check_close(f"{tag}/loss", oloss, loss)
    assert (onc, ont) == (n_correct, n_total), (tag, onc, ont, n_correct, n_total)
    dev = {}
    for n, _ in names_shapes:
        g = grads[n]
        dev[n] = G.check_close(f"{tag}/grad/{n}", tr.p[n].grad, g, tol=5e-5 * max(1.0, float(g.abs().max())))
        keep = g.abs() > 1e-6 * max(1.0, float(g.abs().max()))
        G.check_close(f"{tag}/post/{n}", tr.p[n].detach()[keep], post[n][keep], tol=1e-5)
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **fx)
    print(f"[golden-tcn] {tag}: loss={float(loss):.6f} counts={fx['counts'].tolist()} pad rows="
          f"{int((tgt == pad_idx).sum())}/{tgt.numel()} max f32-vs-f64 grad dev={max(dev.values()):.2e} -> "
          f"{os.path.getsize(path) / 1024:.1f} KB")


def case_train_loop(tag, B, S, num_classes, n_class, pad_idx, n_steps, epochs, seed, val_S):
    """The reference's own train_tcn.train() (with the unpack rebinding above) for `epochs` epochs of n_steps batches + one
    batch of 3 clips (no batch is skipped), torch AdamW, a no-op scheduler, its validate() on two clips of another length."""
    model, names_shapes = build(num_classes)

    class Args:
        pass
    args = Args()
    args.epochs = epochs
    batches = [loop_batch(B, S, n_class, pad_idx, seed + i) for i in range(n_steps)]
    batches.insert(1, loop_batch(3, S, n_class, pad_idx, seed + 50))
    val = [loop_batch(2, val_S, n_class, pad_idx, seed + 100), loop_batch(1, val_S + 2, n_class, pad_idx, seed + 101)]
    step_stats = []

    class SpyAdamW(torch.optim.AdamW):
        def step(self, closure=None):
            r = super().step(closure)
            step_stats.append(np.stack([G.stats(p) for _, p in model.named_parameters()]))
            return r

    class NoSched:
        def step(self):
            pass
    opt = SpyAdamW(model.parameters(), TC.LR, weight_decay=TC.WD)
    buf = io.StringIO()
    with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(buf):
        T.train(args, model, batches, val, opt, NoSched(), None, d, pad_idx, torch.device("cpu"))
        files = sorted(os.listdir(d))
        ck_keys = list(torch.load(os.path.join(d, files[0]), weights_only=True).keys()) if files else []
    fx = {"meta": json.dumps(dict(tag=tag, B=B, S=S, num_classes=num_classes, n_class=n_class, pad_idx=pad_idx, seed=seed,
                                  n_steps=n_steps, epochs=epochs, val_S=val_S, lr=TC.LR, wd=TC.WD, torch=torch.__version__)),
          "param_names": json.dumps([n for n, _ in names_shapes]),
          "param_shapes": json.dumps([list(s) for _, s in names_shapes]),
          "post_stats": np.stack(step_stats), "ckpt_files": json.dumps(files), "ckpt_keys": json.dumps(ck_keys),
          "training_after": np.int64(model.training), "stdout": json.dumps(buf.getvalue())}
    tr = TO.Trainer(TO.fill_params(names_shapes), pad_idx, lr=TC.LR, wd=TC.WD)
    k = 0
    for _ in range(epochs):
        for b in batches:
            tr.step(b[0], b[3])
            ost = np.stack([G.stats(tr.p[n]) for n, _ in names_shapes])
            G.check_close(f"{tag}/step{k}/post", ost[:, :3], step_stats[k][:, :3], tol=2e-5)
            k += 1
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **fx)
    print(f"[golden-tcn] {tag}: ckpts={files} training_after={model.training} -> {os.path.getsize(path) / 1024:.1f} KB")
    print(buf.getvalue())


if __name__ == "__main__":
    for c in TC.STEP_CASES:
        case(*c)
    case_train_loop(**TC.TRAIN_LOOP)
