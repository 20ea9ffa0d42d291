#!/usr/bin/env python3
"""Generates tests/golden/cnn_*.npz by IMPORTING THE REFERENCE's CNN baseline (model/cnn.py) and its loop
(train/train_unimodal.py) on CPU -- build container only, never on the GPU machine.  Parameters: the analytic
oracle.synth fill.  Per case: a train-mode step through the reference's model and the loss composition of
train_unimodal.py:188-225 (class 120 excluded), outputs, losses, counters, gradient statistics of every live parameter
(full tensors at the tiny shape), post-AdamW statistics, the live and dead name lists, a test-mode forward with the bare
feature tensor, the state_dict keys / shapes and the init checksums at torch.manual_seed(1).  Plus the reference's own
train() stdout, validation result and checkpoint names on a tiny batch list (cnn_train_loop).  Every value is
cross-checked against tests/cnn_oracle.py (float64); the script aborts on a mismatch."""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("R3D_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
sys.path[:0] = [REF, os.path.join(REF, "train")]

from oracle import synth  # noqa: E402
from opts import parser  # noqa: E402
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402   (helpers: stats, check_close, t_batch)
from tests import cnn_oracle as RO  # noqa: E402

M = importlib.import_module("model.cnn")
T = importlib.import_module("train_unimodal")
RU = importlib.import_module("utils")
LR, WD = 1e-3, 5e-3
DEPTH_HW = (4, 4)               # the model never reads depth: tiny maps


def _new(H, n_class):
    args = parser.parse_args([])
    args.hidden_dim, args.n_query = H, 8
    pad_idx = n_class + 1
    model = M.FUTR(n_class, H, device=torch.device("cpu"), args=args, src_pad_idx=pad_idx, n_query=8, n_head=args.n_head,
                   num_encoder_layers=args.n_encoder_layer, num_decoder_layers=args.n_decoder_layer)
    return model, args, pad_idx


def build(H, n_class):
    model, args, pad_idx = _new(H, n_class)
    names_shapes = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    state = synth.fill_state(names_shapes)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[n]))
    return model, args, pad_idx, names_shapes


def init_checksums(H, n_class):
    torch.manual_seed(1)
    model, _, _ = _new(H, n_class)
    return np.array([[float(p.detach().double().sum()), float((p.detach().double() ** 2).sum())]
                     for _, p in model.named_parameters()], np.float64)


def make_batch(B, S, n_class, pad_idx, seed, with_exclusion):
    b = synth.make_batch(B, S, n_class, pad_idx, seed, depth_hw=DEPTH_HW)
    if with_exclusion:                    # NTU's UNDEFINED (120) among the observed and the future labels
        b[2][0, 1:4] = 120
        b[2][2, 0] = 120
        b[4][1, 0] = 120
        b[4][3, 1] = 120
    return G.t_batch(b)


def ref_losses(out, lab, dur, tgt, pad_idx):
    """train_unimodal.py:188-225, by calling the reference's functions in that order."""
    crit = torch.nn.MSELoss(reduction="none")
    dur_mask = (dur != pad_idx).long()
    target_dur = dur * dur_mask
    seg = out["seg"]
    B, Tt, C = seg.size()
    l_seg, sc, st, _ = RU.cal_performance(seg.view(-1, C), lab.view(-1), pad_idx, exclude_class_idx=120, reference=None,
                                          target_ref=None)
    act = out["action"]
    B, Tq, C = act.size()
    first = T.get_last_non_padding_labels(lab, pad_idx)
    l_act, ac, at, _ = RU.cal_performance(act.view(-1, C), tgt.contiguous().view(-1), pad_idx, exclude_class_idx=120,
                                          reference=first, target_ref=tgt[:, 0])
    od = RU.normalize_duration(out["duration"], dur_mask)
    l_dur = torch.sum(crit(od, target_dur * dur_mask)) / torch.sum(dur_mask)
    return dict(loss_seg=l_seg, loss_action=l_act, loss_dur=l_dur, loss=l_seg + l_act + l_dur,
                seg_correct=sc, seg_total=st, act_correct=ac, act_total=at)


def case(tag, H, B, S, n_class, seed, with_exclusion, full_grads):
    model, args, pad_idx, names_shapes = build(H, n_class)
    batch = make_batch(B, S, n_class, pad_idx, seed, with_exclusion)
    feats, depth, lab, dur, tgt = batch
    meta = dict(tag=tag, H=H, B=B, S=S, n_class=n_class, pad_idx=pad_idx, seed=seed, n_query=8, depth_hw=list(DEPTH_HW),
                with_exclusion=with_exclusion, lr=LR, wd=WD, torch=torch.__version__)
    fx = {"param_names": json.dumps([n for n, _ in names_shapes]),
          "param_shapes": json.dumps([list(s) for _, s in names_shapes]),
          "state_keys": json.dumps(list(model.state_dict().keys())),
          "state_shapes": json.dumps([list(v.shape) for v in model.state_dict().values()]),
          "init_sums": init_checksums(H, n_class)}
    model.eval()
    with torch.no_grad():
        tout = model(feats, mode="test")                      # the bare tensor outside train mode (:79)
    model.train()
    out = model((feats, lab))
    res = ref_losses(out, lab, dur, tgt, pad_idx)
    res["loss"].backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    live = list(grads)
    dead = [n for n, _ in names_shapes if n not in grads]
    opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    opt.step()
    post = {n: p.detach().clone() for n, p in model.named_parameters()}
    fx.update({
        "meta": json.dumps(meta),
        "out_action": out["action"].detach().numpy(), "out_duration": out["duration"].detach().numpy(),
        "out_seg": out["seg"].detach().numpy(), "supcon_stats": G.stats(out["supcon"]),
        "test_action": tout["action"].numpy(), "test_duration": tout["duration"].numpy(), "test_seg": tout["seg"].numpy(),
        "losses": np.array([float(res[k].detach()) for k in ("loss_seg", "loss_action", "loss_dur", "loss")], np.float64),
        "counts": np.array([res[k] for k in ("seg_correct", "seg_total", "act_correct", "act_total")], np.int64),
        "live_names": json.dumps(live), "dead_names": json.dumps(dead),
        "grad_stats": np.stack([G.stats(grads[n]) for n in live]),
        "post_stats": np.stack([G.stats(post[n]) for n in live]),
    })
    for n in live:
        if (full_grads and not n.endswith("input_embed.weight")) or n in ("input_embed.bias", "fc_seg.bias", "fc_len.weight"):
            fx["grad::" + n] = grads[n].numpy()
    # ---- restatement cross-check (float64) ----------------------------------------------------------------------------
    p0 = {n: torch.from_numpy(synth.fill_value(n, s, j)) for j, (n, s) in enumerate(names_shapes)}
    tr = RO.Trainer(p0, pad_idx, lr=LR, wd=WD)
    with torch.no_grad():
        to = RO.forward(tr.p, feats.double())
    for k in ("action", "duration", "seg"):
        G.check_close(f"{tag}/test/{k}", to[k], tout[k])
    ores, oout, _ = tr.step(batch)
    for k in ("action", "duration", "seg", "supcon"):
        G.check_close(f"{tag}/out/{k}", oout[k], out[k])
    for k in ("loss_seg", "loss_action", "loss_dur", "loss"):
        G.check_close(f"{tag}/{k}", ores[k], res[k])
    for k, j in (("seg_correct", 0), ("seg_total", 1), ("act_correct", 2), ("act_total", 3)):
        assert int(ores[k]) == int(fx["counts"][j]), (tag, k)
    assert sorted(live) == sorted(n for n, q in tr.p.items() if q.grad is not None), "live set"
    for n in live:
        g = grads[n]
        G.check_close(f"{tag}/grad/{n}", tr.p[n].grad, g, tol=5e-5 * max(1.0, float(g.abs().max())))
        # (gradients that are zero up to rounding -- fc_len.bias: the duration normalisation is shift-invariant -- let
        # AdamW move the parameter either way)
        keep = g.abs() > 1e-6 * max(1.0, float(g.abs().max()))
        G.check_close(f"{tag}/post/{n}", tr.p[n].detach()[keep], post[n][keep], tol=1e-5)
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **fx)
    print(f"[golden-cnn] {tag}: loss={float(res['loss']):.6f} counts={fx['counts'].tolist()} live={len(live)} "
          f"dead={len(dead)} -> {os.path.getsize(path)/1024:.1f} KB")


def case_train_loop(tag, H, B, S, n_class, n_steps, seed):
    """The reference's own train_unimodal.train() for one epoch of n_steps batches (+ one batch of 3 clips it skips), torch
    AdamW (lr 1e-3, wd 5e-3), a no-op scheduler, then its validate() on one B = 1 clip and its checkpoint writes."""
    model, args, pad_idx, names_shapes = build(H, n_class)
    args.epochs = 1
    batches = [make_batch(B, S, n_class, pad_idx, seed + i, True) for i in range(n_steps)]
    batches.insert(1, make_batch(3, S, n_class, pad_idx, seed + 50, False))          # < 8 clips: skipped (:163)
    val = [G.t_batch(synth.make_batch(1, S + 3, n_class, pad_idx, seed + 100, pad_tail=False, depth_hw=DEPTH_HW))]
    step_stats = []

    class NoSched:
        def step(self):
            pass
    # With the analytic fill the trained model anticipates none of the synthetic clip's future labels, and the reference's
    # loop saves a checkpoint only when a validation accuracy rises above 0: a first run of the same training (it does not
    # read the validation clip) tells which classes the trained model anticipates, and the clip's future labels are set to
    # them where the decision is clear (top-two gap > 0.01) and the class is neither 120 nor padding.
    m0, a0, _, _ = build(H, n_class)
    a0.epochs = 1
    with tempfile.TemporaryDirectory() as d0, contextlib.redirect_stdout(io.StringIO()):
        T.train(a0, m0, batches, torch.optim.AdamW(m0.parameters(), LR, weight_decay=WD), NoSched(),
                torch.nn.MSELoss(reduction="none"), d0, pad_idx, torch.device("cpu"), val, seed)
    with torch.no_grad():
        act = m0((val[0][0], val[0][2]))["action"][0]
    top = act.topk(2, -1)
    for q in range(act.shape[0]):
        c = int(top.indices[q, 0])
        if int(val[0][4][0, q]) != pad_idx and c not in (120, pad_idx) and float(top.values[q, 0] - top.values[q, 1]) > 1e-2:
            val[0][4][0, q] = c

    class SpyAdamW(torch.optim.AdamW):
        def step(self, closure=None):
            r = super().step(closure)
            step_stats.append(np.stack([G.stats(p) for n, p in model.named_parameters() if p.grad is not None]))
            return r

    opt = SpyAdamW(model.parameters(), LR, weight_decay=WD)
    buf = io.StringIO()
    with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(buf):
        T.train(args, model, batches, opt, NoSched(), torch.nn.MSELoss(reduction="none"), d, pad_idx, torch.device("cpu"),
                val, seed)
        files = sorted(os.listdir(d))
        ck_keys = list(torch.load(os.path.join(d, files[0]), weights_only=True).keys()) if files else []
    live_names = [n for n, p in model.named_parameters() if p.grad is not None]
    with contextlib.redirect_stdout(io.StringIO()):
        vres = T.validate(model, val, torch.nn.MSELoss(reduction="none"), pad_idx, torch.device("cpu"))
    fx = {
        "meta": json.dumps(dict(tag=tag, H=H, B=B, S=S, n_class=n_class, pad_idx=pad_idx, seed=seed, n_steps=n_steps,
                                n_query=8, lr=LR, wd=WD, val_S=S + 3, depth_hw=list(DEPTH_HW), torch=torch.__version__)),
        "param_names": json.dumps([n for n, _ in names_shapes]),
        "param_shapes": json.dumps([list(s) for _, s in names_shapes]),
        "live_names": json.dumps(live_names),
        "post_stats": np.stack(step_stats),
        "val_result": np.array([float(x) for x in vres], np.float64),
        "ckpt_files": json.dumps(files), "ckpt_keys": json.dumps(ck_keys),
        "stdout": json.dumps(buf.getvalue()),
        "val_target": val[0][4].numpy(),
    }
    p0 = {n: torch.from_numpy(synth.fill_value(n, s, j)) for j, (n, s) in enumerate(names_shapes)}
    tr = RO.Trainer(p0, pad_idx, lr=LR, wd=WD)
    for i, b in enumerate(x for x in batches if len(x[0]) >= 8):
        tr.step(b)
        ost = np.stack([G.stats(tr.p[n]) for n in live_names])
        G.check_close(f"{tag}/step{i}/post", ost[:, :3], step_stats[i][:, :3], tol=2e-5)
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **fx)
    assert files, "the loop saved no checkpoint: pick other batches"
    print(f"[golden-cnn] {tag}: val={fx['val_result'].round(4).tolist()} ckpts={files} -> "
          f"{os.path.getsize(path)/1024:.1f} KB")


if __name__ == "__main__":
    if "--loop-only" in sys.argv:
        case_train_loop("cnn_train_loop", H=32, B=8, S=6, n_class=122, n_steps=2, seed=1)
        sys.exit(0)
    case("cnn_tiny", H=16, B=2, S=5, n_class=17, seed=3, with_exclusion=False, full_grads=True)
    case("cnn_cfg", H=128, B=8, S=16, n_class=122, seed=9, with_exclusion=True, full_grads=False)
    case("cnn_odd", H=136, B=13, S=37, n_class=49, seed=5, with_exclusion=False, full_grads=False)
    case_train_loop("cnn_train_loop", H=32, B=8, S=6, n_class=122, n_steps=2, seed=1)
