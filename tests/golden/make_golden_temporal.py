#!/usr/bin/env python3
"""Generates tests/golden/temporal_cases.npz by IMPORTING THE REFERENCE's utils.py (temporal_cluster_loss,
temporal_contrastive_loss, focal_loss, cal_performance_focal) and train/train_unsupervised.py:get_cluster_intervals on CPU --
build container only.  Per case of tests/temporal_cases.py the reference runs on .double() inputs; recorded are the loss, its
autograd gradient with respect to the input (the full tensor, rounded to float32, where it has at most 16384 elements, helpers.stats otherwise),
the intervals get_cluster_intervals finds in the case's labels (as one [n, 3] array of (clip, start, end)), and for the focal
loss the flags and the two counters.  A focal row with a label outside [0, C) is given to the reference as a pad row (the
reference raises on it).  Every value is cross-checked against tests/temporal_oracle.py; the script aborts unless they agree
to 1e-9 relative (plus 1e-11 absolute: the float64 rounding of a softmax probability near 1)."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("R3D_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import utils as RU  # noqa: E402   (the reference's)
from train.train_unsupervised import get_cluster_intervals  # noqa: E402   (the reference's)
from tests import temporal_cases as TC, temporal_oracle as TO  # noqa: E402
from tests.helpers import stats  # noqa: E402

FULL_LIMIT = 16384
RTOL = 1e-9
# A contrastive loss near 0 is -log(p + 1e-5) with p + 1e-5 near 1: scores of |s| <= 1 / tau <= 100 carry 100 * 2^-52 into p
# however p is formed (the reference: exp / sum; the oracle: exp(s - lse)), and the gradient carries it times 1 / (tau |x|).
ATOL = 1e-11


def agree(a, b, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= RTOL * scale + ATOL, (what, err, scale)


def main():
    out, meta = {}, {}
    for case in TC.CASES:
        name = case["name"]
        if case["kind"] == "focal":
            pred, gold = TC.make(case)
            C, pad = case["C"], case["pad"]
            gref = gold.clone()
            gref[(gold < 0) | (gold >= C)] = pad
            xr = pred.double().requires_grad_(True)
            kw = dict(exclude_class_idx=case["exclude"], alpha=case["alpha"], gamma=case["gamma"], penalty_weight=case["penalty"])
            loss, flags = RU.focal_loss(xr, gref, pad, **kw)
            loss.backward()
            grad = xr.grad
            _, n_correct, n_word, _ = RU.cal_performance_focal(pred.double(), gref, pad, exclude_class_idx=case["exclude"])
            (l64, g64), (_, f64, nc64, nw64) = (TO.with_grad(lambda p: TO.focal(p, gold, pad, case["exclude"], case["alpha"],
                                                                               case["gamma"], case["penalty"])[0], pred),
                                                TO.focal(pred, gold, pad, case["exclude"]))
            assert torch.equal(flags, f64) and (n_correct, n_word) == (nc64, nw64), name
            out[f"flags_{name}"] = flags.numpy()
            out[f"counts_{name}"] = np.array([n_correct, n_word], dtype=np.int64)
        else:
            x, iv = TC.make(case)
            lab = TC.labels_of(iv, case["T"])
            with contextlib.redirect_stdout(io.StringIO()):
                found = get_cluster_intervals(lab)
            assert found == iv == TO.intervals(lab), name
            out[f"iv_{name}"] = np.array([(b, s, e) for b, clip in enumerate(found) for s, e in clip], dtype=np.int32)
            xr = x.double().requires_grad_(True)
            if case["kind"] == "cluster":
                loss = RU.temporal_cluster_loss(xr, found)
                l64, g64 = TO.with_grad(TO.cluster, x, iv)
            else:
                loss = RU.temporal_contrastive_loss(xr, found, temperature=case["temperature"])
                l64, g64 = TO.with_grad(TO.contrastive, x, iv, case["temperature"])
            loss.backward()
            grad = xr.grad if xr.grad is not None else torch.zeros_like(xr)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), name
        agree(l64, loss.detach(), f"{name} loss")
        agree(g64, grad, f"{name} gradient")
        out[f"loss_{name}"] = np.float64(float(loss.detach()))
        if grad.numel() <= FULL_LIMIT:
            out[f"grad_{name}"] = grad.numpy().astype(np.float32)
            meta[name] = "full"
        else:
            out[f"gstat_{name}"] = stats(grad)
            meta[name] = "stats"
        print(f"{name:20s} loss {float(loss.detach()):.10f}  oracle {float(l64):.10f}  {meta[name]}")
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "temporal_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
