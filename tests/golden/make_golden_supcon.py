#!/usr/bin/env python3
"""Generates tests/golden/supcon_cases.npz by IMPORTING THE REFERENCE's SupConLoss (loss/spc.py) on CPU -- build container
only.  Per case of tests/supcon_cases.py: the reference's float32 loss and its autograd gradient with respect to the
features (the full tensor where it has at most 16384 elements, helpers.stats otherwise).  A case with ignored rows runs the
reference on the kept rows only (the gradient of an ignored row is 0); a case with normalize=True runs it on
F.normalize(features, dim=2).  Where the reference returns nan the nan is recorded.  Every finite value is cross-checked
against tests/supcon_oracle.py (float64); the script aborts on a mismatch."""
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

from loss.spc import SupConLoss  # noqa: E402   (the reference's)
from tests import supcon_cases as SC, supcon_oracle as SO  # noqa: E402
from tests.helpers import stats  # noqa: E402

FULL_LIMIT = 16384


def reference(case, x, y):
    """(loss, gradient [bsz, V, D]) of the reference in float32; nan loss -> (nan, None)."""
    xr = x.clone().requires_grad_(True)
    kept = torch.ones(case["bsz"], dtype=torch.bool) if (y is None or not case["ignore"]) else (y != SC.IGNORE)
    if not bool(kept.any()):
        return None, None                                       # nothing to run the reference on
    f = xr[kept]
    if case["normalize"]:
        f = torch.nn.functional.normalize(f, dim=2)
    loss = SupConLoss(**SC.module_kwargs(case))(f, None if y is None else y[kept])
    if not bool(torch.isfinite(loss)):
        return float("nan"), None
    loss.backward()
    return float(loss), xr.grad.detach()


def main():
    out, meta = {}, {}
    for case in SC.CASES:
        x, y = SC.make(case)
        loss, grad = reference(case, x, y)
        name = case["name"]
        if loss is None:
            meta[name] = "no_reference"
            continue
        out[f"loss_{name}"] = np.float32(loss)
        if grad is None:
            meta[name] = "nan"
            continue
        l64, g64, _, _ = SO.supcon_with_grad(SO.contrast_rows(x), SC.oracle_labels(case, y), **SC.oracle_kwargs(case))
        g64 = torch.stack(g64.split(case["bsz"]), 1)
        assert abs(float(l64) - loss) <= 1e-5 * max(1.0, abs(loss)), (name, float(l64), loss)
        assert float((g64 - grad).abs().max()) <= 1e-4 * max(float(g64.abs().max()), 1e-5), name
        if grad.numel() <= FULL_LIMIT:
            out[f"grad_{name}"] = grad.numpy().astype(np.float32)
            meta[name] = "full"
        else:
            out[f"gstat_{name}"] = stats(grad)
            meta[name] = "stats"
        print(f"{name:24s} loss {loss:.7f}  fp64 {float(l64):.7f}  {meta[name]}")
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "supcon_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v for k, v in meta.items() if v not in ("full", "stats")})


if __name__ == "__main__":
    main()
