"""Shared helpers for the parity tests (fixtures -> parameters / batches)."""
import json
import os

import numpy as np
import torch

from oracle import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture(tag):
    z = np.load(os.path.join(GOLDEN, f"{tag}.npz"), allow_pickle=False)
    fx = {k: z[k] for k in z.files}
    fx["meta"] = json.loads(str(fx["meta"]))
    for k in ("param_names", "param_shapes", "live_names", "ckpt_files", "ckpt_keys"):
        if k in fx:
            fx[k] = json.loads(str(fx[k]))
    return fx


def fixture_params(fx):
    """dict name -> torch tensor, regenerated bit-identically from the hash fill."""
    return {n: torch.from_numpy(synth.fill_value(n, tuple(s), j))
            for j, (n, s) in enumerate(zip(fx["param_names"], fx["param_shapes"]))}


def fixture_batch(fx, seed=None, **kw):
    m = fx["meta"]
    b = synth.make_batch(m["B"], m["S"], m["n_class"], m["pad_idx"], m["seed"] if seed is None else seed,
                         zero_mean_depth=m.get("zero_mean_depth", False), **kw)
    return [torch.from_numpy(x) for x in b]


def stats(t):
    a = t.detach().double().reshape(-1).cpu()
    n = a.numel()
    idx = torch.linspace(0, n - 1, steps=min(n, 16)).long()
    return np.concatenate([[float(a.norm()), float(a.sum()), float(a.abs().sum())],
                           a[:16].numpy() if n >= 16 else np.pad(a.numpy(), (0, 16 - n)),
                           a[idx].numpy() if n >= 16 else np.pad(a[idx].numpy(), (0, 16 - idx.numel()))])


def assert_close(a, b, rtol=1e-3, atol=1e-5, what=""):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    if a.numel() == 0:
        return
    err = (a - b).abs()
    lim = atol + rtol * b.abs()
    bad = err > lim
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{a.numel()} outside tol; max abs err "
                                 f"{float(err.max()):.3e}, ref scale {float(b.abs().max()):.3e}")


def ffn_kink_units(ffn_pre):
    """ReLU units of the decoder FFN whose pre-activation is within rounding of zero in the oracle (ffn_pre: the oracle's
    per-layer pre-activations, aux["ffn_pre"]): the fp32 product may land on the other side of the kink, which flips that
    unit's contribution (its row of linear1's gradient entirely, everything upstream by the unit's share).  Identified BY
    CONSTRUCTION from the oracle: |u| <= 2e-6 max|u|, the size of the fp32 accumulation error of a K = H dot product.
    Returns {(layer, unit)}."""
    units = set()
    for l, u in enumerate(ffn_pre):
        near = (u.abs() <= 2e-6 * float(u.abs().max())).reshape(-1, u.shape[-1])
        units |= {(l, int(j)) for j in near.any(dim=0).nonzero().flatten()}
    return units


def without_kink_units(n, g, r, units):
    """(g, r) -- the kernel's and the oracle's gradient of parameter n -- with the rows of linear1 (weight and bias) and the
    columns of linear2.weight of the kink units removed; other parameters pass through unchanged."""
    for (l, j) in units:
        if n in (f"transformer.decoder.layers.{l}.linear1.weight", f"transformer.decoder.layers.{l}.linear1.bias"):
            keep = torch.ones(r.shape[0], dtype=torch.bool)
            keep[j] = False
            g, r = g[keep], r[keep]
        elif n == f"transformer.decoder.layers.{l}.linear2.weight":
            keep = torch.ones(r.shape[1], dtype=torch.bool)
            keep[j] = False
            g, r = g[:, keep], r[:, keep]
    return g, r
