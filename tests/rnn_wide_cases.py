"""Pinned shapes of the stepwise LSTM recurrence (csrc/lstm_steps.hip, opts --wide_rnn) for tests/test_rnn_wide_cpu.py and
tests/test_rnn_wide_gpu.py, the float64 reference of each and the bounds the kernels are held to.

The bounds are measured, not chosen: per case and tensor, e32 = max|f32 - f64| where f32 is tests/rnn_oracle.lstm_layer_grads
run on the float32 casts of the same inputs (the oracle is dtype-agnostic).  The bound is max(8 e32, 2e-6 max|ref|): 8x is the
project's margin for a different summation order (cnn_cases, l3_cases, m3_cases), the floor is 16 fp32 ulp of the tensor's
scale for the device's expf / tanhf, which are not correctly rounded.  A tensor whose reference is identically zero must come
back exactly zero.  CAP is the condition 8 e32 <= 2e-5 max|ref| that the CPU test asserts of every case and tensor, so that a
reference that loses its own precision cannot widen a bound unnoticed."""
import functools

import torch

from tests import rnn_oracle as RO

# (B, S, H): each chosen for one edge, none the workload's size
KERNEL_CASES = [
    (1, 1, 264),        # the smallest wide hidden; h = 132: a partial unit tile and a contraction tail; a single step
    (1, 2, 1024),       # the widest
    (8, 16, 512),
    (13, 37, 1024),     # a partial clip tile
    (5, 3, 520),        # h = 260
    (17, 5, 776),       # a second clip tile with one clip in it
    (16, 2, 272),       # exactly one full clip tile
    (33, 3, 1000),      # h = 500; three clip tiles
    (2, 130, 264),
    (2, 520, 264),      # a long walk: 2080 launches
]
# the steps route forced where the registers route exists too (h = 4 is less than one unit tile)
NARROW_CASES = [(8, 16, 128), (1, 2, 8), (13, 37, 136)]
ALL_CASES = KERNEL_CASES + NARROW_CASES

# engine_rnn.check_rnn_shape(..., wide=True)
ADMITTED_WIDE_H = (8, 128, 256, 264, 512, 1000, 1024)
REFUSED_WIDE_H = (0, 4, 12, 260, 1028, 1032, 2048)

TENSORS = ("y", "gates", "cell", "hprev", "dg", "dx", "dw_ih", "db_ih", "dw_hh", "db_hh")
MARGIN, FLOOR, CAP = 8.0, 2e-6, 2e-5


def seed(B, S, H):
    return B * 1000 + S * 7 + H


def inputs(B, S, H):
    from tests.test_rnn_gpu import _layer_inputs
    return _layer_inputs(B, S, H, seed=seed(B, S, H))


def by_tensor(r, N, H):
    """tests/rnn_oracle.lstm_layer_grads' result as one 2-D (or 1-D) tensor per name of TENSORS, in the kernels' layouts."""
    out = {k: r[k].reshape(N, -1) for k in ("y", "gates", "cell", "hprev", "dg")}
    out["dx"] = r["dx"].reshape(N, H)
    out["dw_ih"] = torch.cat(r["dw_ih"], 0)
    out["db_ih"] = torch.cat(r["db"])
    out["dw_hh"] = torch.cat(r["dw_hh"], 0)
    out["db_hh"] = torch.cat(r["db"])
    return out


@functools.lru_cache(maxsize=None)
def reference(B, S, H):
    """(ref, bounds): ref[name] float64; bounds[name] = (bound, e32, scale).  Computed once per case and shared."""
    w, x, dy = inputs(B, S, H)
    ref = by_tensor(RO.lstm_layer_grads(x, w, dy), B * S, H)
    f32 = by_tensor(RO.lstm_layer_grads(x.float(), {k: v.float() for k, v in w.items()}, dy.float()), B * S, H)
    bounds = {}
    for k in TENSORS:
        assert f32[k].dtype == torch.float32 and ref[k].dtype == torch.float64
        e32 = float((f32[k].double() - ref[k]).abs().max())
        scale = float(ref[k].abs().max())
        bounds[k] = (max(MARGIN * e32, FLOOR * scale), e32, scale)
    return ref, bounds


def check(got, B, S, H, what=""):
    """got[name]: float tensors in by_tensor's layouts.  Prints each figure, then asserts the bounds."""
    ref, bounds = reference(B, S, H)
    bad = []
    for k in TENSORS:
        g = got[k].detach().cpu().double()
        assert g.shape == ref[k].shape, (k, g.shape, ref[k].shape)
        bound, e32, scale = bounds[k]
        finite = bool(torch.isfinite(g).all())
        err = float((g - ref[k]).abs().max()) if finite else float("inf")
        print(f"{what} B{B} S{S} H{H} {k}: err {err:.3e} bound {bound:.3e} e32 {e32:.3e} scale {scale:.3e}")
        if scale == 0.0:
            if not (finite and bool((g == 0).all())):
                bad.append((k, err, "reference is identically zero"))
        elif not err <= bound:
            bad.append((k, err, bound))
    assert not bad, (what, B, S, H, bad)
