"""The (hidden, heads, clip length, decoder depth) shapes of the two query models that run through r3d_amd/engine_unsup.py --
the depth-as-query model (model/futr_unsupervised_depth.py, "depth") and the label-query model (model/futr_proposed.py,
"label") -- and the attention route each must take, or the limit that refuses it.  tests/test_query_admission_cpu.py checks
every row against the host-side admission predicates (engine_unsup.check_query_engine_shape / check_query_clip_shape);
tests/test_query_shapes_gpu.py runs every admitted row against the float64 oracle and checks that every refused row is
refused before anything is enqueued.

Every clip brings S queries, so both decoder attentions run Lq = Lk = S.  All rows: Q = 8 pooled queries, n_class K, pad_idx
K + 1.  Columns:
  variant -- "depth" (a training step: forward + losses + backward) or "label" (forward + the autograd bridge's gradients of
             tests/test_proposed_cpu.probe_loss; the label model has no fused loss);
  pad     -- as in tests/chain_cases.py: "tail", "none" or a tuple of per-clip valid lengths;
  hw      -- the depth frame (height, width) of a "depth" row: the depth projection's input width;
  attn    -- the attention cores' route: "small" (mha_small.h: Lq = 8, Lk <= 64, dh in {16, 32, 64, 128}, so S = 8) or
             "general" (decided inside attention.hip: the tests check the row against that rule and the launch's (Lq, Lk, dh));
  fwd     -- a forward alone (need_grad=False) is admitted at the row's shape;
  refuse  -- None (admitted) or a fragment of the ValueError message naming the limit."""
import collections

import numpy as np
import torch

from oracle import synth

Q = 8
SMALL_HW, FULL_HW = (12, 16), (120, 160)        # (FULL_HW: the reference's 160 x 120 depth frames, split-K projection)
QUERY_NUM = 48                                  # label rows: query_embed rows; the indices used are < N_USED (they repeat)
N_USED = 7

Case = collections.namedtuple("Case", "variant B S H heads n_dec K pad hw attn fwd refuse why")


def _c(variant, B, S, H, heads, n_dec=1, K=17, pad="tail", hw=SMALL_HW, attn="general", fwd=True, refuse=None, why=""):
    return Case(variant, B, S, H, heads, n_dec, K, pad, hw, attn, fwd, refuse, why)


CASES = [
    _c("depth", 2, 1, 128, 8, pad="none", why="one frame per clip (Lq = Lk = 1)"),
    _c("depth", 2, 7, 40, 8, why="S < Q: the pooling windows overlap and repeat; dh 5"),
    _c("depth", 2, 8, 128, 8, attn="small", why="S = 8 at dh 16: the small attention kernels"),
    _c("depth", 1, 8, 1024, 8, attn="small", why="S = 8 at dh 128: the small kernels at their widest head"),
    _c("depth", 2, 9, 128, 8, why="S = 9 at dh 16: Lq * dh just above 128 (16 output slots)"),
    _c("depth", 2, 64, 128, 8, why="S = 64 at dh 16: Lq * dh = 1024, the longest training clip there"),
    _c("depth", 1, 112, 64, 8, pad="none", why="S = 112 at dh 8: the longest training clip, two key chunks"),
    _c("depth", 3, 40, 200, 8, pad=(1, 20, 40), hw=FULL_HW, why="ragged keys at dh 25, S = 40 (its longest clip)"),
    _c("depth", 2, 15, 520, 8, hw=FULL_HW, why="dh 65"),
    _c("depth", 1, 4, 2048, 8, pad="none", why="hidden 2048 / 8 heads: dh 256, S = 4"),
    _c("depth", 2, 16, 64, 1, why="one head (dh 64, S = 16: its longest clip)"),
    _c("depth", 2, 12, 96, 6, why="six heads (dh 16)"),
    _c("depth", 2, 11, 64, 8, n_dec=3, why="three decoder layers"),
    _c("depth", 2, 16, 128, 8, K=122, why="NTU-sized head, K = 122"),
    _c("label", 2, 5, 32, 8, why="label queries, S = 5 at dh 4"),
    _c("label", 2, 9, 128, 8, n_dec=2, why="label queries, S = 9, two decoder layers"),
    _c("label", 1, 64, 128, 8, pad="none", why="label queries, S = 64"),
    # refused: the engine (or the step) raises before any launch
    _c("depth", 1, 65, 128, 8, pad="none", fwd=False, refuse="clip length", why="dh 16: S * dh = 1040 > 1024"),
    _c("depth", 1, 17, 512, 8, pad="none", fwd=False, refuse="clip length", why="dh 64: S * dh = 1088 > 1024"),
    _c("depth", 1, 113, 64, 8, pad="none", fwd=True, refuse="clip length",
       why="dh 8: past the backward's LDS, within the forward's"),
    _c("depth", 1, 4, 2048, 4, pad="none", fwd=False, refuse="head width 512", why="dh 512: no clip length trains"),
    _c("depth", 1, 4, 2056, 8, pad="none", fwd=False, refuse="hidden 2056 > 2048", why="past the widest row kernel"),
]

# the longest training clip by head width (H, heads, head width, last admitted S); README's table is generated from these
QUERY_BOUNDS = [(32, 8, 4, 114), (64, 8, 8, 112), (128, 8, 16, 64), (200, 8, 25, 40), (512, 8, 64, 16), (1024, 8, 128, 8),
                (2048, 8, 256, 4), (2048, 4, 512, 0)]

BATCH_SEED = 91


def case_id(c):
    p = c.pad if isinstance(c.pad, str) else "ragged"
    return f"{c.variant}-B{c.B}-S{c.S}-H{c.H}x{c.heads}-L{c.n_dec}-K{c.K}-{p}"


def engine_refused(c):
    """The row is refused when the engine is built (its hidden / heads), not only at its clip length."""
    return c.refuse is not None and c.refuse != "clip length"


def small_route(S, dh):
    """attention.hip mha_small_ok restated for the engine's operands (16-byte aligned slices of 16-byte aligned rows)."""
    return S == Q and S <= 64 and dh in (16, 32, 64, 128)


def make_batch(c, seed=BATCH_SEED):
    """[features, depth (a "depth" row) or label indices [B, S] (a "label" row), past_label, trans_dur_future,
    trans_future_target] (torch, CPU)."""
    pad_idx = c.K + 1
    b = synth.make_batch(c.B, c.S, c.K, pad_idx, seed, depth_hw=c.hw if c.variant == "depth" else (1, 1),
                         pad_tail=(c.pad == "tail"))
    if not isinstance(c.pad, str):
        assert len(c.pad) == c.B and all(1 <= n <= c.S for n in c.pad)
        for i, n in enumerate(c.pad):
            b[0][i, n:] = 0.0
            b[1][i, n:] = 0.0
            b[2][i, n:] = pad_idx
    if c.variant == "label":
        b[1] = synth.randint(c.B * c.S, N_USED, (seed << 8) + 77).reshape(c.B, c.S).astype(np.int64)
    return [torch.from_numpy(np.ascontiguousarray(x)) for x in b]
