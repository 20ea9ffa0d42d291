"""Pinned cases of the three-modality fuser (csrc/fuser3.hip, model/cmfuser3.py) for tests/test_fuser3_cpu.py and
tests/test_fuser3_gpu.py, their seeded inputs, and the tolerances of the attention core and of the whole model.

The tolerances are MEASURED ON THE CPU FROM THE REFERENCE ALONE, never from the kernel: the float32 evaluation of
tests/fuser3_oracle.py against its float64 evaluation, over every case below, in the test's own error measure; the test
allows 8 times the largest ratio (a wave tree reduction and expf against torch's serial sum and exp).  Reproduce with

    python -m tests.fuser3_cases

which printed (largest ratio per output; every case's own line is left out here):

    attn3 saturated, against the condition size: d_q 1.18e-08   d_k 9.64e-09
    attn3 all cases: probs 5.14e-08   out 8.67e-08   d_q 4.30e-01   d_k 5.00e-01   d_v 1.06e-07
    attn3 unsaturated cases: probs 5.14e-08   out 8.67e-08   d_q 2.34e-07   d_k 1.67e-07   d_v 1.06e-07
    model fused / d input 7.96e-07   parameter gradients 8.66e-07
"""
import numpy as np
import torch

from oracle import synth

# ---------------------------------------------------------------------------------------------------------------------
# attn3 kernel cases: (N, C, heads, variant)
# ---------------------------------------------------------------------------------------------------------------------
ATTN_CASES = [
    (1, 1, 1, "plain"),        # dh = 1
    (3, 48, 3, "plain"),       # dh = 16; 9 units, so the last workgroup (4 waves) is partly filled
    (5, 63, 1, "plain"),       # dh just under one lane slot
    (2, 128, 2, "plain"),      # dh = 64, exactly one slot
    (2, 65, 1, "plain"),       # dh = 65, one lane of the second slot
    (3, 192, 2, "plain"),      # dh = 96
    (2, 127, 1, "plain"),      # dh = 127
    (2, 128, 1, "plain"),      # dh = 128, one head
    (4, 1024, 8, "plain"),     # dh = 128, the configs[4] shape
    (67, 64, 4, "plain"),      # 268 units, many workgroups
    (3, 192, 2, "sat"),        # q and k scaled by 30: the softmax saturates, expf underflows on one side
    (3, 192, 2, "q0"),         # q = 0: every probability is exactly 0.5
]

# |got - ref| <= tol (|ref| + largest |ref| in the same frame's rows of that tensor); 8 x the measured ratios above.
# ATTN_TOL is the largest over ALL cases.  For d_q and d_k that largest ratio comes from the saturated variant alone and
# leaves a bound of order 1: there d s = p (d p - sum p d p) cancels below float32's reach, so float32 itself is wrong by
# the size of the answer.  So that this does not blunt the other eleven cases, they are held to ATTN_TOL_UNSATURATED (the
# largest over them only, never looser than ATTN_TOL), and the saturated variant's d_q / d_k are held IN ADDITION to
# ATTN_TOL_CONDITION times the size of the cancelling terms (fuser3_oracle.attn3_grad_condition), measured the same way.
ATTN_TOL = {"probs": 8 * 5.14e-08, "out": 8 * 8.67e-08, "d_q": 8 * 4.30e-01, "d_k": 8 * 5.00e-01, "d_v": 8 * 1.06e-07}
ATTN_TOL_UNSATURATED = dict(ATTN_TOL, d_q=8 * 2.34e-07, d_k=8 * 1.67e-07)
ATTN_TOL_CONDITION = {"d_q": 8 * 1.18e-08, "d_k": 8 * 9.64e-09}


def attn_tol(variant):
    return ATTN_TOL if variant == "sat" else ATTN_TOL_UNSATURATED


# ---------------------------------------------------------------------------------------------------------------------
# exchange / triple mean kernel cases: (N, C); each runs with and without a keep mask, under every mask kind
# ---------------------------------------------------------------------------------------------------------------------
ROW_CASES = [
    (1, 4),                    # one frame, k = 1
    (7, 100),                  # odd rows, width off the 64 grid
    (5, 130),                  # C % 4 != 0
    (256, 1024),               # the configs[4] shape
    (343, 1021),               # 3 N C = 1,050,609 > 4096 x 256: the loops over 3 N C elements go round a second time
    (1027, 1023),              # N C = 1,050,621: the same for the loops over N C elements
]
MASK_KINDS = ("zero",          # nothing exchanged
              "one",           # modality 1 takes every channel of modality 2, the others none
              "overlap")       # C // 4 ones per modality at three shifted index sets: own-slot and fed-slot terms both live
DROP_P = 0.1                   # embd_drop

# ---------------------------------------------------------------------------------------------------------------------
# model cases: (B, S, H, heads, mode, training)
# ---------------------------------------------------------------------------------------------------------------------
MODEL_CASES = [
    (1, 1, 96, 1, "val", False),       # one frame, dh = 96: about half of each post-ReLU stream scores exactly 0 (ties)
    (1, 1, 96, 1, "train", True),
    (1, 7, 100, 4, "val", True),       # dh = 25, width off the 64 grid
    (1, 7, 100, 4, "train", False),
    (2, 3, 130, 2, "val", False),      # dh = 65, H % 4 != 0: the GEMMs take their scalar-load twins
    (2, 3, 130, 2, "train", True),
    (2, 5, 64, 4, "val", True),        # the smallest case of the eval-state test
    (2, 5, 64, 4, "train", True),
    (3, 5, 256, 2, "val", True),       # dh = 128
    (3, 5, 256, 2, "train", False),
]
BIG_TRAINING_CASE = (16, 16, 1024, 8, "train", True)      # configs[4]: the training-state twin of the eval-state test's case
EVAL_STATE_CASES = [(2, 5, 64, 4, "train"), (16, 16, 1024, 8, "train"), (4, 8, 256, 8, "val")]    # the eval-state test's own

# error against tensor scale (max |got - ref| / max |ref|), 8 x the measured ratios above; never looser than the 1e-3 / 2e-3
# of the eval-state test
MODEL_TOL = min(8 * 7.96e-07, 1e-3)
MODEL_TOL_PARAM = min(8 * 8.66e-07, 2e-3)

MIN_SCORE_GAP_ULP = 64         # k-th and (k + 1)-th smallest validation scores: bit-equal or at least this far apart


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs (float32, exactly representable hash fills)
# ---------------------------------------------------------------------------------------------------------------------
def _sym(shape, stream):
    return torch.from_numpy(synth.symmetric(int(np.prod(shape)), stream).reshape(shape)).clone()


def attn_inputs(N, C, heads, variant):
    """-> (qkv [3N, 3C], d_out [3N, C]) float32"""
    qkv = _sym((3 * N, 3 * C), 0xF3A000 + 131 * N + C)
    if variant == "sat":
        qkv[:, :2 * C] *= 30.0
    elif variant == "q0":
        qkv[:, :C] = 0.0
    return qkv, _sym((3 * N, C), 0xF3B000 + 131 * N + C)


def exchange_mask(kind, C):
    """[3, C] float32 of 1.0 / 0.0"""
    mask = torch.zeros(3, C)
    if kind == "one":
        mask[1] = 1.0
    elif kind == "overlap":
        k = max(1, C // 4)
        s = max(1, k // 3)
        for m in range(3):
            mask[m, (m * s + torch.arange(k)) % C] = 1.0
    return mask


def keep_mask(rows, C, stream=0xF3D000):
    """[rows, C] uint8 keep mask of density 1 - DROP_P"""
    return torch.from_numpy((synth.uniform01(rows * C, stream + rows) >= DROP_P).astype(np.uint8).reshape(rows, C))


def row_inputs(N, C):
    """-> (three streams [N, C], a cotangent / stacked tensor [3N, C], a frame tensor [N, C]) float32, not on the 2^-23 grid"""
    xs = [(_sym((N, C), 0xF3C000 + 7 * m + N) * 1.7).float() for m in range(3)]
    return xs, (_sym((3 * N, C), 0xF3C100 + N) * 1.3).float(), (_sym((N, C), 0xF3C200 + N) * 0.9).float()


PARAM_PREFIX = "fuser."


def param_shapes(H):
    """CMFuser3(H)'s named_parameters(), in order (tests/test_fuser3_cpu.py holds this list against the module)."""
    b = "blocks.0."
    return [("modality_token", (1, 1, 1, H)),
            (b + "norm1.weight", (H,)), (b + "norm1.bias", (H,)), (b + "attn.qkv.weight", (3 * H, H)),
            (b + "attn.proj.weight", (H, H)), (b + "attn.proj.bias", (H,)), (b + "norm2.weight", (H,)), (b + "norm2.bias", (H,)),
            (b + "mlp.mlp.0.weight", (4 * H, H)), (b + "mlp.mlp.0.bias", (4 * H,)), (b + "mlp.mlp.2.weight", (H, 4 * H)),
            (b + "mlp.mlp.2.bias", (H,)), ("norm.weight", (H,)), ("norm.bias", (H,)),
            ("projection.weight", (H, H)), ("projection.bias", (H,)),
            ("fusion_conv.weight", (1, 2, 1, 1)), ("fusion_conv.bias", (1,))]


LIVE = tuple(PARAM_PREFIX + n for n, _ in param_shapes(1)[1:14])        # the 13 parameters that receive gradient


def model_params(H):
    """name ("fuser." + ...) -> float32 tensor: the fill the eval-state test gives the module."""
    vals = synth.fill_state([(PARAM_PREFIX + n, s) for n, s in param_shapes(H)])
    return {n: torch.from_numpy(v).clone() for n, v in vals.items()}


def model_inputs(B, S, H):
    """-> (three streams [B, S, H], cotangent [B, S, H]) float32: the eval-state test's inputs (two streams after a ReLU)."""
    xs = [_sym((B, S, H), 0xF3000 + 17 * m) for m in range(3)]
    xs[0] = xs[0].relu()
    xs[1] = xs[1].relu() * 0.7
    return xs, _sym((B, S, H), 0xF3900)


# ---------------------------------------------------------------------------------------------------------------------
# error measures (shared by the tests and by the measurement below)
# ---------------------------------------------------------------------------------------------------------------------
def frame_ratio(got, ref, rows_per_frame=3):
    """max over elements of |got - ref| / (|ref| + s), s = the largest |ref| in the same frame's rows; got / ref: [F * r, W]"""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = (got - ref).abs().reshape(-1, rows_per_frame * ref.shape[-1])
    if bool(torch.isnan(d).any()):
        return float("inf")
    r = ref.abs().reshape(d.shape)
    den = r + r.max(dim=1, keepdim=True).values
    return float(torch.where(den > 0, d / den, torch.where(d > 0, torch.full_like(d, float("inf")), d)).max())


def attn_ratios(got_probs, got_out, got_dqkv, ref_probs, ref_out, ref_dqkv):
    """the five frame ratios of one attn3 case; probs [N, heads, 3, 2] is judged per frame (its 6 heads values)"""
    N, C = ref_probs.shape[0], ref_out.shape[1]
    out = {"probs": frame_ratio(got_probs.reshape(N, -1), ref_probs.reshape(N, -1), 1), "out": frame_ratio(got_out, ref_out)}
    for i, n in enumerate(("d_q", "d_k", "d_v")):
        out[n] = frame_ratio(got_dqkv[:, i * C:(i + 1) * C], ref_dqkv[:, i * C:(i + 1) * C])
    return out


def condition_ratios(got_dqkv, ref_dqkv, c_q, c_k):
    """max over elements of |got - ref| / (the frame's condition size), for the d_q and d_k thirds"""
    C = ref_dqkv.shape[1] // 3
    out = {}
    for i, (n, c) in enumerate((("d_q", c_q), ("d_k", c_k))):
        d = (got_dqkv[:, i * C:(i + 1) * C].double().cpu() - ref_dqkv[:, i * C:(i + 1) * C].double()).abs().reshape(c.shape[0], -1)
        out[n] = float("inf") if bool(torch.isnan(d).any()) else float((d / c.double()[:, None]).max())
    return out


def scale_ratio(got, ref):
    """the eval-state test's measure: max |got - ref| / max(max |ref|, 1e-6)"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = (got - ref).abs().max()
    return float("inf") if bool(torch.isnan(d)) else float(d) / max(float(ref.abs().max()), 1e-6)


def model_reference(case, dtype, keep=None, drop_scale=1.0 / (1.0 - DROP_P)):
    """cm_fuser3 and its autograd gradients for one model case in `dtype` -> (fused, aux, input grads, {name: grad})."""
    from tests import fuser3_oracle as F3
    B, S, H, heads, mode, training = case
    xs, cot = model_inputs(B, S, H)
    p = {n: v.to(dtype).requires_grad_(n in LIVE) for n, v in model_params(H).items()}
    xs = [x.to(dtype).requires_grad_(True) for x in xs]
    fused, aux = F3.cm_fuser3(p, xs, mode, heads, keep if training else None, drop_scale)
    (fused * cot.to(dtype)).sum().backward()
    return fused.detach(), aux, [x.grad for x in xs], {n: p[n].grad for n in LIVE}


def _measure():
    from tests import fuser3_oracle as F3
    worst, unsat = {}, {}
    for N, C, heads, variant in ATTN_CASES:
        qkv, d_out = attn_inputs(N, C, heads, variant)
        ref = F3.attn3(qkv.double(), heads) + (F3.attn3_adjoint(qkv.double(), d_out.double(), heads),)
        got = F3.attn3(qkv, heads) + (F3.attn3_adjoint(qkv, d_out, heads),)
        r = attn_ratios(*got, *ref)
        print(f"attn3 {(N, C, heads, variant)}: " + "  ".join(f"{k} {v:.2e}" for k, v in r.items()))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            if variant != "sat":
                unsat[k] = max(unsat.get(k, 0.0), v)
        if variant == "sat":
            c = condition_ratios(got[2], ref[2], *F3.attn3_grad_condition(qkv.double(), d_out.double(), heads))
            print("attn3 saturated, against the condition size: " + "   ".join(f"{k} {v:.2e}" for k, v in c.items()))
    print("attn3 all cases: " + "   ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print("attn3 unsaturated cases: " + "   ".join(f"{k} {v:.2e}" for k, v in unsat.items()))
    w_io = w_par = 0.0
    for case in MODEL_CASES + [BIG_TRAINING_CASE] + [c + (False,) for c in EVAL_STATE_CASES]:
        B, S, H = case[:3]
        keep = keep_mask(3 * B * S, H)
        f64, _, gx64, gp64 = model_reference(case, torch.float64, keep)
        f32, _, gx32, gp32 = model_reference(case, torch.float32, keep)
        io = max([scale_ratio(f32, f64)] + [scale_ratio(a, b) for a, b in zip(gx32, gx64)])
        par = max(scale_ratio(gp32[n], gp64[n]) for n in LIVE)
        print(f"model {case}: fused / d input {io:.2e}   parameter gradients {par:.2e}")
        w_io, w_par = max(w_io, io), max(w_par, par)
    print(f"model fused / d input {w_io:.2e}   parameter gradients {w_par:.2e}")


if __name__ == "__main__":
    _measure()
