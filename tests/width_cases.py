"""The (hidden, heads, clip length) shapes of the composed path -- every shape the hidden-128 chains refuse -- and the path
the engine must take for each, or the limit that refuses it.  tests/test_width_admission_cpu.py checks every row against
the host-side admission predicates (engine.check_engine_shape / check_clip_shape); tests/test_width_shapes_gpu.py runs every
admitted row against the float64 oracle and checks that every refused row is refused before anything is enqueued.
VAL_CASES and VAL_CLIP_BOUNDS (at the end) are the validation forwards, whose routes training does not take.

All rows: Q = 8 queries, one decoder layer, n_class K, pad_idx K + 1, training step (forward + losses + backward).  Columns:
  variant -- "tf" token fusion, "bn" BN-blend fuser, "vary" activation-magnitude fuser, "plain" plain SA-Fuser (its
             batches carry 120 x 160 depth frames);
  pad     -- as in tests/chain_cases.py: "tail", "none" or a tuple of per-clip valid lengths;
  erank   -- weight of the effective-rank penalty (0: off);
  seam    -- the variant's own seam launch (SEAMS) runs: token fusion's fused embedding seam (embed.hip) at hidden <= 1024
             (past it: token_exchange + layernorm), the BN-blend, activation-magnitude and plain seams at every admitted
             hidden;
  tail1   -- the tail forward, the losses and the tail backward are ONE launch (r3d_decoder_tail_losses_supported:
             hidden <= 512, K + 1 <= 24);
  attn    -- the cross-attention core's route: "small" (mha_small.h: Lk <= 64, dh in {16, 32, 64, 128}) or "general"
             (decided inside attention.hip: the tests check the row against that rule and the launch's (Lq, Lk, dh));
  side    -- the query self-attention branch on a second stream (auto_side_stream: hidden >= 512);
  refuse  -- None (admitted) or a fragment of the ValueError message naming the limit."""
import collections

from tests import chain_cases as CC

Q = 8

Case = collections.namedtuple("Case", "B S H heads K variant pad erank seam tail1 attn side refuse why")


def _c(B, S, H, heads, K=17, variant="tf", pad="tail", erank=0.0, seam=True, tail1=True, attn="general", side=False,
       refuse=None, why=""):
    return Case(B, S, H, heads, K, variant, pad, erank, seam, tail1, attn, side, refuse, why)


CASES = [
    _c(2, 16, 40, 8, why="dh 5: every row slot e >= 1 empty"),
    _c(2, 16, 96, 8, why="dh 12, slot 1 half filled"),
    _c(2, 16, 136, 8, why="first EPL-8 width, slot 2 one eighth filled"),
    _c(2, 16, 200, 8, K=122, tail1=False, why="dh 25, NTU head (tail in three launches)"),
    _c(2, 16, 384, 6, attn="small", why="dh 64 on the small attention path"),
    _c(2, 16, 520, 8, tail1=False, side=True, why="first EPL-16 width, dh 65, side stream"),
    _c(2, 16, 768, 12, tail1=False, attn="small", side=True, why="dh 64 at a wide row"),
    _c(1, 12, 1032, 12, seam=False, tail1=False, side=True, why="past the seam: token_exchange + layernorm, dh 86"),
    _c(1, 8, 2048, 16, seam=False, tail1=False, attn="small", side=True, why="widest admitted hidden, dh 128"),
    _c(2, 16, 128, 4, attn="small", why="hidden 128 with 4 heads: both chains refused"),
    _c(2, 16, 128, 1, attn="small", why="hidden 128 with 1 head (dh 128)"),
    _c(1, 257, 128, 8, why="long clip, 5 key chunks"),
    _c(1, 1000, 128, 8, pad="none", why="long clip, S = 1000"),
    _c(3, 300, 128, 8, pad=(1, 150, 300), why="ragged long clips: 1, S/2 and S valid frames"),
    _c(1, 933, 1024, 8, pad="none", tail1=False, side=True, why="largest admitted S at hidden 1024 (dh 128)"),
    _c(2, 16, 136, 8, erank=0.05, why="rank penalty off the grid"),
    # the activation-magnitude fuser (varyfuse.hip seam; channel scores from |x| column sums in every mode)
    _c(2, 16, 200, 8, variant="vary", why="activation-magnitude fuser off the grid"),
    _c(2, 16, 520, 8, variant="vary", tail1=False, side=True, why="vary: first EPL-16 width, dh 65"),
    _c(2, 16, 1000, 8, variant="vary", tail1=False, side=True, why="vary: dh 125, last slot partly filled"),
    _c(2, 16, 1024, 8, variant="vary", tail1=False, attn="small", side=True, why="vary: widest seam, dh 128"),
    _c(2, 16, 384, 6, variant="vary", attn="small", why="vary: dh 64 on the small attention path"),
    _c(2, 16, 128, 4, variant="vary", attn="small", why="vary: hidden 128 with 4 heads, chains refused"),
    _c(3, 300, 128, 8, variant="vary", pad=(1, 150, 300), why="vary: ragged long clips"),
    _c(2, 16, 136, 8, variant="vary", erank=0.05, why="vary: rank penalty off the grid"),
    # the BN-blend fuser (bnfuse.hip seam; batch statistics in training)
    _c(2, 16, 200, 8, variant="bn", why="BN-blend fuser off the grid"),
    _c(2, 16, 520, 8, variant="bn", tail1=False, side=True, why="BN-blend fuser past the EPL-8 bracket"),
    _c(2, 16, 1000, 8, variant="bn", tail1=False, side=True, why="bn: dh 125, last slot partly filled"),
    _c(2, 16, 1024, 8, variant="bn", tail1=False, attn="small", side=True, why="bn: widest seam, dh 128"),
    _c(2, 16, 384, 6, variant="bn", attn="small", why="bn: dh 64 on the small attention path"),
    _c(2, 16, 128, 4, variant="bn", attn="small", why="bn: hidden 128 with 4 heads, chains refused"),
    _c(3, 300, 128, 8, variant="bn", pad=(1, 150, 300), why="bn: ragged long clips"),
    _c(2, 16, 136, 8, variant="bn", erank=0.05, why="bn: rank penalty off the grid"),
    # the plain SA-Fuser (plainfuse.hip seam in every mode; d modality_token from the seam's per-frame partials)
    _c(2, 16, 40, 8, variant="plain", why="plain: dh 5, every row slot e >= 1 empty"),
    _c(2, 16, 136, 8, variant="plain", why="plain: first EPL-8 width"),
    _c(2, 16, 200, 8, K=122, variant="plain", tail1=False, why="plain: dh 25, NTU head"),
    _c(2, 16, 384, 6, variant="plain", attn="small", why="plain: dh 64 on the small attention path"),
    _c(2, 16, 520, 8, variant="plain", tail1=False, side=True, why="plain: first EPL-16 width, dh 65"),
    _c(2, 16, 1000, 8, variant="plain", tail1=False, side=True, why="plain: dh 125, last slot partly filled"),
    _c(2, 16, 1024, 8, variant="plain", tail1=False, attn="small", side=True, why="plain: widest seam, dh 128"),
    _c(2, 16, 128, 4, variant="plain", attn="small", why="plain: hidden 128 with 4 heads, chains refused"),
    _c(1, 257, 128, 8, variant="plain", why="plain: long clip, 5 key chunks"),
    _c(3, 300, 128, 8, variant="plain", pad=(1, 150, 300), why="plain: ragged long clips"),
    _c(2, 16, 136, 8, variant="plain", erank=0.05, why="plain: rank penalty off the grid"),
    # refused: the engine (or the step) raises before any launch
    _c(1, 16, 1032, 8, seam=False, tail1=False, side=True, refuse="head width", why="dh 129: Lq * dh > 1024"),
    _c(1, 16, 1024, 4, tail1=False, side=True, refuse="head width", why="dh 256"),
    _c(1, 16, 256, 1, refuse="head width", why="dh 256 at hidden 256"),
    _c(1, 16, 1032, 12, variant="bn", seam=False, tail1=False, side=True, refuse="BN-blend", why="BN seam is C <= 1024"),
    _c(1, 16, 1032, 12, variant="vary", seam=False, tail1=False, side=True, refuse="activation-magnitude",
       why="vary seam is C <= 1024"),
    _c(1, 16, 1032, 12, variant="plain", tail1=False, side=True, refuse="plain SA-Fuser", why="plain seam is C <= 1024"),
    _c(1, 16, 1024, 4, variant="plain", tail1=False, side=True, refuse="head width", why="plain: dh 256"),
    _c(1, 16, 1024, 4, variant="vary", tail1=False, side=True, refuse="head width", why="vary: dh 256"),
    _c(1, 934, 1024, 8, variant="plain", pad="none", tail1=False, side=True, refuse="clip length",
       why="plain: first S past the backward attention LDS at dh 128"),
    _c(1, 1606, 128, 8, pad="none", refuse="clip length", why="first S past the backward attention LDS at dh 16"),
    _c(1, 934, 1024, 8, pad="none", tail1=False, side=True, refuse="clip length",
       why="first S past the backward attention LDS at dh 128"),
    _c(1, 16, 2056, 8, seam=False, tail1=False, side=True, refuse="hidden 2056 > 2048", why="past the widest row kernel"),
]

# the boundaries the refused rows name: (H, heads, last admitted training S, first refused training S)
CLIP_BOUNDS = [(128, 8, 1605, 1606), (512, 8, 1317, 1318), (1024, 8, 933, 934)]

# the variants' own seam launches (r3d_amd.ops attributes), and the hidden-128 chain's seam-free route
SEAMS = {"tf": "embed_fuse_fwd", "bn": "bn_blend_fwd", "vary": "scaled_exchange_fwd", "plain": "plain_fuse_fwd"}
DEPTH_HW = {"plain": (120, 160)}               # the plain model's 160 x 120 depth projection; the others take 224 x 224

# validation forwards (validate()'s own call: forward(..., "val", need_grad=False)), B 2, S 16, no padding:
# (variant, H, heads).  At hidden > 128 token fusion skips its seam (train mode only) and, like the activation-magnitude
# fuser, selects from |x| column sums (colabssum + token_select); the BN-blend fuser runs on running statistics.
VAL_CASES = ([(v, H, 8) for v in ("tf", "bn", "vary", "plain") for H in (40, 136, 520, 1000)] +
             [("tf", 1032, 12), ("tf", 2048, 16)])

# the forward-only clip bound (validation at B 1): (H, heads, last admitted S, first refused S, the limit's message).  At
# hidden 128 the attention core would admit 2416 keys, so pos_embedding's max_pos_len rows decide.
VAL_CLIP_BOUNDS = [(128, 8, 2000, 2001, "max_pos_len"), (1024, 8, 1464, 1465, "clip length")]


def case_id(c):
    p = c.pad if isinstance(c.pad, str) else "ragged"
    v = "" if c.variant == "tf" else f"-{c.variant}"
    e = "-erank" if c.erank else ""
    return f"B{c.B}-S{c.S}-H{c.H}x{c.heads}-K{c.K}{v}-{p}{e}"


def engine_refused(c):
    """The row is refused when the engine is built (its hidden / heads / variant), not only at its clip length."""
    return c.refuse is not None and c.refuse != "clip length"


def make_batch(c, seed=CC.BATCH_SEED):
    return CC.make_batch(c, seed, depth_hw=DEPTH_HW.get(c.variant, (224, 224)))


def val_id(v):
    return f"{v[0]}-H{v[1]}x{v[2]}"
