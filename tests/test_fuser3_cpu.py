"""What the GPU tests of the three-modality fuser rest on (tests/fuser3_oracle.py), pinned without a GPU:

  * the float64 whole (cm_fuser3, no keep mask) is oracle.cm_fuser_m at M = 3 to float32 rounding, with equal index sets, on
    the inputs of the eval-state GPU test;
  * with the third stream removed it is oracle.cm_fuser, the function the reference fixtures pin -- the exchange and the
    attention piece separately, and the whole;
  * the hand-written adjoints are autograd of the float64 forwards to 1e-12;
  * no model case's validation selection sits on a near-tie, so the GPU tests may compare index sets."""
import numpy as np
import pytest
import torch

from oracle import futr_oracle as O
from tests import fuser3_cases as FC, fuser3_oracle as F3


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


def test_param_list_is_the_modules():
    from r3d_amd.model.cmfuser3 import CMFuser3
    fz = CMFuser3(8, depth=1, num_heads=2)
    assert [(n, tuple(p.shape)) for n, p in fz.named_parameters()] == FC.param_shapes(8)
    assert len(FC.LIVE) == 13


@pytest.mark.parametrize("B,S,H,heads,mode", FC.EVAL_STATE_CASES + [(1, 1, 96, 1, "val")])
def test_float64_whole_is_the_float32_restatement_at_three_modalities(B, S, H, heads, mode, oracle_lib):
    xs, _ = FC.model_inputs(B, S, H)
    p = FC.model_params(H)
    want, aux = O.cm_fuser_m(p, xs, mode, heads)
    got, mine = F3.cm_fuser3({n: v.double() for n, v in p.items()}, [x.double() for x in xs], mode, heads)
    for m in range(3):
        assert np.array_equal(mine["idx"][m].numpy(), np.sort(aux["idx"][m].numpy())), m
    # float32 rounding of the restatement itself: tests/fuser3_cases.py measures 8e-7 of scale for float32 against float64
    assert FC.scale_ratio(want, got) <= FC.MODEL_TOL


@pytest.mark.parametrize("mode", ["train", "val"])
def test_two_modality_form_is_the_reference_pinned_fuser(mode, oracle_lib):
    B, S, H, heads = 2, 5, 64, 4
    xs, _ = FC.model_inputs(B, S, H)
    xs = xs[:2]
    p = FC.model_params(H)
    p64 = {n: v.double() for n, v in p.items()}
    want, aux = O.cm_fuser(p, xs[0], xs[1], mode, heads)
    got, mine = F3.cm_fuser3(p64, [x.double() for x in xs], mode, heads)
    assert np.array_equal(mine["idx"][0].numpy(), np.sort(aux["idx_rgb"].numpy()))
    assert np.array_equal(mine["idx"][1].numpy(), np.sort(aux["idx_dep"].numpy()))
    assert FC.scale_ratio(want, got) <= FC.MODEL_TOL
    # the exchange piece: oracle.token_fusion's stack, exactly (a select)
    stacked = O.token_fusion(xs[0], xs[1], mode)[0].reshape(B * S * 2, H)
    assert torch.equal(F3.exchange3([x.reshape(B * S, H) for x in xs], mine["mask"].float()), stacked)
    # the attention piece: oracle.fuser_block's masked softmax over two tokens (each attends to the other, p = 1)
    pre = "fuser.blocks.0."
    h1 = O.layer_norm(stacked.double(), p64[pre + "norm1.weight"], p64[pre + "norm1.bias"])
    qkv = h1 @ p64[pre + "attn.qkv.weight"].t()
    q, k, v = qkv.reshape(B * S, 2, 3, heads, H // heads).permute(2, 0, 3, 1, 4)
    att = (q @ k.transpose(-2, -1)) * (H // heads) ** -0.5
    att = (att + torch.eye(2).masked_fill(torch.eye(2) == 1, float("-inf"))).softmax(dim=-1)
    ref = (att @ v).transpose(1, 2).reshape(B * S * 2, H)
    probs, out = F3.attn3(qkv, heads, M=2)
    assert torch.equal(probs, torch.ones_like(probs))
    assert _rel(out, ref) <= 1e-14


@pytest.mark.parametrize("N,C,heads,variant", FC.ATTN_CASES)
def test_attention_adjoint_is_autograd_of_the_forward(N, C, heads, variant):
    qkv, d_out = (t.double() for t in FC.attn_inputs(N, C, heads, variant))
    leaf = qkv.clone().requires_grad_(True)
    probs, out = F3.attn3(leaf, heads)
    (out * d_out).sum().backward()
    hand = F3.attn3_adjoint(qkv, d_out, heads)
    # float64 against float64: rounding of sums of at most 128 terms.  Against the gradient's scale (in the saturated
    # variant the q / k thirds cancel to ~ 1e-100 of their terms; an elementwise ratio there compares two roundings of zero)
    for i, n in enumerate(("d_q", "d_k", "d_v")):
        a, b = hand[:, i * C:(i + 1) * C], leaf.grad[:, i * C:(i + 1) * C]
        c_q, c_k = F3.attn3_grad_condition(qkv, d_out, heads)
        scale = max(float(b.abs().max()), float((c_q if i == 0 else c_k).max()) if i < 2 else 0.0, 1e-300)
        assert float((a - b).abs().max()) <= 1e-12 * scale, (n, float((a - b).abs().max()), scale)
    probs = probs.detach()
    assert tuple(probs.shape) == (N, heads, 3, 2)
    assert float((probs.sum(-1) - 1).abs().max()) <= 1e-15
    if variant == "q0":
        assert torch.equal(probs, torch.full_like(probs, 0.5))
    if variant == "sat":
        assert float(probs.min()) < 1e-45, "the saturated variant must underflow float32 on one side"


def test_probs_are_in_the_abi_partner_order():
    """token 0: 1, 2; token 1: 0, 2; token 2: 0, 1 -- against a dense 3 x 3 masked softmax"""
    N, C, heads = 3, 48, 3
    qkv = FC.attn_inputs(N, C, heads, "plain")[0].double()
    dh = C // heads
    q, k, v = qkv.reshape(N, 3, 3, heads, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * dh ** -0.5 + torch.eye(3).masked_fill(torch.eye(3) == 1, float("-inf"))
    dense = s.softmax(dim=-1)                                                     # [N, heads, 3, 3]
    probs, out = F3.attn3(qkv, heads)
    for i, (a, b) in enumerate(((1, 2), (0, 2), (0, 1))):
        assert _rel(probs[:, :, i, 0], dense[:, :, i, a]) <= 1e-14 and _rel(probs[:, :, i, 1], dense[:, :, i, b]) <= 1e-14
    assert _rel(out, (dense @ v).transpose(1, 2).reshape(3 * N, C)) <= 1e-14


@pytest.mark.parametrize("N,C", FC.ROW_CASES[:3])
@pytest.mark.parametrize("kind", FC.MASK_KINDS)
@pytest.mark.parametrize("with_keep", [False, True])
def test_exchange_and_mean_adjoints_are_autograd_of_the_forwards(N, C, kind, with_keep):
    xs, g, d = FC.row_inputs(N, C)
    mask = FC.exchange_mask(kind, C).double()
    keep = FC.keep_mask(3 * N, C) if with_keep else None
    ds = float(np.float32(1.0 / (1.0 - FC.DROP_P)))
    leaves = [x.double().requires_grad_(True) for x in xs]
    (F3.exchange3(leaves, mask, keep, ds) * g.double()).sum().backward()
    for a, b in zip(F3.exchange3_adjoint(g.double(), mask, keep, ds), leaves):
        assert float((a - b.grad).abs().max()) <= 1e-12 * float(g.abs().max())
    y = g.double().requires_grad_(True)
    (F3.triple_mean(y) * d.double()).sum().backward()
    assert float((F3.triple_mean_adjoint(d.double()) - y.grad).abs().max()) <= 1e-12 * float(d.abs().max())
    if kind == "overlap" and C >= 8:
        k = mask != 0
        assert all(bool((~k[m] & k[m - 1]).any()) for m in range(3)), "own-slot and fed-slot terms must both be live somewhere"
        assert all(bool((k[m] & k[m - 1]).any()) for m in range(3)), "the three index sets must overlap pairwise"


def _ulps(a, b):
    """distance in float32 steps between two non-negative float32 values"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("B,S,H", sorted({c[:3] for c in FC.MODEL_CASES + [FC.BIG_TRAINING_CASE]} | {c[:3] for c in FC.EVAL_STATE_CASES}))
def test_selection_inputs_are_safe(B, S, H):
    """A condition on the INPUTS, from the oracle alone: every modality's k-th and (k + 1)-th smallest validation scores are
    bit-equal (an exact tie, which the tie rule decides) or at least 64 float32 steps apart."""
    xs, _ = FC.model_inputs(B, S, H)
    k = H // 4
    tied = 0
    for m, sc in enumerate(F3.scores([x.double() for x in xs], "val")):
        assert sc.dtype == np.float32 and bool((sc >= 0).all())
        s = np.sort(sc)
        gap = _ulps(s[k - 1], s[k])
        assert gap == 0 or gap >= FC.MIN_SCORE_GAP_ULP, (m, s[k - 1], s[k], gap)
        tied += gap == 0
    if (B, S) == (1, 1):
        assert tied == 2, "at one frame the two post-ReLU streams must drive validation through the tie path"


def test_validation_score_rule():
    """float64 column sums / row count, rounded once to float32 -- not a float32 mean"""
    x = torch.tensor([[1.0, 2.0 ** -30], [1.0, 1.0], [2.0 ** -25, -1.0]], dtype=torch.float64)
    sc = F3.validation_scores(x)
    assert sc.dtype == np.float32
    assert sc[0] == np.float32((2.0 + 2.0 ** -25) / 3.0) and sc[1] == np.float32((2.0 + 2.0 ** -30) / 3.0)
    assert all(bool((s == np.float32(1.0 / (2 * 3 * 8))).all()) for s in F3.scores([torch.zeros(2, 3, 8)] * 3, "train"))
