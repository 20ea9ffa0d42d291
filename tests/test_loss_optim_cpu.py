"""The float64 references of tests/loss_optim_oracle.py against something outside that file, and the loss case table against its
own claims.  No GPU."""
import numpy as np
import pytest
import torch

from tests import loss_cases as LC
from tests import loss_optim_oracle as R

SUBSET = [c["name"] for c in LC.CASES if LC.in_oracle_subset(c)]


def _ref(c, t=None):
    t = t or LC.make(c)
    return R.losses64(t["seg"], t["act"], t["dur"], t["past_label"], t["target"], t["target_dur"], c["pad"], c["exclude"],
                      Kseg=c["Kseg"], val_mode=c["val_mode"], dur_den=c["dur_den"], grad_scale=c["grad_scale"])


# ----------------------------------------------------------------------------------------------------------
# losses64
# ----------------------------------------------------------------------------------------------------------
def test_the_oracle_subset_is_not_empty_and_spans_the_table():
    ks = {LC.BY_NAME[n]["K"] for n in SUBSET}
    assert len(SUBSET) >= 8 and {1, 2, 17, 63, 64, 65, 122, 128} <= ks
    assert any(LC.BY_NAME[n]["dur_den"] is not None for n in SUBSET)


@pytest.mark.parametrize("name", SUBSET)
def test_losses64_equals_the_projects_oracle_where_that_is_defined(name):
    from oracle import futr_oracle as O
    assert O.EXCLUDE_CLASS_IDX == 47
    c = LC.BY_NAME[name]
    t = LC.make(c)
    seg, act, dur = (t[k].double().requires_grad_(True) for k in ("seg", "act", "dur"))
    res = O.losses(dict(seg=seg, action=act, duration=dur), t["past_label"], t["target_dur"].double(), t["target"], c["pad"],
                   dur_den=c["dur_den"])
    res["loss"].backward()
    got = _ref(c, t)
    want = torch.stack([res[k].detach() for k in ("loss_seg", "loss_action", "loss_dur", "loss")])
    assert float((got["loss"] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (got["loss"], want)
    assert got["counts"] == [res[k] for k in ("seg_correct", "seg_total", "act_correct", "act_total")]
    for k, x in (("d_seg", seg), ("d_act", act), ("d_dur", dur)):
        assert float((got[k] - x.grad * c["grad_scale"]).abs().max()) <= 1e-12, k


def test_losses64_modes_against_their_definitions():
    """what the project's oracle does not cover, on one case, from the definitions: val_mode takes the unmasked duration target
    and drops seg, dur_den replaces the mask sum, Kseg ignores labels >= Kseg, grad_scale scales the gradients"""
    c = LC.BY_NAME["k17_clips"]
    t = LC.make(c)
    base = _ref(c, t)
    a = (t["seg"], t["act"], t["dur"], t["past_label"], t["target"], t["target_dur"], c["pad"], c["exclude"])
    mask = (t["target_dur"] != c["pad"]).double()
    od = torch.nn.functional.normalize(torch.exp(t["dur"].double()) * mask, p=1, dim=-1)
    val = R.losses64(None, *a[1:], val_mode=True)
    assert float(val["loss"][0]) == 0.0 and val["counts"][:2] == [0, 0] and val["d_seg"] is None
    want = float(((od - t["target_dur"].double()) ** 2).sum() / mask.sum())
    assert abs(float(val["loss"][2]) - want) <= 1e-12 * want
    assert float(val["loss"][2]) > 100 * float(base["loss"][2])         # the padded targets (pad_idx = 18) are in it
    assert abs(float(val["loss"][1]) - float(base["loss"][1])) <= 1e-15
    dd = R.losses64(*a, dur_den=2.5, grad_scale=0.25)
    assert abs(float(dd["loss"][2]) - float(base["loss"][2]) * float(mask.sum()) / 2.5) <= 1e-12
    assert float((dd["d_seg"] - 0.25 * base["d_seg"]).abs().max()) <= 1e-15
    assert float((dd["d_dur"] - 0.25 * base["d_dur"] * float(mask.sum()) / 2.5).abs().max()) <= 1e-12
    ks = R.losses64(t["seg"][..., :16].contiguous(), *a[1:], Kseg=16)
    lab = t["past_label"].reshape(-1)
    assert int((lab == 16).sum()) > 0                                   # last_max put the label K - 1 there
    assert ks["counts"][1] == base["counts"][1] - int((lab == 16).sum())
    assert float(ks["d_seg"].reshape(-1, 16)[lab == 16].abs().max()) == 0.0


def test_the_case_table_holds_what_its_docstring_lists():
    S, Q, B, K, mod4 = set(), set(), set(), set(), set()
    seen = dict(penalty=0, pad_argmax_ignored=0, w1=0, w10=0, allpad_w1=0, allpad_w10=0, tie_le64=0, tie_gt64=0, tie_wrong=0,
                last_max=0, dead_clip=0, one_live=0, excluded_seg=0, excluded_act=0, oob_seg=0, oob_act=0, kseg_oob=0,
                mid_pad=0, bq_gt64=0, bq_le64=0)
    lasts = set()
    for c in LC.CASES:
        t = LC.make(c)
        r = _ref(c, t)
        i = r["info"]
        S.add(c["S"]); Q.add(c["Q"]); B.add(c["B"]); K.add(c["K"]); mod4.add(LC.units(c) % 4 == 0)
        seen["bq_gt64" if c["B"] * c["Q"] > 64 else "bq_le64"] += 1
        lab, tgt, pad = t["past_label"], t["target"], c["pad"]
        sides = [(t["act"].reshape(-1, c["K"]), tgt.reshape(-1), i["act_argmax"], i["act_valid"])]
        if c["seg"]:
            Ks = c["Kseg"] or c["K"]
            sides.append((t["seg"].reshape(-1, Ks), lab.reshape(-1), i["seg_argmax"], i["seg_valid"]))
            seen["penalty"] += int(i["seg_penalty"].sum())
            seen["pad_argmax_ignored"] += int(((i["seg_argmax"] == pad) & ~i["seg_valid"]).sum())
            seen["excluded_seg"] += int((lab == c["exclude"]).sum()) if 0 <= c["exclude"] < c["K"] else 0
            seen["oob_seg"] += int((lab >= c["K"]).sum() - (lab == pad).sum()) if pad >= c["K"] else int((lab >= c["K"]).sum())
            seen["kseg_oob"] += int((lab == Ks).sum()) if c["Kseg"] else 0
        seen["excluded_act"] += int((tgt == c["exclude"]).sum()) if 0 <= c["exclude"] < c["K"] else 0
        seen["oob_act"] += int((tgt < 0).sum())
        for x, gold, am, valid in sides:
            mx = x.max(1, keepdim=True).values
            tied = ((x == mx).sum(1) > 1) & valid
            C = x.shape[1]
            seen["tie_le64" if C <= 64 else "tie_gt64"] += int(tied.sum())
            seen["tie_wrong"] += int((tied & (am != gold)).sum())
            seen["last_max"] += int(((am == C - 1) & valid & (gold == C - 1)).sum()) if C > 1 else 0
        for b in range(c["B"]):
            nz = (lab[b] != pad).nonzero().flatten()
            w = float(i["weights"][b])
            if nz.numel() == 0:
                seen["allpad_w1" if w == 1.0 else "allpad_w10"] += 1
            else:
                lasts.add((int(nz[-1]), c["S"]))
                seen["mid_pad"] += int(int(nz[-1]) == c["S"] - 1 and nz.numel() < c["S"])
            seen["w1" if w == 1.0 else "w10"] += 1
            live = int((t["target_dur"][b] != pad).sum())
            seen["dead_clip"] += int(live == 0)
            seen["one_live"] += int(live == 1 and c["Q"] > 1)
        assert float((t["target_dur"] != pad).sum()) > 0, c["name"]     # a batch-wide zero mask is no case
    assert {1, 7, 64, 65, 130} <= S and {1, 8, 9, 70} <= Q and {1, 3, 9} <= B
    assert {1, 2, 17, 63, 64, 65, 122, 128, 129} <= K and mod4 == {True, False}
    assert all(v > 0 for v in seen.values()), seen
    last_pos = {p for p, _ in lasts}
    assert {0, 63, 64} <= last_pos and any(p == s - 1 for p, s in lasts)
    assert sum(1 for c in LC.CASES if c["val_mode"] and not c["seg"]) >= 2
    assert any(c["val_mode"] and c["seg"] for c in LC.CASES) and any(c["Kseg"] for c in LC.CASES)
    assert {c["grad_scale"] for c in LC.CASES} == {1.0, 0.25} and {c["layout"] for c in LC.CASES} == {"inter", "sep"}
    assert len(LC.CASES) <= 30


# ----------------------------------------------------------------------------------------------------------
# adamw64
# ----------------------------------------------------------------------------------------------------------
def test_adamw64_equals_torch_adamw_on_float64():
    g = torch.Generator().manual_seed(5)
    n, lr, wd, gs = 1000, 1e-3, 5e-3, 0.5
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    grads = [torch.randn(n, generator=g, dtype=torch.float64) * 1e-2 for _ in range(3)]
    w = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([w], lr=lr, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    p, m, v = p0.numpy().copy(), np.zeros(n), np.zeros(n)
    for step, gr in enumerate(grads, 1):
        w.grad = gr * gs
        opt.step()
        p, m, v = R.adamw64(p, gr.numpy(), m, v, step, lr, wd, grad_scale=gs)
        st = opt.state[w]
        assert np.abs(p - w.detach().numpy()).max() <= 1e-12, step
        assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-12 and np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-12, step
    assert np.abs(p - p0.numpy()).max() > 1e-4                         # (it moved)


# ----------------------------------------------------------------------------------------------------------
# Philox
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    got = R.philox4x32_10(ctr, key)
    assert tuple(int(x[0]) for x in got) == out


def test_philox_mask_layout_and_threshold():
    assert R.philox_thresh(0.1) == 429496736 and R.philox_thresh(0.0) == 0 and R.philox_thresh(0.5) == 1 << 31
    assert R.philox_thresh(0.999) == int(float(np.float32(0.999)) * 2.0 ** 32) < 4294967295
    seed, off = 0x1234567890ABCDEF, (1 << 32) + 3
    w = R.philox_words(9, seed, off)
    assert w.shape == (3, 4)
    one = R.philox4x32_10((2, 0, 3, 1), (0x90ABCDEF, 0x12345678))      # counter (i lo, i hi, off lo, off hi), key (seed lo, hi)
    assert [int(x[0]) for x in one] == w[2].tolist()
    m = R.philox_mask(9, 0.5, seed, off)
    assert m.dtype == np.uint8 and m.tolist() == [int(x >= 1 << 31) for x in w.reshape(-1)[:9]]
    assert R.philox_mask(1000, 0.0, seed, 0).all()
    big = R.philox_mask(1 << 16, 0.1, seed, 0)
    assert abs(float(big.mean()) - 0.9) < 5e-3


def test_finalize64_is_the_sum_it_says():
    B, S, Q = 2, 3, 2
    part = np.zeros((B * (S + Q + 1), 4), dtype=np.float32)
    part[:6, 0], part[:6, 1], part[:6, 2] = 1.5, [1, 0, 1, 0, 0, 1], [1, 1, 1, 0, 1, 1]
    part[6:10, 0], part[6:10, 1], part[6:10, 2] = [1, 2, 3, 4], [0, 1, 0, 0], [1, 1, 0, 1]
    part[10:, 0], part[10:, 2] = [0.5, 0.25], 3.0
    loss, counts = R.finalize64(part, B, S, Q, True, None)
    assert loss.tolist() == [1.5, 2.5, 0.25, 4.25] and counts == [3, 5, 1, 3]
    loss, counts = R.finalize64(part, B, S, Q, False, 1.5)
    assert loss.tolist() == [0.0, 2.5, 0.5, 3.0]
