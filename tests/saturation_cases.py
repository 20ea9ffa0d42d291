"""Inputs, float64 references and bounds of tests/test_saturation_cpu.py and tests/test_saturation_gpu.py: the softmax, row
cross-entropy, contrastive and LSTM gate kernels where their inputs SATURATE.  The other case tables draw operands from randn
or U(-1, 1), so every exp argument stays of order one; here the softmax is sharp, whole tiles or chunks underflow, the
running maximum moves by several units per tile, s - lse cancels, and gates sit on their rails.

A. attention cores (csrc/attention.hip both paths with mha_small.h, attention_tiled.hip, attention_splitk.hip,
   attention_xclip.hip).  A score profile edits q and k BEFORE the reference sees them, so the reference and the kernel get
   the same float32 operands:
     sharp        q and k each scaled by sqrt(30): score std about 30
     stair_up/dn  feature 0 of every head: q0 = sqrt(dh), k0(j) = +-STAIR (j // 64): every 64-key tile moves the maximum by 4
     cliff_up/dn  the same with a gap of CLIFF per tile (per chunk for the split-key core): a whole tile or chunk underflows to 0
     shift        q0 = 4, k0 = 4 sqrt(dh) on every key: +16 on every score; `flat` is the same problem with k0 = 0
   A stair or cliff needs two tiles, so the one-tile rows of the small path run sharp and shift only; the cliffs run at
   dh = 16 only (at dh = 128 float32 PyTorch itself misses the condition below).
B. row cross-entropies (ce_row of losses_dev.h through r3d_losses_fwd_bwd / _kseg on both sides of its K <= 64 split,
   r3d_ce_rows_fwd_bwd, r3d_focal_rows) under the logit profiles sharp (x 30), shift (+100 on a row), confident_right (label
   logit = row max + 50) and confident_wrong (label logit = row min - 50).  The rows a table edited for ties or arg-maxima
   are left alone by the two confident profiles.  Out of scope: the duration term (exp(dur) overflows in the reference
   too; it stays at unit scale in every case here), and the launches that compute their own logits from activations
   (decoder_tail_losses, decoder_chain, cnn_seg_step, afft_head_step): saturating them means scaling weights, which moves
   every other tensor's conditioning.
C. the supervised contrastive loss at T = Tb = 0.01 on unit rows: scores reach +-100.
D. the LSTM recurrences (csrc/lstm.hip, csrc/lstm_steps.hip) with gates on their rails through the recurrent bias b_hh,
   which the kernels read directly: per direction the units are split into four quarters, +RAIL on the forget gate of
   quarter 0, -RAIL on the input gate of quarter 1, +RAIL on the output gate and +RAIL_G on the cell candidate of quarter 2.

Bounds.  None is new.  A: 1e-4 of max|ref| for o / probs / lse / delta and 1e-3 for the gradients (tests/test_engine_gpu.
close_rel, as the tiled and split-key tests); B: tests/loss_cases.py's margins (losses rtol 1e-4 / atol 1e-6, gradients 1e-3
of scale, counters exact); C: tests/test_supcon_gpu.py's (1e-4 loss and lse, 1e-3 gradient); D: tests/rnn_wide_cases.py's
rule max(8 e32, 2e-6 max|ref|) with its CAP.  What keeps A-C honest is a condition tests/test_saturation_cpu.py asserts
of every case and tensor: with e32 = max|f32 - f64| of the SAME restatement run in float32 on the same operands,
8 e32 <= bound (8 is the project's margin for another summation order).  The references of the existing suites cast to
float64 on entry, so the restatements here take a dtype; the CPU test ties each of them, at float64, to the reference it
restates.  A case that missed the condition was made milder, never its bound wider; the values in use:

  SHIFT   16    (+64 misses the condition: o 1.2e-5 .. 2.4e-5 of scale in float32)
  SHARP   30; 20 (SHARP_MILD) on the (8, 64, 128, 1) row, whose o misses the condition at 30 (8 e32 = 1.1 x the bound)
  CLIFF   112, centred: k0(j) = +-CLIFF (j // step - (levels - 1) / 2).  A gap of 100 leaves float32 exp(m_tile - m_row) a
                denormal (e^-100 = 3.8e-44; a partial last tile's maximum lies lower still), not the exact 0 the profile is
                named for: 112 underflows in every row of every case.  Uncentred, scores of 110 and 220 miss the
                condition (delta 1.5 x, o 0.94 x the bound); centred, the same gap keeps |score| near 56 and meets it
  cliffs  dh = 16 only (at dh = 128 float32 PyTorch itself misses the condition)
  the general-path row (70, 70, 25, 4) runs at Lq = 40: r3d_mha_core_supported refuses Lq dh > 1024, and 40 is the most
  queries the core takes at dh = 25; Lk = 70 keeps its two key chunks

A gradient whose exact value is 0 -- dq and dk where one key holds all the weight (a single valid key; the one key of a last
chunk above a cliff) -- comes out of a kernel as the rounding of dP - delta, two float32 sums that cancel, times k or q.
tests/test_attention_splitk_gpu.py holds such a tensor to the gradients' joint scale (dq | dk | dv as one tensor, 1e-3)
alone; here that rule applies to a gradient whose reference scale is below one float32 epsilon of the joint scale, and the
joint tensor is held in every case.
  RAIL    20, RAIL_G 12 (no case needed a lower rail)
"""
import functools
import math

import torch
import torch.nn.functional as F

PAD, B = 99, 3
MARGIN = 8.0
SHIFT_Q0, SHIFT = 4.0, 16.0
STAIR, CLIFF = 4.0, 112.0
SHARP, SHARP_MILD = 30.0, 20.0
TT = 64                                  # keys per tile of every core


def rel_bound(name):
    """1e-3 of max|ref| for a gradient (dq, dk, dv, d_qkv, d), 1e-4 for everything else; "x vs unshifted" is x's"""
    name = name.split()[0]
    return 1e-3 if name.startswith("d") and name != "delta" else 1e-4


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


# ---------------------------------------------------------------------------------------------------------------------
# A. attention
# ---------------------------------------------------------------------------------------------------------------------
# (core, Lq, Lk, dh, heads, masked): masked = dropout on and the "three" key mask of the tiled test
ATT_ROWS = [
    ("core", 8, 21, 16, 8, True),            # small path (Lq = 8, Lk <= 64, 16-byte aligned rows)
    ("core", 8, 64, 128, 1, False),          # small path; sharp at SHARP_MILD
    ("core", 8, 130, 16, 8, False),          # general path, three 64-key chunks
    ("core", 40, 70, 25, 4, True),           # general path; the issue's Lq = 70 is refused (the core takes Lq dh <= 1024)
    ("tiled", 70, 70, 16, 8, False),
    ("tiled", 8, 130, 25, 8, True),
    ("tiled", 16, 130, 128, 1, True),
    ("splitk", 8, "C+1", 16, 8, True),
    ("splitk", 16, "2C+1", 16, 8, False),
    ("splitk", 8, "C+1", 128, 1, False),
]


def att_profiles(i, row, Lk):
    """the profiles of row i"""
    dh = row[3]
    if Lk <= TT:
        return ["sharp", "shift"]
    out = ["sharp", "stair_up" if i % 2 == 0 else "stair_down", "shift"]
    return out + ["cliff_up", "cliff_down"] if dh == 16 else out


def att_step(core, profile, C):
    """keys per step of a stair / cliff: a 64-key tile, the split-key core's cliffs its chunk"""
    return C if core == "splitk" and profile.startswith("cliff") else TT


def att_cases(chunk_of):
    """[(id, row index, Lk, C, profile)]; chunk_of(Lk, dh) is ops.mha_splitk_chunk"""
    from tests import splitk_cases as SK
    out = []
    for i, row in enumerate(ATT_ROWS):
        core, Lq, lk, dh, heads, masked = row
        Lk = SK.resolve(lk, dh, chunk_of)
        C = chunk_of(Lk, dh) if core == "splitk" else 0
        for p in att_profiles(i, row, Lk):
            out.append((f"{core}-Lq{Lq}-Lk{lk}-dh{dh}x{heads}-{'drop' if masked else 'plain'}-{p}", i, Lk, C, p))
    return out


MILD_ROWS = (1,)                         # rows whose sharp profile missed 8 e32 <= bound at SHARP (o: 1.1 x the bound)


def apply_profile(profile, q, k, heads, dh, step, sharp=SHARP):
    """q [B*Lq, H], k [B*Lk, H] float32 -> edited float32 copies"""
    q, k = q.clone(), k.clone()
    if profile == "sharp":
        s = torch.tensor(math.sqrt(sharp), dtype=torch.float32)
        return q * s, k * s
    Lk = k.shape[0] // B
    q0, k0 = q.view(-1, heads, dh)[:, :, 0], k.view(B, Lk, heads, dh)[..., 0]
    if profile in ("shift", "flat"):
        q0.fill_(SHIFT_Q0)
        k0.fill_(SHIFT / SHIFT_Q0 * math.sqrt(dh) if profile == "shift" else 0.0)
        return q, k
    kind, way = profile.split("_")
    height = {"stair": STAIR, "cliff": CLIFF}[kind] * (1.0 if way == "up" else -1.0)
    level = (torch.arange(Lk) // step).float()
    if kind == "cliff":                          # centred: the gap between tiles is CLIFF, the scores stay within CLIFF / 2 of 0
        level = level - (float(level.max()) / 2)
    q0.fill_(math.sqrt(dh))
    k0.copy_((height * level)[None, :, None].expand(B, Lk, heads))
    return q, k


def attention(q, k, v, d_o, lab, keep, dsc, heads, dh, Lq, Lk, dtype=torch.float64):
    """tests/test_tiled_attention_gpu.reference with every operation in `dtype` (at float64 the same values, which
    tests/test_saturation_cpu.py asserts), plus the probabilities before dropout and delta = rowsum(dO o O)."""
    H = heads * dh
    qr, kr, vr = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    qh = qr.reshape(B, Lq, heads, dh).transpose(1, 2)
    kh = kr.reshape(B, Lk, heads, dh).transpose(1, 2)
    vh = vr.reshape(B, Lk, heads, dh).transpose(1, 2)
    s = ((qh @ kh.transpose(-2, -1)) / math.sqrt(dh)).masked_fill((lab == PAD)[:, None, None, :], float("-inf"))
    att = s.softmax(-1)
    attd = att if keep is None else att * keep.to(dtype) * dsc
    o = (attd @ vh).transpose(1, 2).reshape(B * Lq, H)
    o.backward(d_o.to(dtype))
    od = o.detach()
    delta = (od * d_o.to(dtype)).reshape(B, Lq, heads, dh).sum(-1).transpose(1, 2)
    return dict(o=od, probs=att.detach(), lse=torch.logsumexp(s, -1).detach(), delta=delta, dq=qr.grad, dk=kr.grad, dv=vr.grad)


ATT_TENSORS = ("o", "probs", "lse", "delta", "dq", "dk", "dv")
EPS32 = 2.0 ** -23


def joint(r):
    """dq | dk | dv of a result as one flat float64 tensor"""
    return torch.cat([r[n].detach().double().cpu().reshape(-1) for n in ("dq", "dk", "dv")])


def negligible(ref, name):
    """a gradient whose reference is 0 at float32's resolution of the gradients' joint scale: held to the joint scale alone"""
    return name.split()[0] in ("dq", "dk", "dv") and float(ref[name.split()[0]].abs().max()) < EPS32 * float(joint(ref).abs().max())


def att_labels(core, Lk, C, masked, profile):
    from tests import splitk_cases as SK
    from tests.test_tiled_attention_gpu import labels as three
    if core == "splitk" and profile == "cliff_down" and Lk > 2 * C:
        return SK.labels(Lk, "first", C)         # the wholly masked first chunk (m = -inf) beside chunks that underflow
    return three(Lk) if masked else torch.zeros(B, Lk, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def att_problem(i, Lk, C, profile):
    """Host inputs and float64 reference of row i under a profile, computed once and left unchanged:
    dict(q, kv, d_o, lab, keep, dsc, ref, ref32[, flat, flat32][, cut])."""
    from tests.test_tiled_attention_gpu import keep_mask
    core, Lq, _, dh, heads, masked = ATT_ROWS[i]
    H = heads * dh
    q, kv, d_o = rnd(B * Lq, H, seed=900 + 7 * i), rnd(B * Lk, 2 * H, seed=901 + 7 * i), rnd(B * Lq, H, seed=902 + 7 * i)
    step = att_step(core, profile, C)
    q, k = apply_profile(profile, q, kv[:, :H], heads, dh, step, sharp=SHARP_MILD if i in MILD_ROWS else SHARP)
    kv = torch.cat([k, kv[:, H:]], 1).contiguous()
    lab = att_labels(core, Lk, C, masked, profile)
    keep, dsc = keep_mask(heads, Lq, Lk, masked)
    a = (kv[:, H:], d_o, lab, keep, dsc, heads, dh, Lq, Lk)
    out = dict(q=q, kv=kv, d_o=d_o, lab=lab, keep=keep, dsc=dsc, step=step,
               ref=attention(q, k, *a), ref32=attention(q, k, *a, dtype=torch.float32))
    if profile == "shift":                      # the unshifted problem: k0 = 0
        qf, kf = apply_profile("flat", q, k, heads, dh, step)
        assert torch.equal(qf, q)
        out["flat"] = attention(qf, kf, *a)
    if profile == "cliff_down" and not masked:
        # the attention over the first tile or chunk that is not wholly masked, alone: what the later ones add is exactly 0
        n = step * (2 if bool((lab[:, :step] == PAD).all()) else 1)
        cut = lambda t: t.reshape(B, Lk, -1)[:, :n].reshape(B * n, -1)        # noqa: E731
        o_cut = attention(q, cut(k), cut(kv[:, H:]), d_o, lab[:, :n], None, 1.0, heads, dh, Lq, n)["o"].reshape(B, Lq, H)
        dead = (lab[:, :n] == PAD).all(1)         # a clip whose only valid keys lie later (the "first" mask's clip 2): as it is
        o_cut[dead] = out["ref"]["o"].reshape(B, Lq, H)[dead]
        assert int(dead.sum()) <= 1
        out["cut"] = o_cut.reshape(B * Lq, H)
    return out


def att_pairs(p):
    """[(tensor, float32 restatement, float64 reference)]: every tensor against its own problem, and the shifted problem's
    against the unshifted reference (lse moved back by the shift, probs and the rest as they are)."""
    out = [(n, p["ref32"][n], p["ref"][n]) for n in ATT_TENSORS]
    if "flat" in p:
        out += [(n + " vs unshifted", p["ref32"][n] - (SHIFT if n == "lse" else 0.0), p["flat"][n]) for n in ATT_TENSORS]
    return out


def scores(p, i, Lk):
    """unmasked float64 scores [B, heads, Lq, Lk] of a problem's float32 operands"""
    _, Lq, _, dh, heads, _ = ATT_ROWS[i]
    H = heads * dh
    qh = p["q"].double().reshape(B, Lq, heads, dh).transpose(1, 2)
    kh = p["kv"][:, :H].double().reshape(B, Lk, heads, dh).transpose(1, 2)
    return (qh @ kh.transpose(-2, -1)) / math.sqrt(dh)


# cross-clip attention: two cases of tests/l3_cases.XCLIP (dh 16 over 13 clips; dh 128 over 2), sharp and shift only
XCLIP_NAMES = ["B13_S5_H128_h8", "B2_S5_H1024_h8"]


@functools.lru_cache(maxsize=None)
def xclip_problem(name, profile):
    """dict(case, qkv, d_o: float32; ref, ref32[, flat]: dict(o, d_qkv)) by tests/l3_oracle.py"""
    from tests import l3_cases as LC, l3_oracle as LO
    case = LC.XCLIP_BY_NAME[name]
    qkv, d_o = LC.xclip_inputs(case)
    Bc, S, H, heads = case["B"], case["S"], case["H"], case["heads"]
    dh = H // heads

    def edit(profile):
        x = qkv.clone()
        parts = x.view(Bc, S, 3, heads, dh)
        if profile == "sharp":
            parts[:, :, :2] *= torch.tensor(math.sqrt(SHARP), dtype=torch.float32)
        else:
            parts[:, :, 0, :, 0] = SHIFT_Q0
            parts[:, :, 1, :, 0] = SHIFT / SHIFT_Q0 * math.sqrt(dh) if profile == "shift" else 0.0
        return x
    run = lambda x, dt: dict(o=LO.xclip_fwd(x, heads, dt), d_qkv=LO.xclip_bwd(x, d_o, heads, dt))      # noqa: E731
    x = edit(profile)
    out = dict(case=case, qkv=x, d_o=d_o, ref=run(x, torch.float64), ref32=run(x, torch.float32))
    if profile == "shift":
        out["flat"] = run(edit("flat"), torch.float64)
    out["probs"] = LO.xclip_probs(x.double(), heads)
    return out


def xclip_pairs(p):
    out = [(n, p["ref32"][n], p["ref"][n]) for n in ("o", "d_qkv")]
    if "flat" in p:
        out += [(n + " vs unshifted", p["ref32"][n], p["flat"][n]) for n in ("o", "d_qkv")]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# B. row cross-entropies
# ---------------------------------------------------------------------------------------------------------------------
LOGIT_PROFILES = ("sharp", "shift", "confident_right", "confident_wrong")
LOGIT_SHIFT, CONFIDENT = 100.0, 50.0


def apply_logit_profile(profile, x, gold, live, skip):
    """x [rows, C] float32 (a copy is edited), gold [rows]; live: rows whose label counts; skip: rows left alone by the
    confident profiles (the ties and arg-max rows a table built)."""
    x = x.clone()
    if profile == "sharp":
        return x * SHARP
    if profile == "shift":
        return x + LOGIT_SHIFT
    for r in range(x.shape[0]):
        if bool(live[r]) and not bool(skip[r]):
            x[r, int(gold[r])] = x[r].max() + CONFIDENT if profile == "confident_right" else x[r].min() - CONFIDENT
    return x


def ce_rows(pred, gold, valid, dtype):
    """(per-row CE [rows], softmax - one-hot [rows, C]) in `dtype`, zero on the rows that are not valid"""
    x = pred.to(dtype)
    g = torch.where(valid, gold, torch.zeros_like(gold))
    lse = torch.logsumexp(x, dim=1)
    ce = torch.where(valid, lse - x.gather(1, g[:, None])[:, 0], torch.zeros_like(lse))
    d = torch.exp(x - lse[:, None]) - F.one_hot(g, x.shape[1]).to(dtype)
    return ce, d * valid[:, None].to(dtype)


# the loss launches: cases of tests/loss_cases.py with K in {17, 64, 65, 122}, and the `_kseg` entry point on both sides of
# ce_row's K <= 64 split
LOSS_CASES = ["k17_clips", "k64_ties_pad_inside", "k65_ties", "k122_ties", "kseg_k17", "kseg_k65"]


@functools.lru_cache(maxsize=None)
def loss_problem(name, profile):
    """dict(c, t (the case's tensors, its logits under the profile), ref (loss_optim_oracle.losses64), r64, r32 (the CE terms
    restated in float64 / float32: dict(loss_seg, loss_act, d_seg, d_act))[, flat: losses64 of the unshifted case])"""
    from tests import loss_cases as LC, loss_optim_oracle as R
    c = LC.BY_NAME[name]
    t = LC.make(c)
    plain = LC.make(dict(c, ties=(), seg_ties=None, act_ties=None, last_max=False, pad_argmax=False))
    Bc, S, Q, K = c["B"], c["S"], c["Q"], c["K"]
    Ks = c["Kseg"] or K
    t0 = dict(t)

    def edit(key, C, gold, gold_plain):
        x, x0 = t[key].reshape(-1, C), plain[key].reshape(-1, C)
        skip = (x != x0).any(1) | (gold != gold_plain)
        live = (gold != c["pad"]) & (gold != c["exclude"]) & (gold >= 0) & (gold < C)
        return apply_logit_profile(profile, x, gold, live, skip).view(t[key].shape)
    t = dict(t, seg=edit("seg", Ks, t["past_label"].reshape(-1), plain["past_label"].reshape(-1)),
             act=edit("act", K, t["target"].reshape(-1), plain["target"].reshape(-1)))
    run = lambda tt: R.losses64(tt["seg"], tt["act"], tt["dur"], tt["past_label"], tt["target"], tt["target_dur"],   # noqa: E731
                                c["pad"], c["exclude"], Kseg=c["Kseg"], val_mode=c["val_mode"], dur_den=c["dur_den"],
                                grad_scale=c["grad_scale"])
    ref = run(t)
    info = ref["info"]

    def restate(dtype):
        ce_s, d_s = ce_rows(t["seg"].reshape(-1, Ks), t["past_label"].reshape(-1), info["seg_valid"], dtype)
        ce_a, d_a = ce_rows(t["act"].reshape(-1, K), t["target"].reshape(-1), info["act_valid"], dtype)
        w = info["weights"].to(dtype).repeat_interleave(Q)
        return dict(loss_seg=(ce_s + 2.0 * info["seg_penalty"].to(dtype)).mean(), loss_act=(ce_a * w).mean(),
                    d_seg=d_s / (Bc * S) * c["grad_scale"], d_act=d_a * w[:, None] / (Bc * Q) * c["grad_scale"])
    out = dict(c=c, t=t, ref=ref, r64=restate(torch.float64), r32=restate(torch.float32))
    if profile == "shift":
        out["flat"] = run(t0)
    return out


def loss_pairs(p):
    """[(name, f32, f64, kind)], kind "loss" (rtol 1e-4 / atol 1e-6) or "grad" (1e-3 of scale)"""
    c, ref = p["c"], p["ref"]
    N, BQ = c["B"] * c["S"], c["B"] * c["Q"]
    want = dict(loss_seg=ref["loss"][0], loss_act=ref["loss"][1], d_seg=ref["d_seg"].reshape(N, -1), d_act=ref["d_act"].reshape(BQ, -1))
    out = [(n, p["r32"][n], want[n], "loss" if n.startswith("loss") else "grad") for n in want]
    if "flat" in p:
        f = p["flat"]
        flat = dict(loss_seg=f["loss"][0], loss_act=f["loss"][1], d_seg=f["d_seg"].reshape(N, -1), d_act=f["d_act"].reshape(BQ, -1))
        out += [(n + " vs unshifted", p["r32"][n], flat[n], "loss" if n.startswith("loss") else "grad") for n in flat]
    return out


# r3d_ce_rows_fwd_bwd: (rows, C, pad); every third target is the pad
CE_ROWS = [(24, 17, 16), (40, 64, 70), (40, 65, 3), (32, 122, 123)]


@functools.lru_cache(maxsize=None)
def ce_problem(rows, C, pad, profile):
    """dict(x, tgt, ref, ref32: dict(loss, d, counts)[, flat]) by tests/tcn_oracle.loss_counts"""
    from tests import tcn_oracle as TO
    x0 = 3.0 * rnd(rows, C, seed=rows + C)
    g = torch.Generator().manual_seed(rows)
    tgt = torch.randint(0, C, (rows,), generator=g)
    tgt[::3] = pad
    live = tgt != pad
    x = apply_logit_profile(profile, x0, tgt, live, torch.zeros(rows, dtype=torch.bool))

    def run(x, dtype):
        q = x.detach().to(dtype).clone().requires_grad_(True)
        loss, nc, nt = TO.loss_counts(q, tgt, pad)
        loss.backward()
        return dict(loss=loss.detach(), d=q.grad, counts=[nc, nt])
    out = dict(x=x, tgt=tgt, ref=run(x, torch.float64), ref32=run(x, torch.float32))
    if profile == "shift":
        out["flat"] = run(x0, torch.float64)
    return out


def ce_pairs(p):
    out = [("loss", p["ref32"]["loss"], p["ref"]["loss"], "loss"), ("d", p["ref32"]["d"], p["ref"]["d"], "grad")]
    if "flat" in p:
        out += [("loss vs unshifted", p["ref32"]["loss"], p["flat"]["loss"], "loss"), ("d vs unshifted", p["ref32"]["d"], p["flat"]["d"], "grad")]
    return out


# r3d_focal_rows: cases in the form of tests/temporal_cases.FOCAL (its make() builds them), gamma in {1, 2} x alpha in {1, 0.25}
def _focal(N, C, exclude, alpha, gamma, penalty, oob):
    return dict(name=f"sat_f_n{N}_c{C}", kind="focal", N=N, C=C, pad=C - 1, exclude=exclude, alpha=alpha, gamma=gamma,
                penalty=penalty, argmax_pad=True, oob=oob)


FOCAL = [_focal(24, 17, None, 1.0, 1.0, 0.0, None), _focal(40, 64, 0, 1.0, 2.0, 2.0, None), _focal(40, 65, None, 0.25, 1.0, 2.0, 70),
         _focal(32, 122, 3, 0.25, 2.0, 0.0, -2)]
FOCAL_BY_NAME = {c["name"]: c for c in FOCAL}


def focal(pred, gold, pad, exclude, alpha, gamma, penalty, dtype=torch.float64):
    """tests/temporal_oracle.focal with every operation in `dtype` (at float64 the same values): (loss, flags, correct, live)"""
    pred = pred.to(dtype)
    N, C = pred.shape
    live = (gold != pad) & (gold >= 0) & (gold < C)
    if exclude is not None:
        live &= gold != exclude
    logp = F.log_softmax(pred, dim=1)
    ce = -logp[torch.arange(N), gold.clamp(0, C - 1)]
    arg = pred.argmax(1)
    row = alpha * (1.0 - torch.exp(-ce)) ** gamma * ce + penalty * (arg == pad).to(dtype)
    loss = (row * live).sum() / N
    flags = live & (arg == gold)
    return loss, flags, int(flags.sum()), int(live.sum())


@functools.lru_cache(maxsize=None)
def focal_problem(name, profile):
    """dict(case, pred, gold, ref, ref32: dict(loss, d, flags, counts)[, flat])"""
    from tests import temporal_cases as TC
    case = FOCAL_BY_NAME[name]
    pred0, gold = TC.make(case)
    C = case["C"]
    live = (gold != case["pad"]) & (gold >= 0) & (gold < C)
    if case["exclude"] is not None:
        live &= gold != case["exclude"]
    skip = pred0.argmax(1) == case["pad"]                       # the arg-max row make() built
    pred = apply_logit_profile(profile, pred0, gold, live, skip)

    def run(x, dtype):
        q = x.detach().to(dtype).clone().requires_grad_(True)
        loss, flags, nc, nl = focal(q, gold, case["pad"], case["exclude"], case["alpha"], case["gamma"], case["penalty"], dtype)
        loss.backward()
        return dict(loss=loss.detach(), d=q.grad, flags=flags, counts=[nc, nl])
    out = dict(case=case, pred=pred, gold=gold, live=live, skip=skip, ref=run(pred, torch.float64), ref32=run(pred, torch.float32))
    if profile == "shift":
        out["flat"] = run(pred0, torch.float64)
    return out


def loss_bound(want, kind):
    """the element-wise (loss) or whole-tensor (grad) bound of tests/loss_cases.py's margins on a float64 reference"""
    want = torch.as_tensor(want).double()
    return 1e-4 * want.abs() + 1e-6 if kind == "loss" else torch.full_like(want, 1e-3 * max(float(want.abs().max()), 1e-5))


# ---------------------------------------------------------------------------------------------------------------------
# C. supervised contrastive loss at T = Tb = 0.01
# ---------------------------------------------------------------------------------------------------------------------
def _supcon_cases():
    from tests import supcon_cases as SC
    return [SC._case("sat_n65_d16", 65, 16, T=0.01, Tb=0.01), SC._case("sat_n130_d128", 130, 128, T=0.01, Tb=0.01),
            SC._case("sat_n65_d20_v2_ign", 65, 20, V=2, mode="all", T=0.01, Tb=0.01, ignore="scattered")]


SUPCON_NAMES = ["sat_n65_d16", "sat_n130_d128", "sat_n65_d20_v2_ign"]


def supcon(x, y, *, A, temperature, base_temperature, ignore_index, normalize, dtype=torch.float64):
    """tests/supcon_oracle.supcon with every operation in `dtype` (at float64 the same values): (loss, lse, P)"""
    assert not normalize
    z = x.to(dtype)
    N = z.shape[0]
    kept = torch.ones(N, dtype=torch.bool) if ignore_index is None else (y != ignore_index)
    s = (z[:A] @ z.t()) / temperature
    in_c = kept[None, :].expand(A, N) & ~torch.eye(N, dtype=torch.bool)[:A]
    pos = in_c & (y[:A, None] == y[None, :])
    P = pos.sum(1)
    lse = torch.logsumexp(s.masked_fill(~in_c, float("-inf")), dim=1)
    live = kept[:A] & (P > 0)
    pos_sum = (s * pos).sum(1)
    per_row = torch.zeros(A, dtype=dtype)
    if bool(live.any()):
        idx = live.nonzero().flatten()
        per_row = per_row.index_put((idx,), -(temperature / base_temperature) * (pos_sum[idx] / P[idx] - lse[idx]))
    return per_row.sum() / max(1, int(kept[:A].sum())), lse.detach(), P


@functools.lru_cache(maxsize=None)
def supcon_problem(name):
    """dict(case, x [bsz, V, D], y, z (the contrast rows), yo, kw, ref, ref32: dict(loss, d, lse, P))"""
    from tests import supcon_cases as SC, supcon_oracle as SO
    case = {c["name"]: c for c in _supcon_cases()}[name]
    x, y = SC.make(case)
    if name == "sat_n65_d16":
        x[1], y[1] = x[0], y[0]                                 # cos = 1 with the same label: a positive at score exactly 1 / T
        other = int((y != y[2]).nonzero()[-1])
        assert other > 2
        x[other] = x[2]                                         # and a contrast of another label at the maximum
    z, yo, kw = SO.contrast_rows(x), SC.oracle_labels(case, y), SC.oracle_kwargs(case)

    def run(dtype):
        q = z.detach().to(dtype).clone().requires_grad_(True)
        loss, lse, P = supcon(q, yo, dtype=dtype, **kw)
        loss.backward()
        return dict(loss=loss.detach(), d=q.grad, lse=lse, P=P)
    return dict(case=case, x=x, y=y, z=z, yo=yo, kw=kw, ref=run(torch.float64), ref32=run(torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# D. LSTM gates on their rails
# ---------------------------------------------------------------------------------------------------------------------
RAIL, RAIL_G = 20.0, 12.0
# (route, B, S, H)
LSTM_CASES = [("registers", 8, 16, 128), ("registers", 13, 37, 136), ("steps", 1, 2, 264), ("steps", 5, 3, 520),
              ("steps", 8, 16, 512), ("steps", 8, 16, 128)]


def quarters(h):
    """the unit ranges of the four quarters of a direction"""
    e = [h * i // 4 for i in range(5)]
    return [slice(e[i], e[i + 1]) for i in range(4)]


def lstm_inputs(Bc, S, H):
    """tests/rnn_wide_cases.inputs with the rails added to b_hh (gate order i, f, g, o; rounded to float32, as every input)"""
    from tests import rnn_wide_cases as WC
    w, x, dy = WC.inputs(Bc, S, H)
    h = H // 2
    q = quarters(h)
    w = dict(w)
    for d in (0, 1):
        b = w[("b_hh", d)].clone().view(4, h)
        b[1, q[0]] += RAIL
        b[0, q[1]] -= RAIL
        b[3, q[2]] += RAIL
        b[2, q[2]] += RAIL_G
        w[("b_hh", d)] = b.reshape(-1).float().double()
    return w, x, dy


@functools.lru_cache(maxsize=None)
def lstm_reference(Bc, S, H):
    """(ref, bounds) as tests/rnn_wide_cases.reference, on the railed inputs"""
    from tests import rnn_oracle as RO, rnn_wide_cases as WC
    w, x, dy = lstm_inputs(Bc, S, H)
    ref = WC.by_tensor(RO.lstm_layer_grads(x, w, dy), Bc * S, H)
    f32 = WC.by_tensor(RO.lstm_layer_grads(x.float(), {k: v.float() for k, v in w.items()}, dy.float()), Bc * S, H)
    bounds = {}
    for k in WC.TENSORS:
        assert f32[k].dtype == torch.float32 and ref[k].dtype == torch.float64
        e32 = float((f32[k].double() - ref[k]).abs().max())
        scale = float(ref[k].abs().max())
        bounds[k] = (max(WC.MARGIN * e32, WC.FLOOR * scale), e32, scale)
    return ref, bounds, f32


def lstm_check(got, Bc, S, H, what):
    """tests/rnn_wide_cases.check against lstm_reference: prints each figure, then asserts the bounds"""
    from tests import rnn_wide_cases as WC
    ref, bounds, _ = lstm_reference(Bc, S, H)
    bad = []
    for k in WC.TENSORS:
        g = got[k].detach().cpu().double()
        assert g.shape == ref[k].shape, (k, g.shape, ref[k].shape)
        bound, e32, scale = bounds[k]
        finite = bool(torch.isfinite(g).all())
        err = float((g - ref[k]).abs().max()) if finite else float("inf")
        print(f"[saturation] lstm {what} B{Bc} S{S} H{H} {k}: err {err:.3e} scale {scale:.3e} bound {bound:.3e} e32 {e32:.3e}")
        if scale == 0.0:
            if not (finite and bool((g == 0).all())):
                bad.append((k, err, "reference is identically zero"))
        elif not err <= bound:
            bad.append((k, err, bound))
    assert not bad, (what, Bc, S, H, bad)
