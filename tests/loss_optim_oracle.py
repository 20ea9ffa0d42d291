"""Float64 references of what losses.hip and optim.hip compute (tests/test_loss_optim_cpu.py ties each of them to something
outside this file: oracle.futr_oracle.losses, torch.optim.AdamW, the published Philox known-answer vectors).

losses64      the reference's loss block (utils.py cal_loss / cal_weighted_loss / cal_performance / normalize_duration as
              composed by train_proposed_depth.py's train() and validate()), with autograd for the gradients
adamw64       torch.optim.AdamW, single tensor, one step
philox_mask   the keep-mask r3d_dropout_mask documents: Philox4x32-10, counter (i, offset), key (seed)
finalize64    the sum r3d_losses_finalize takes over the per-unit partials a loss launch leaves behind"""
import numpy as np
import torch
import torch.nn.functional as F


# ----------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------
def first_argmax(x):
    """index of the FIRST maximum of each row (numpy.argmax documents that rule)"""
    return torch.from_numpy(np.argmax(x.detach().numpy(), axis=1).astype(np.int64))


def _masked_ce(pred, gold, pad_idx, exclude_idx):
    """per-row CE; rows whose label is the pad, the excluded class or outside [0, classes) are ignored"""
    C = pred.shape[1]
    valid = (gold != pad_idx) & (gold != exclude_idx) & (gold >= 0) & (gold < C)
    g = gold.clone()
    g[~valid] = -1
    return F.cross_entropy(pred, g, ignore_index=-1, reduction="none"), valid


def losses64(seg, act, dur, past_label, target, target_dur, pad_idx, exclude_idx, Kseg=None, val_mode=False, dur_den=None,
             grad_scale=1.0):
    """seg [B, S, Kseg or K] or None, act [B, Q, K], dur [B, Q], past_label [B, S] int64, target [B, Q] int64, target_dur
    [B, Q] (pad_idx where padded).  Every floating input is taken to float64 first.  Returns a dict:
    loss [4] float64 (seg, action, duration, total), counts [4] ints, d_seg / d_act / d_dur = d total * grad_scale, and
    info: per-clip weights, the rows that drew the penalty, the row arg-maxima."""
    B, Q, K = act.shape
    S = past_label.shape[1]
    act64 = act.detach().double().requires_grad_(True)
    dur64 = dur.detach().double().requires_grad_(True)
    td = target_dur.detach().double()
    info = {}
    zero = torch.zeros((), dtype=torch.float64)
    l_seg, seg64, n_seg_ok, n_seg = zero, None, 0, 0
    if seg is not None:
        Ks = seg.shape[-1]
        assert Ks == (K if Kseg is None else Kseg)
        seg64 = seg.detach().double().requires_grad_(True)
        pred, gold = seg64.reshape(B * S, Ks), past_label.reshape(-1)
        base, valid = _masked_ce(pred, gold, pad_idx, exclude_idx)
        am = first_argmax(pred)
        pen = (am == pad_idx) & valid
        l_seg = (base + 2.0 * pen.double()).mean()
        n_seg_ok, n_seg = int(((am == gold) & valid).sum()), int(valid.sum())
        info.update(seg_argmax=am, seg_valid=valid, seg_penalty=pen)
    # anticipation: weight 1 when the last observed label equals the first future label, else 10
    ref = torch.full((B,), pad_idx, dtype=torch.int64)
    for b in range(B):
        nz = (past_label[b] != pad_idx).nonzero().flatten()
        if nz.numel() > 0:
            ref[b] = past_label[b, nz[-1]]
    w = torch.where(ref == target[:, 0], 1.0, 10.0).double()
    pred, gold = act64.reshape(B * Q, K), target.reshape(-1)
    base, valid = _masked_ce(pred, gold, pad_idx, exclude_idx)
    am = first_argmax(pred)
    l_act = (base * w.repeat_interleave(Q)).mean()
    n_act_ok, n_act = int(((am == gold) & valid).sum()), int(valid.sum())
    info.update(act_argmax=am, act_valid=valid, weights=w, last_ref=ref)
    # duration
    mask = (td != float(pad_idx)).double()
    od = F.normalize(torch.exp(dur64) * mask, p=1, dim=-1)
    tgt = td if val_mode else td * mask * mask
    den = mask.sum() if dur_den is None else torch.tensor(float(dur_den), dtype=torch.float64)
    l_dur = ((od - tgt) ** 2).sum() / den
    total = l_seg + l_act + l_dur
    wrt = [t for t in (seg64, act64, dur64) if t is not None]
    grads = list(torch.autograd.grad(total, wrt, allow_unused=True))
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, wrt)]
    d_dur, d_act = grads.pop() * grad_scale, grads.pop() * grad_scale
    d_seg = grads.pop() * grad_scale if grads else None
    return dict(loss=torch.stack([l_seg, l_act, l_dur, total]).detach(), counts=[n_seg_ok, n_seg, n_act_ok, n_act],
                d_seg=d_seg, d_act=d_act, d_dur=d_dur, info=info)


def finalize64(part, B, S, Q, has_seg, dur_den):
    """part: [units, 4] float32 partials in the layout [N | BQ | B] of a loss launch -> (loss [4] float64, counts [4])"""
    N, BQ = B * S, B * Q
    p = np.asarray(part, dtype=np.float64).reshape(N + BQ + B, 4)
    g0, g1, g2 = p[:N], p[N:N + BQ], p[N + BQ:]
    den = float(dur_den) if dur_den is not None else g2[:, 2].sum() / B
    ls = g0[:, 0].sum() / N if has_seg else 0.0
    la = g1[:, 0].sum() / BQ
    ld = g2[:, 0].sum() / den
    counts = [int(round(g0[:, 1].sum())), int(round(g0[:, 2].sum())), int(round(g1[:, 1].sum())), int(round(g1[:, 2].sum()))]
    return np.array([ls, la, ld, ls + la + ld]), counts


# ----------------------------------------------------------------------------------------------------------
# AdamW
# ----------------------------------------------------------------------------------------------------------
def adamw64(p, g, m, v, step, lr, wd, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
    """One torch.optim.AdamW step (single-tensor form) on float64 numpy copies of p, g, m, v; step is 1-based.  Returns the
    new (p, m, v).  The hyper-parameters are used as given: a caller that compares with a launch whose hyper-parameters
    travel as float32 passes their float32 values."""
    p, g, m, v = (np.array(a, dtype=np.float64) for a in (p, g, m, v))
    g *= grad_scale
    p *= 1.0 - lr * wd
    m += (g - m) * (1.0 - b1)                       # exp_avg.lerp_(grad, 1 - beta1)
    v *= b2
    v += (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    g = np.sqrt(v)                                  # (g's storage is free from here)
    g /= np.sqrt(bc2)
    g += eps
    np.divide(m, g, out=g)
    g *= lr / bc1
    p -= g
    return p, m, v


# ----------------------------------------------------------------------------------------------------------
# Philox4x32-10 keep-masks
# ----------------------------------------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays"""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]             # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _LO, p1 >> _S32, p1 & _LO
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def philox_thresh(p):
    t = float(np.float32(p)) * 4294967296.0
    return int(min(t, 4294967295.0))


def philox_words(n, seed, offset):
    """the raw words behind a mask of n bytes: [ceil(n / 4), 4] uint32, row i = Philox(counter (i, offset), key seed)"""
    n4 = (n + 3) // 4
    i = np.arange(n4, dtype=np.uint64)
    off = int(offset) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10((i & _LO, i >> _S32, np.full(n4, off & 0xFFFFFFFF, dtype=np.uint64), np.full(n4, off >> 32, dtype=np.uint64)),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return np.stack(r, axis=1)


def mask_of_words(words, n, p):
    return (words.reshape(-1)[:n] >= np.uint32(philox_thresh(p))).astype(np.uint8)


def philox_mask(n, p, seed, offset):
    """uint8 [n]: byte 4 i + j is 1 (keep) when word j of counter i is >= thresh(p)"""
    return mask_of_words(philox_words(n, seed, offset), n, p)
