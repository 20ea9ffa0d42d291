"""Float64 restatement of the CNN baseline (reference model/cnn.py: the RNN baseline without its recurrence), of its loss
composition in train/train_unimodal.py and of the AdamW step, plus the row-tile kernel of csrc/cnn.hip piece by piece
(logits, per-row loss / valid / correct, d_seg, d_pre with d_x0 and d_extra) in numpy at any precision and summation
order -- the float32 variants measure what float32 arithmetic alone costs on a case's inputs (tests/cnn_cases.py).
Written here, not copied; tests/golden/make_golden_cnn.py cross-checks the model part against the imported reference."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import futr_oracle as O

EXCLUDE = 120                                   # train_unimodal.py:102,198,212
POOL = 8                                        # model/cnn.py:94
LIVE_PREFIXES = ("input_embed.", "fc_seg.", "fc.", "fc_len.")


def is_live(name):
    return name.startswith(LIVE_PREFIXES)


def forward(p, src, capture=None):
    """model/cnn.py:66-111 for src [B, S, D].  Returns dict(action [B,8,K], duration [B,8], seg [B,S,K-1], supcon [B,S,H])."""
    x = F.relu(src @ p["input_embed.weight"].T + p["input_embed.bias"])
    pooled = F.adaptive_avg_pool1d(x.permute(0, 2, 1), POOL).permute(0, 2, 1)
    out = dict(action=pooled @ p["fc.weight"].T + p["fc.bias"],
               duration=(pooled @ p["fc_len.weight"].T + p["fc_len.bias"]).squeeze(2),
               seg=x @ p["fc_seg.weight"].T + p["fc_seg.bias"], supcon=x)
    if capture is not None:
        capture.update(x=x, pooled=pooled)
    return out


def losses(out, past_label, dur, tgt, pad_idx):
    """train_unimodal.py:188-225: seg CE (cal_loss, + 2 where the arg-max is pad_idx) + weighted action CE + duration MSE,
    class 120 excluded from both cross entropies."""
    past_label = past_label.long()
    dur_mask = (dur != pad_idx).long()
    seg = out["seg"]
    Ks = seg.shape[-1]
    sp, sg = seg.reshape(-1, Ks), past_label.reshape(-1)
    base, mask = O.masked_ce(sp, sg, pad_idx, EXCLUDE)
    l_seg = (base + 2.0 * ((sp.argmax(dim=1) == pad_idx) & mask).to(base.dtype)).mean()
    sc, st = O.counts(sp, sg, pad_idx, EXCLUDE)
    K = out["action"].shape[-1]
    act, tg = out["action"].reshape(-1, K), tgt.reshape(-1)
    ref = O.last_non_padding_labels(past_label, pad_idx)
    base_a, _ = O.masked_ce(act, tg, pad_idx, EXCLUDE)
    w = torch.where(ref == tgt[:, 0], 1.0, 10.0).to(base_a.dtype).repeat_interleave(base_a.shape[0] // tgt.shape[0])
    l_act = (base_a * w).mean()
    ac, at = O.counts(act, tg, pad_idx, EXCLUDE)
    od = O.normalize_duration(out["duration"], dur_mask)
    l_dur = torch.sum((od - dur * dur_mask * dur_mask) ** 2) / torch.sum(dur_mask)
    return dict(loss_seg=l_seg, loss_action=l_act, loss_dur=l_dur, loss=l_seg + l_act + l_dur, seg_correct=sc,
                seg_total=st, act_correct=ac, act_total=at)


class Trainer:
    """forward + the three losses (+ extra(out, batch), e.g. a contrastive term) + autograd backward + AdamW over a
    parameter dict (float64 by default)."""

    def __init__(self, params, pad_idx, lr=1e-3, wd=5e-3, dtype=torch.float64, extra=None):
        self.p = {n: t.detach().to(dtype).clone().requires_grad_(is_live(n)) for n, t in params.items()}
        self.m = {n: torch.zeros_like(t) for n, t in self.p.items()}
        self.v = {n: torch.zeros_like(t) for n, t in self.p.items()}
        self.pad_idx, self.lr, self.wd, self.dtype, self.t, self.extra = pad_idx, lr, wd, dtype, 0, extra

    def step(self, batch, apply=True):
        feats, _depth, lab, dur, tgt = batch
        for q in self.p.values():
            q.grad = None
        aux = {}
        out = forward(self.p, feats.to(self.dtype), capture=aux)
        res = losses(out, lab, dur.to(self.dtype), tgt, self.pad_idx)
        total = res["loss"]
        if self.extra is not None:
            res["extra"] = self.extra(out, batch)
            total = total + res["extra"]
        total.backward()
        if apply:
            self.t += 1
            with torch.no_grad():
                for k, q in self.p.items():
                    if q.grad is not None:
                        O.adamw_step(q, q.grad, self.m[k], self.v[k], self.t, self.lr, self.wd)
        return res, out, aux


# ---------------------------------------------------------------------------------------------------------------------
# the row-tile kernel (csrc/cnn.hip), piece by piece
# ---------------------------------------------------------------------------------------------------------------------
ORDERS = ("ascending", "descending", "by4", "by16")


def _dot_rows(a, b, dtype, order):
    """a [M, C] . b [R, C]^T -> [M, R], every product and every addition rounded to dtype, the C terms added in `order`:
    ascending, descending, or as 4 / 16 interleaved partial sums (c mod 4, c mod 16) combined at the end.  float64: exact
    enough that the order does not matter; float32: the sums a kernel may legitimately reorder."""
    a, b = a.astype(dtype), b.astype(dtype)
    C = a.shape[1]
    if order in ("ascending", "descending"):
        acc = np.zeros((a.shape[0], b.shape[0]), dtype)
        for c in (range(C) if order == "ascending" else range(C - 1, -1, -1)):
            acc = (acc + a[:, c, None] * b[None, :, c]).astype(dtype)
        return acc
    lanes = 4 if order == "by4" else 16
    parts = [np.zeros((a.shape[0], b.shape[0]), dtype) for _ in range(lanes)]
    for c in range(C):
        parts[c % lanes] = (parts[c % lanes] + a[:, c, None] * b[None, :, c]).astype(dtype)
    acc = parts[0]
    for q in parts[1:]:
        acc = (acc + q).astype(dtype)
    return acc


def _exp(v, dtype):
    return np.exp(v.astype(np.float64)).astype(dtype)          # the correctly rounded exponential of the dtype's argument


def _log(v, dtype):
    return np.log(v.astype(np.float64)).astype(dtype)


def seg_rows(x, w, b, labels, pad_idx, exclude_idx, d_x0=None, d_extra=None, grad_scale=1.0, dtype=np.float64,
             order="ascending"):
    """What r3d_cnn_seg_step computes for x [N, H], w [Kseg, H], b [Kseg], labels [N]:
         logits [N, Kseg]; units [N, 3] = (loss term, correct, valid); argmax [N] (first occurrence of the largest logit);
         d_seg [N, Kseg] = (softmax - onehot) grad_scale / N on valid rows, 0 on masked ones;
         d_pre [N, H] = (x > 0) ? d_seg . w + d_x0 + d_extra : 0.
    A row is masked when its label is pad_idx, exclude_idx or outside [0, Kseg); a valid row whose arg-max is pad_idx pays
    + 2.  All arithmetic in `dtype`, sums in `order`."""
    x, w, b = np.asarray(x), np.asarray(w), np.asarray(b)
    labels = np.asarray(labels).astype(np.int64)
    N, H = x.shape
    K = w.shape[0]
    logits = (_dot_rows(x, w, dtype, order) + b.astype(dtype)[None, :]).astype(dtype)
    valid = (labels != pad_idx) & (labels != exclude_idx) & (labels >= 0) & (labels < K)
    am = logits.argmax(axis=1)
    m = logits.max(axis=1)
    e = _exp((logits - m[:, None]).astype(dtype), dtype)
    cols = range(K) if order != "descending" else range(K - 1, -1, -1)
    se = np.zeros(N, dtype)
    for c in cols:
        se = (se + e[:, c]).astype(dtype)
    lse = (m + _log(se, dtype)).astype(dtype)
    safe = np.where(valid, labels, 0)
    loss = np.where(valid, (lse - logits[np.arange(N), safe]).astype(dtype), dtype(0)).astype(dtype)
    loss = np.where(valid & (am == pad_idx), (loss + dtype(2.0)).astype(dtype), loss)
    units = np.stack([loss, (valid & (am == labels)).astype(dtype), valid.astype(dtype)], 1)
    scale = dtype(dtype(grad_scale) / dtype(N))
    soft = _exp((logits - lse[:, None]).astype(dtype), dtype)
    onehot = np.zeros((N, K), dtype)
    onehot[np.arange(N)[valid], labels[valid]] = 1
    d_seg = np.where(valid[:, None], ((soft - onehot).astype(dtype) * scale).astype(dtype), dtype(0)).astype(dtype)
    d_x = _dot_rows(d_seg, w.T, dtype, order)
    return dict(logits=logits, units=units, argmax=am, valid=valid, d_seg=d_seg, d_x=d_x,
                d_pre=gate(x, d_x, d_x0, d_extra, dtype))


def gate(x, d_x, d_x0=None, d_extra=None, dtype=np.float64):
    """d_pre = (x > 0) ? (d_x + d_x0) + d_extra : 0 in dtype (the kernel's epilogue)"""
    d = np.asarray(d_x).astype(dtype)
    if d_x0 is not None:
        d = (d + np.asarray(d_x0).astype(dtype)).astype(dtype)
    if d_extra is not None:
        d = (d + np.asarray(d_extra).astype(dtype)).astype(dtype)
    return np.where(np.asarray(x) > 0, d, dtype(0)).astype(dtype)


def top2_gap(logits):
    """per row: largest minus second largest logit (inf with a single class)"""
    if logits.shape[1] < 2:
        return np.full(logits.shape[0], np.inf)
    s = np.sort(logits, axis=1)
    return s[:, -1] - s[:, -2]
