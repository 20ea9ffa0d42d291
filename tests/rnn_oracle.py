"""Float64 restatement of the RNN baseline (reference model/rnn.py) and of its loss composition in train/train_unimodal.py,
with the LSTM written out gate by gate (PyTorch's order i, f, g, o; h0 = c0 = 0; no packing, no masking).  Gradients come
from autograd over this restatement.  tests/golden/make_golden_rnn.py cross-checks it against the imported reference."""
import torch
import torch.nn.functional as F

from oracle import futr_oracle as O

EXCLUDE = 120                                   # train_unimodal.py:102,198,212
POOL = 8                                        # model/rnn.py:97
LIVE_PREFIXES = ("input_embed.", "rnn.", "rnn_fc.", "fc_seg.", "fc.", "fc_len.")


def is_live(name):
    return name.startswith(LIVE_PREFIXES)


def lstm_direction(x, w_ih, w_hh, b_ih, b_hh, reverse):
    """One direction over x [B, S, I].  Returns y [B, S, h] and, per time step t, the activated gates [B, S, 4h], c_t
    [B, S, h] and the state the step started from, h_prev [B, S, h] (in the direction's own order)."""
    B, S, _ = x.shape
    h = w_hh.shape[1]
    hs = x.new_zeros(B, h)
    cs = x.new_zeros(B, h)
    ys, gates, cells, hprev = [None] * S, [None] * S, [None] * S, [None] * S
    for t in (range(S - 1, -1, -1) if reverse else range(S)):
        pre = x[:, t] @ w_ih.T + b_ih + hs @ w_hh.T + b_hh
        i = torch.sigmoid(pre[:, 0:h])
        f = torch.sigmoid(pre[:, h:2 * h])
        g = torch.tanh(pre[:, 2 * h:3 * h])
        o = torch.sigmoid(pre[:, 3 * h:4 * h])
        hprev[t] = hs
        cs = f * cs + i * g
        hs = o * torch.tanh(cs)
        ys[t], gates[t], cells[t] = hs, torch.cat([i, f, g, o], 1), cs
    st = lambda v: torch.stack(v, 1)       # noqa: E731
    return st(ys), st(gates), st(cells), st(hprev)


def lstm_layer(p, l, x):
    """Layer l of the bidirectional LSTM: y [B, S, 2h] = [fwd | rev]; aux per direction (gates, cell, hprev)."""
    outs, aux = [], []
    for sfx, rev in (("", False), ("_reverse", True)):
        y, g, c, hp = lstm_direction(x, p[f"rnn.weight_ih_l{l}{sfx}"], p[f"rnn.weight_hh_l{l}{sfx}"],
                                     p[f"rnn.bias_ih_l{l}{sfx}"], p[f"rnn.bias_hh_l{l}{sfx}"], rev)
        outs.append(y)
        aux.append((g, c, hp))
    return torch.cat(outs, -1), aux


def forward(p, src, capture=None):
    """model/rnn.py:71-114 for src [B, S, D].  Returns dict(action [B,8,K], duration [B,8], seg [B,S,K-1], supcon [B,S,H])."""
    x = F.relu(src @ p["input_embed.weight"].T + p["input_embed.bias"])
    y0, a0 = lstm_layer(p, 0, x)
    y1, a1 = lstm_layer(p, 1, y0)
    tgt = y1 @ p["rnn_fc.weight"].T + p["rnn_fc.bias"]
    pooled = F.adaptive_avg_pool1d(tgt.permute(0, 2, 1), POOL).permute(0, 2, 1)
    out = dict(action=pooled @ p["fc.weight"].T + p["fc.bias"],
               duration=(pooled @ p["fc_len.weight"].T + p["fc_len.bias"]).squeeze(2),
               seg=x @ p["fc_seg.weight"].T + p["fc_seg.bias"], supcon=tgt)
    if capture is not None:
        capture.update(x=x, y0=y0, y1=y1, aux0=a0, aux1=a1)
    return out


def losses(out, past_label, dur, tgt, pad_idx):
    """train_unimodal.py:188-225: seg CE (cal_loss) + weighted action CE + duration MSE, class 120 excluded."""
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
    """forward + the three losses + autograd backward + AdamW over a parameter dict (float64 by default)."""

    def __init__(self, params, pad_idx, lr=1e-3, wd=5e-3, dtype=torch.float64):
        self.p = {n: t.detach().to(dtype).clone().requires_grad_(is_live(n)) for n, t in params.items()}
        self.m = {n: torch.zeros_like(t) for n, t in self.p.items()}
        self.v = {n: torch.zeros_like(t) for n, t in self.p.items()}
        self.pad_idx, self.lr, self.wd, self.dtype, self.t = pad_idx, lr, wd, dtype, 0

    def step(self, batch, apply=True):
        feats, _depth, lab, dur, tgt = batch
        for q in self.p.values():
            q.grad = None
        aux = {}
        out = forward(self.p, feats.to(self.dtype), capture=aux)
        res = losses(out, lab, dur.to(self.dtype), tgt, self.pad_idx)
        res["loss"].backward()
        if apply:
            self.t += 1
            with torch.no_grad():
                for k, q in self.p.items():
                    if q.grad is not None:
                        O.adamw_step(q, q.grad, self.m[k], self.v[k], self.t, self.lr, self.wd)
        return res, out, aux


def lstm_layer_grads(x, w, dy):
    """Reference values for one bidirectional layer: x [B,S,H] f64, w = dict of the layer's 8 tensors keyed by
    (name, direction), dy [B,S,H] = dL/dy.  Returns dict(y, gates, cell, hprev, dg [B,S,4H] (pre-activation gate gradients
    of both directions), dx, dw_ih, dw_hh, db) -- dg by the explicit adjoint of the gate equations."""
    x = x.detach().clone().requires_grad_(True)
    ps = {k: v.detach().clone().requires_grad_(True) for k, v in w.items()}
    outs, keep = [], []
    for d, rev in ((0, False), (1, True)):
        y, g, c, hp = lstm_direction(x, ps[("w_ih", d)], ps[("w_hh", d)], ps[("b_ih", d)], ps[("b_hh", d)], rev)
        outs.append(y)
        keep.append((g, c, hp))
    y = torch.cat(outs, -1)
    y.backward(dy)
    h = w[("w_hh", 0)].shape[1]
    dgs = []
    for d, rev in ((0, False), (1, True)):
        g, c, hp = (t.detach() for t in keep[d])
        dgs.append(_gate_adjoint(g, c, dy[..., d * h:(d + 1) * h], ps[("w_hh", d)].detach(), rev))
    return dict(y=y.detach(), gates=torch.cat([k[0].detach() for k in keep], -1),
                cell=torch.cat([k[1].detach() for k in keep], -1), hprev=torch.cat([k[2].detach() for k in keep], -1),
                dg=torch.cat(dgs, -1), dx=x.grad, dw_ih=[ps[("w_ih", d)].grad for d in (0, 1)],
                dw_hh=[ps[("w_hh", d)].grad for d in (0, 1)], db=[ps[("b_ih", d)].grad for d in (0, 1)])


def _gate_adjoint(g, c, dy, w_hh, reverse):
    """dL/d(pre-activation gates) [B,S,4h] of one direction, walking its steps backwards (the recurrence kernel's math)."""
    B, S, h4 = g.shape
    h = h4 // 4
    dh_rec = g.new_zeros(B, h)
    dc = g.new_zeros(B, h)
    out = g.new_zeros(B, S, h4)
    order = list(range(S - 1, -1, -1)) if reverse else list(range(S))
    for k in range(S - 1, -1, -1):
        t = order[k]
        i, f, gg, o = g[:, t, :h], g[:, t, h:2 * h], g[:, t, 2 * h:3 * h], g[:, t, 3 * h:]
        cp = c[:, order[k - 1]] if k > 0 else torch.zeros_like(dc)
        tc = torch.tanh(c[:, t])
        dh = dy[:, t] + dh_rec
        dct = dc + dh * o * (1 - tc * tc)
        dg = torch.cat([dct * gg * i * (1 - i), dct * cp * f * (1 - f), dct * i * (1 - gg * gg), dh * tc * o * (1 - o)], 1)
        dc = dct * f
        out[:, t] = dg
        dh_rec = dg @ w_hh
    return out
