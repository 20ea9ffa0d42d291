"""CPU restatement of the AFFT baseline (model/afft.py of the reference), on the front of tests/plain_oracle.py.  The front
is the plain SA-Fuser's (stack, + modality token, Block, fuser.norm, token mean); behind the fused tokens there is no
decoder (:189-201):
    pooled = adaptive_avg_pool1d(fused, Q)   -- as an explicit window average, pool_windows(S, Q)
    action, duration = fc(pooled), fc_len(pooled)
and no 'seg' output, so the loss is the weighted anticipation CE plus the duration loss (train_proposed_depth.py:184-213
with args.seg off).  Padded frames are pooled like any other: nothing of the forward reads the labels."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import futr_oracle as O
from tests import plain_oracle as PO

LIVE_PREFIXES = ("input_embed.", "depth_projection.", "depth_layernorm.", "fuser.blocks.0.", "fuser.norm.",
                 "fuser.modality_token", "fc.", "fc_len.")


def is_live(name):
    return name.startswith(LIVE_PREFIXES)


def pool_windows(S, Q):
    """[(start, end)] of F.adaptive_avg_pool1d over S frames down to Q: [floor(q S / Q), ceil((q + 1) S / Q))."""
    return [((q * S) // Q, -((-(q + 1) * S) // Q)) for q in range(Q)]


def pool_matrix(S, Q, dtype=torch.float64):
    """P [Q, S] with pooled = P @ frames; its transpose is the pool's adjoint (frame s: sum of d_pooled[q] / len_q)."""
    P = torch.zeros(Q, S, dtype=dtype)
    for q, (s0, s1) in enumerate(pool_windows(S, Q)):
        P[q, s0:s1] = 1.0 / (s1 - s0)
    return P


def pool(fused, Q):
    """fused [B, S, H] -> [B, Q, H]"""
    return torch.einsum("qs,bsh->bqh", pool_matrix(fused.shape[1], Q, fused.dtype), fused)


def front(p, src, depth, n_head, x0_hook=None):
    """relu(input_embed), relu(depth_layernorm(depth_projection)), the plain fuser -> fused [B, S, H].  x0_hook: callable on
    the stacked tokens + modality token [B*S, 2, H] (embd_drop with a given keep mask); None: no dropout."""
    B, S, _ = src.shape
    rgb = F.relu(F.linear(src, p["input_embed.weight"], p["input_embed.bias"]))
    d = F.linear(depth.reshape(B, S, -1), p["depth_projection.weight"], p["depth_projection.bias"])
    d = F.relu(O.layer_norm(d, p["depth_layernorm.weight"], p["depth_layernorm.bias"]))
    C = rgb.shape[-1]
    x = torch.stack([rgb, d], dim=2) + p["fuser.modality_token"].reshape(1, 1, 1, C)
    x = x.reshape(B * S, 2, C)
    if x0_hook is not None:
        x = x0_hook(x)
    x = O.fuser_block(p, x, n_head)
    x = O.layer_norm(x, p["fuser.norm.weight"], p["fuser.norm.bias"])
    return x.mean(dim=1).view(B, S, C), rgb, d


def heads(p, fused, Q):
    pooled = pool(fused, Q)
    return {"action": F.linear(pooled, p["fc.weight"], p["fc.bias"]),
            "duration": F.linear(pooled, p["fc_len.weight"], p["fc_len.bias"]).squeeze(2)}, pooled


def forward(p, inputs, depth, mode, pad_idx, n_head=8, n_query=8, x0_hook=None):
    """FUTR.forward (afft.py:138-214).  inputs: (features, labels) in train mode; the bare features or that tuple otherwise."""
    src = inputs[0] if isinstance(inputs, (tuple, list)) else inputs
    fused, rgb, dep = front(p, src, depth, n_head, x0_hook)
    out, pooled = heads(p, fused, n_query)
    return out, {"fused": fused, "pooled": pooled, "rgb": rgb, "dep": dep}


def losses(out, past_label, trans_dur_future, trans_future_target, pad_idx, val_mode=False):
    """train_proposed_depth.py:184-213 with args.seg off; val_mode: validate()'s unmasked duration target (:98-99)."""
    K = out["action"].shape[-1]
    dur_mask = (trans_dur_future != pad_idx).long()
    act = out["action"].reshape(-1, K)
    tgt = trans_future_target.reshape(-1)
    ref = O.last_non_padding_labels(past_label, pad_idx)
    l_act = O.action_loss(act, tgt, pad_idx, ref, trans_future_target[:, 0])
    res = {}
    res["act_correct"], res["act_total"] = O.counts(act, tgt, pad_idx)
    od = O.normalize_duration(out["duration"], dur_mask)
    td = trans_dur_future if val_mode else trans_dur_future * dur_mask * dur_mask
    l_dur = torch.sum((od - td) ** 2) / torch.sum(dur_mask)
    res.update(loss_seg=torch.zeros_like(l_act), loss_action=l_act, loss_dur=l_dur, loss=l_act + l_dur, seg_correct=0, seg_total=0)
    return res


def tail(fused, w_head, b_head, Q, past_label, dur, tgt, pad_idx, grad_scale=1.0):
    """The pooled-head chain on its own, float64 by default: fused [B, S, H] -> dict(pooled, actdur, d_actdur, d_fused, losses,
    counts); gradients of grad_scale * (loss_action + loss_dur)."""
    f = fused.detach().clone().requires_grad_(True)
    pooled = pool(f, Q)
    actdur = F.linear(pooled, w_head, b_head)
    actdur.retain_grad()
    K = w_head.shape[0] - 1
    res = losses({"action": actdur[..., :K], "duration": actdur[..., K]}, past_label, dur.to(f.dtype), tgt, pad_idx)
    (grad_scale * res["loss"]).backward()
    return dict(pooled=pooled.detach(), actdur=actdur.detach(), d_actdur=actdur.grad.detach(), d_fused=f.grad.detach(),
                losses=np.array([0.0] + [float(res[k].detach()) for k in ("loss_action", "loss_dur", "loss")]),
                counts=np.array([0, 0, res["act_correct"], res["act_total"]], np.int64))


class Trainer:
    """forward + the two losses + autograd backward + AdamW on the live set over a parameter dict; float32 or float64."""

    def __init__(self, params, pad_idx, n_head=8, n_query=8, lr=1e-3, wd=5e-3, dtype=torch.float32):
        self.p = {k: v.clone().to(dtype).requires_grad_(is_live(k)) for k, v in params.items()}
        self.pad_idx, self.n_head, self.n_query, self.lr, self.wd = pad_idx, n_head, n_query, lr, wd
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items() if v.requires_grad}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items() if v.requires_grad}
        self.t = 0

    def step(self, batch, apply=True, mode="train", x0_hook=None):
        feats, depth, lab, dur, tgt = batch
        dt = self.p["fc.weight"].dtype
        for q in self.p.values():
            q.grad = None
        out, aux = forward(self.p, (feats.to(dt), lab), depth.to(dt), mode, self.pad_idx, self.n_head, self.n_query, x0_hook)
        res = losses(out, lab, dur.to(dt), tgt, self.pad_idx)
        res["loss"].backward()
        if apply:
            self.t += 1
            with torch.no_grad():
                for k, q in self.p.items():
                    if q.grad is not None:
                        O.adamw_step(q, q.grad, self.m[k], self.v[k], self.t, self.lr, self.wd)
        return res, out, aux


assert PO.is_live("fuser.modality_token")       # (the front this restatement stands on)
