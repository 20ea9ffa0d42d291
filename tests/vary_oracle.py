"""CPU restatement of the activation-magnitude token fuser model (model/futr_safuser_tokenfusion_vary.py), composed from
the building blocks of oracle/futr_oracle.py.  The FUTR around the fuser is the token-fusion one (:89-220); the fuser
differs in three places:
  * score = mean_(B,T) |x| per channel in every mode, k = C // 4 smallest by the CPU torch.topk rule (:40-46);
  * selected RGB channels <- alpha * depth, selected depth channels <- alpha * rgb, the rest unchanged (:48-56);
  * no x_res: fused = mean over the token pair of norm(Block(x)) (:76-86)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import futr_oracle as O
from tests.helpers import fixture_params


def is_live(name):
    return name == "fuser.alpha" or O.is_live(name)


def vary_params(fx):
    """The fixture's parameters: the analytic fill, with the RGB embedding channels meta['dead_rgb'] made dead (zero
    weight row, negative bias: ReLU output exactly 0 on every row, so their scores tie at exactly 0)."""
    p = fixture_params(fx)
    dead = fx["meta"].get("dead_rgb", [])
    if dead:
        p["input_embed.weight"][dead] = 0.0
        p["input_embed.bias"][dead] = -1.0
    return p


def token_fusion_vary(p, rgb, dep):
    B, T, C = rgb.shape
    s_rgb = rgb.detach().abs().mean(dim=(0, 1))
    s_dep = dep.detach().abs().mean(dim=(0, 1))
    k = C // 4
    idx_rgb = torch.from_numpy(O.select_smallest(s_rgb.numpy().astype(np.float32), k))
    idx_dep = torch.from_numpy(O.select_smallest(s_dep.numpy().astype(np.float32), k))
    m_rgb = torch.zeros(C, dtype=torch.bool)
    m_dep = torch.zeros(C, dtype=torch.bool)
    m_rgb[idx_rgb] = True
    m_dep[idx_dep] = True
    alpha = p["fuser.alpha"].reshape(C)
    ex_rgb = torch.where(m_rgb, alpha * dep, rgb)
    ex_dep = torch.where(m_dep, alpha * rgb, dep)
    return torch.stack([ex_rgb, ex_dep], dim=2), idx_rgb, idx_dep, s_rgb, s_dep


def cm_fuser_vary(p, rgb, dep, n_head):
    B, T, C = rgb.shape
    stacked, idx_rgb, idx_dep, s_rgb, s_dep = token_fusion_vary(p, rgb, dep)
    x = O.fuser_block(p, stacked.reshape(B * T, 2, C), n_head)
    x = O.layer_norm(x, p["fuser.norm.weight"], p["fuser.norm.bias"])
    fused = x.mean(dim=1).view(B, T, C)
    return fused, dict(idx_rgb=idx_rgb, idx_dep=idx_dep, score_rgb=s_rgb, score_dep=s_dep)


def forward(p, inputs, depth, mode, pad_idx, n_head=8, n_layers=1):
    """FUTR.forward (futr_safuser_tokenfusion_vary.py:152-220), input_type 'i3d_transcript', dropout omitted."""
    src, src_label = inputs
    B, S, _ = src.shape
    kpm = (src_label == pad_idx) if mode == "train" else None
    rgb = F.relu(F.linear(src, p["input_embed.weight"], p["input_embed.bias"]))
    pos = p["pos_embedding"][:, :S]
    d = depth.reshape(B, S, -1)
    d = F.linear(d, p["depth_projection.weight"], p["depth_projection.bias"])
    d = F.relu(O.layer_norm(d, p["depth_layernorm.weight"], p["depth_layernorm.bias"]))
    fused, aux = cm_fuser_vary(p, rgb, d, n_head)
    qpos = p["query_embed.weight"].unsqueeze(0)
    tgt = O.decoder(p, fused, pos, qpos, kpm, n_head, n_layers, capture=aux)
    out = {"action": F.linear(tgt, p["fc.weight"], p["fc.bias"]),
           "duration": F.linear(tgt, p["fc_len.weight"], p["fc_len.bias"]).squeeze(2),
           "seg": F.linear(fused, p["fc_seg.weight"], p["fc_seg.bias"])}
    aux["fused"] = fused
    return out, aux


class Trainer:
    """forward + the three losses + autograd backward + AdamW over a parameter dict; dtype float32 or float64."""

    def __init__(self, params, pad_idx, n_head=8, n_layers=1, lr=1e-3, wd=5e-3, dtype=torch.float32):
        self.p = {k: v.clone().to(dtype).requires_grad_(is_live(k)) for k, v in params.items()}
        self.pad_idx, self.n_head, self.n_layers, self.lr, self.wd = pad_idx, n_head, n_layers, lr, wd
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items() if v.requires_grad}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items() if v.requires_grad}
        self.t = 0

    def step(self, batch, apply=True, mode="train"):
        feats, depth, lab, dur, tgt = batch
        dt = self.p["fc.weight"].dtype
        for q in self.p.values():
            q.grad = None
        out, aux = forward(self.p, (feats.to(dt), lab), depth.to(dt), mode, self.pad_idx, self.n_head, self.n_layers)
        res = O.losses(out, lab, dur.to(dt), tgt, self.pad_idx)
        res["loss"].backward()
        if apply:
            self.t += 1
            with torch.no_grad():
                for k, q in self.p.items():
                    if q.grad is not None:
                        O.adamw_step(q, q.grad, self.m[k], self.v[k], self.t, self.lr, self.wd)
        return res, out, aux
