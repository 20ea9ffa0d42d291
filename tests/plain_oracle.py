"""CPU restatement of the plain SA-Fuser model (model/futr_safuser_depth.py), composed from the building blocks of
oracle/futr_oracle.py.  The FUTR around the fuser is the token-fusion one with a 160 x 120 depth projection; the fuser
differs in three places:
  * no selection or exchange: the two embeddings are stacked as they are (:43-46);
  * the learnable fuser.modality_token [1, 1, 1, C] is added to both tokens of every frame (:40,48);
  * no x_res: fused = mean over the token pair of norm(Block(x)) (:53-62)."""
import torch
import torch.nn.functional as F

from oracle import futr_oracle as O
from tests.helpers import fixture_params


def is_live(name):
    return name == "fuser.modality_token" or O.is_live(name)


def plain_params(fx):
    return fixture_params(fx)


def cm_fuser_plain(p, rgb, dep, n_head):
    B, T, C = rgb.shape
    x = torch.stack([rgb, dep], dim=2) + p["fuser.modality_token"].reshape(1, 1, 1, C)
    x = O.fuser_block(p, x.reshape(B * T, 2, C), n_head)
    x = O.layer_norm(x, p["fuser.norm.weight"], p["fuser.norm.bias"])
    return x.mean(dim=1).view(B, T, C)


def forward(p, inputs, depth, mode, pad_idx, n_head=8, n_layers=1):
    """FUTR.forward (futr_safuser_depth.py:138-217), input_type 'i3d_transcript', dropout omitted.  inputs: (features,
    labels) in train mode; the bare features or that tuple otherwise."""
    if mode == "train" or isinstance(inputs, (tuple, list)):
        src, src_label = inputs
    else:
        src, src_label = inputs, None
    B, S, _ = src.shape
    kpm = (src_label == pad_idx) if mode == "train" else None
    rgb = F.relu(F.linear(src, p["input_embed.weight"], p["input_embed.bias"]))
    pos = p["pos_embedding"][:, :S]
    d = depth.reshape(B, S, -1)
    d = F.linear(d, p["depth_projection.weight"], p["depth_projection.bias"])
    d = F.relu(O.layer_norm(d, p["depth_layernorm.weight"], p["depth_layernorm.bias"]))
    fused = cm_fuser_plain(p, rgb, d, n_head)
    qpos = p["query_embed.weight"].unsqueeze(0)
    aux = {}
    tgt = O.decoder(p, fused, pos, qpos, kpm, n_head, n_layers, capture=aux)
    out = {"action": F.linear(tgt, p["fc.weight"], p["fc.bias"]),
           "duration": F.linear(tgt, p["fc_len.weight"], p["fc_len.bias"]).squeeze(2),
           "seg": F.linear(fused, p["fc_seg.weight"], p["fc_seg.bias"])}
    aux["fused"] = fused
    return out, aux


class Trainer:
    """forward + the three losses + autograd backward + AdamW over a parameter dict; dtype float32 or float64.
    erank_weight != 0: total loss -= erank_weight * effective rank of the fused tokens (through torch.linalg.svdvals)."""

    def __init__(self, params, pad_idx, n_head=8, n_layers=1, lr=1e-3, wd=5e-3, dtype=torch.float32, erank_weight=0.0):
        self.p = {k: v.clone().to(dtype).requires_grad_(is_live(k)) for k, v in params.items()}
        self.pad_idx, self.n_head, self.n_layers, self.lr, self.wd = pad_idx, n_head, n_layers, lr, wd
        self.erank_weight = erank_weight
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
        loss = res["loss"]
        if self.erank_weight != 0.0:
            aux["erank"] = O.effective_rank_torch(aux["fused"].reshape(-1, aux["fused"].shape[-1]))
            loss = loss - self.erank_weight * aux["erank"]
        loss.backward()
        if apply:
            self.t += 1
            with torch.no_grad():
                for k, q in self.p.items():
                    if q.grad is not None:
                        O.adamw_step(q, q.grad, self.m[k], self.v[k], self.t, self.lr, self.wd)
        return res, out, aux
