"""Float64 restatement of the build-defined three-modality (RGB + depth + gaze) token-fusion model
(r3d_amd/model/futr_safuser_tokenfusion3.py, r3d_amd/engine_m3.py, csrc/fuse3_seam.hip): the embedding seam piece by piece --
its backward written out by hand, not taken from autograd -- and the whole training step.  Plain torch on the CPU; nothing here
comes from r3d_amd.  Every function computes in the dtype of its inputs, so the same text on float32 copies is the "float32
restatement" tests/m3_cases.py measures its tolerances with.

The step is composed of pieces that are already pinned: oracle.futr_oracle's embeddings, decoder, heads, losses and AdamW (the
fixtures made from the imported reference pin them), tests/fuser3_oracle.py for the fuser (tied to oracle.cm_fuser_m and, at
two modalities, to the reference-pinned oracle.cm_fuser), and the gaze branch -- Linear, LayerNorm, ReLU, the form of the
reference's depth branch (model/futr_safuser_tokenfusion.py:194-197)."""
import torch
import torch.nn.functional as F

from oracle import futr_oracle as O
from tests import fuser3_oracle as F3

LN_EPS = 1e-5
LIVE_PREFIXES = O.LIVE_PREFIXES + ("gaze_projection.", "gaze_layernorm.")
GAZE_KEYS = ("gaze_projection.weight", "gaze_projection.bias", "gaze_layernorm.weight", "gaze_layernorm.bias")


# ---------------------------------------------------------------------------------------------------------------------
# the seam: forward and hand-written backward
# ---------------------------------------------------------------------------------------------------------------------
def _ln_stats(x):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + LN_EPS)


def seam_forward(rgb_src, ns_r, bias_r, dep_src, bias_d, lnd_g, lnd_b, gaze, w_g, b_g, lng_g, lng_b, mask, keep, drop_scale,
                 ln1_g, ln1_b):
    """rgb_src: [ns_r, N, H] slabs (bias_r and the ReLU applied here) or, with ns_r == 0, the finished [N, H] embedding;
    dep_src [ns_d, N, H] slabs (+ bias_d when given); gaze [N, G]; mask [3, H]; keep None or [3 N, H] of 0 / 1.
    -> dict(rgb, dep_pre, mean_d, rstd_d, dep, gz_pre, mean_g, rstd_g, gz, x0, h1, m1, r1); rows of x0 / h1 are 3 n + m."""
    rgb_pre = rgb_src.sum(dim=0) + bias_r if ns_r > 0 else None
    rgb = F.relu(rgb_pre) if ns_r > 0 else rgb_src
    dep_pre = dep_src.sum(dim=0)
    if bias_d is not None:
        dep_pre = dep_pre + bias_d
    mean_d, rstd_d = _ln_stats(dep_pre)
    dep = F.relu((dep_pre - mean_d) * rstd_d * lnd_g + lnd_b)
    gz_pre = gaze @ w_g.t() + b_g
    mean_g, rstd_g = _ln_stats(gz_pre)
    gz = F.relu((gz_pre - mean_g) * rstd_g * lng_g + lng_b)
    x0 = F3.exchange3([rgb, dep, gz], mask, keep, drop_scale)
    m1, r1 = _ln_stats(x0)
    h1 = (x0 - m1) * r1 * ln1_g + ln1_b
    return dict(rgb=rgb, rgb_pre=rgb_pre, dep_pre=dep_pre, mean_d=mean_d[:, 0], rstd_d=rstd_d[:, 0], dep=dep, gz_pre=gz_pre, mean_g=mean_g[:, 0],
                rstd_g=rstd_g[:, 0], gz=gz, x0=x0, h1=h1, m1=m1[:, 0], r1=r1[:, 0])


def _ln_adjoint(dy, x, mean, rstd, gamma):
    """(dx, per-row dgamma terms, per-row dbeta terms) of y = (x - mean) rstd gamma + beta for the cotangent dy"""
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(dim=-1, keepdim=True) - xhat * (g * xhat).mean(dim=-1, keepdim=True))
    return dx, dy * xhat, dy


def seam_backward(d_h1, fw, add1, add2, keep, drop_scale, mask, ln1_g, lnd_g, lnd_b, lng_g, lng_b, gaze):
    """The adjoint of seam_forward from the cotangent d_h1 [3 N, H] of h1 and the residual gradients add1 / add2 (None or
    [3 N, H], added to norm1's input gradient), written out from the formulas.  fw: seam_forward's dict.
    -> dict(d_rgb_pre, d_dep_pre, d_gz_pre [N, H]; p_n1, p_dep, p_gz [N, 2, H]: per-frame (dgamma, dbeta) partials, the three
    token rows of a frame summed for norm1; d_w_g [H, G], d_b_g [H])."""
    N, H = fw["rgb"].shape
    d_x0, t_g, t_b = _ln_adjoint(d_h1, fw["x0"], fw["m1"], fw["r1"], ln1_g)
    if add1 is not None:
        d_x0 = d_x0 + add1
    if add2 is not None:
        d_x0 = d_x0 + add2
    p_n1 = torch.stack([t_g.reshape(N, 3, H).sum(dim=1), t_b.reshape(N, 3, H).sum(dim=1)], dim=1)
    d_rgb, d_dep, d_gz = F3.exchange3_adjoint(d_x0, mask, keep, drop_scale)
    d_rgb_pre = torch.where(fw["rgb"] > 0, d_rgb, torch.zeros_like(d_rgb))
    out = dict(d_rgb_pre=d_rgb_pre, p_n1=p_n1)
    for tag, d, pre, mean, rstd, g, b in (("dep", d_dep, fw["dep_pre"], fw["mean_d"], fw["rstd_d"], lnd_g, lnd_b),
                                          ("gz", d_gz, fw["gz_pre"], fw["mean_g"], fw["rstd_g"], lng_g, lng_b)):
        y = (pre - mean[:, None]) * rstd[:, None] * g + b
        d = torch.where(y > 0, d, torch.zeros_like(d))
        dx, tg, tb = _ln_adjoint(d, pre, mean, rstd, g)
        out["d_" + tag + "_pre"] = dx
        out["p_" + tag] = torch.stack([tg, tb], dim=1)
    out["d_w_g"] = out["d_gz_pre"].t() @ gaze
    out["d_b_g"] = out["d_gz_pre"].sum(dim=0)
    return out


def relu_margin(fw, lnd_g, lnd_b, lng_g, lng_b, ns_r):
    """The smallest |pre-activation| in front of the seam's three ReLUs (the RGB one only where the seam applies it): a
    float32 implementation gates an element within rounding of zero either way."""
    ys = [(fw["dep_pre"] - fw["mean_d"][:, None]) * fw["rstd_d"][:, None] * lnd_g + lnd_b,
          (fw["gz_pre"] - fw["mean_g"][:, None]) * fw["rstd_g"][:, None] * lng_g + lng_b]
    if ns_r > 0:
        ys.append(fw["rgb_pre"])
    return min(float(y.abs().min()) for y in ys)


# ---------------------------------------------------------------------------------------------------------------------
# the whole model and its training step
# ---------------------------------------------------------------------------------------------------------------------
def gaze_embed(p, gaze):
    g = F.linear(gaze, p["gaze_projection.weight"], p["gaze_projection.bias"])
    return F.relu(O.layer_norm(g, p["gaze_layernorm.weight"], p["gaze_layernorm.bias"]))


def forward(p, inputs, depth, gaze, mode, pad_idx, n_head=8, n_layers=1, keep=None, drop_scale=1.0):
    """p: {name: tensor} of one dtype.  The two-modality oracle.forward with the gaze embedding and the three-modality fuser;
    everything behind `fused` is that function's text.  Returns (outputs, aux)."""
    src, src_label = inputs
    dt = p["input_embed.weight"].dtype
    src, depth, gaze = src.to(dt), depth.to(dt), gaze.to(dt)
    B, S, _ = src.shape
    kpm = (src_label == pad_idx) if mode == "train" else None
    rgb = F.relu(F.linear(src, p["input_embed.weight"], p["input_embed.bias"]))
    pos = p["pos_embedding"][:, :S]
    d = F.linear(depth.reshape(B, S, -1), p["depth_projection.weight"], p["depth_projection.bias"])
    d = F.relu(O.layer_norm(d, p["depth_layernorm.weight"], p["depth_layernorm.bias"]))
    gz = gaze_embed(p, gaze)
    fused, aux = F3.cm_fuser3(p, [rgb, d, gz], mode, n_head, keep, drop_scale)
    tgt = O.decoder(p, fused, pos, p["query_embed.weight"].unsqueeze(0), kpm, n_head, n_layers, capture=aux)
    out = {"action": F.linear(tgt, p["fc.weight"], p["fc.bias"]),
           "duration": F.linear(tgt, p["fc_len.weight"], p["fc_len.bias"]).squeeze(2),
           "seg": F.linear(fused, p["fc_seg.weight"], p["fc_seg.bias"])}
    aux.update(fused=fused, rgb_embed=rgb, depth_embed=d, gaze_embed=gz)
    return out, aux


def step(params, batch, pad_idx, n_head, n_layers, dtype=torch.float64, erank_weight=0.0, keep=None, drop_scale=1.0):
    """One forward + the three losses (- erank_weight * effective rank of the fused tokens) + backward.
    batch = (features, depth, past_label, trans_dur_future, trans_future_target, gaze).
    -> (outputs, losses dict of oracle.losses, {name: grad or None}, aux)"""
    p = {n: v.detach().to(dtype).clone().requires_grad_(n.startswith(LIVE_PREFIXES)) for n, v in params.items()}
    feats, depth, lab, dur, tgt, gaze = batch
    out, aux = forward(p, (feats, lab), depth, gaze, "train", pad_idx, n_head, n_layers, keep, drop_scale)
    res = O.losses(out, lab, dur, tgt, pad_idx)
    total = res["loss"]
    if erank_weight != 0.0:
        H = aux["fused"].shape[-1]
        total = total - erank_weight * O.effective_rank_torch(aux["fused"].reshape(-1, H))
    total.backward()
    return out, res, {n: v.grad for n, v in p.items()}, aux
