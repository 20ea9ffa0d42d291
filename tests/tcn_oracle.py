"""Float64 restatement of the TCN baseline (reference model/tcn.py), of the loss its loop uses (cal_performance without an
excluded class) and of one AdamW step, in plain tensor operations: each convolution is written as three shifted matrix
products (tap j of the [C_out, C_in, 3] weight reads frame t - (2 - j) d of the same clip, zeros before frame 0), weight
normalisation as g v / |v|.  Gradients come from autograd over this restatement.  tests/golden/make_golden_tcn.py
cross-checks it against the imported reference."""
import torch
import torch.nn.functional as F

from oracle import futr_oracle as O

CHANNELS = (256, 512, 512, 256)
IN_DIM = 2048
LEVELS = [(i, IN_DIM if i == 0 else CHANNELS[i - 1], c, 2 ** i) for i, c in enumerate(CHANNELS)]
# (C_in, C_out, dilation) of the eight convolutions
CONVS = [(ci, co, d) for _, ci, co, d in LEVELS] + [(co, co, d) for _, _, co, d in LEVELS]


def shift_frames(x, k):
    """x [B, S, C] -> frames moved k steps later (k > 0: frame t holds x[t - k], zeros before) or earlier (k < 0)."""
    if k == 0:
        return x
    S = x.shape[1]
    z = torch.zeros_like(x)
    if abs(k) >= S:
        return z
    if k > 0:
        z[:, k:] = x[:, :S - k]
    else:
        z[:, :S + k] = x[:, -k:]
    return z


def conv_raw(x, v, d):
    """P = X (*) v: x [B, S, C_in], v [C_out, C_in, 3] -> [B, S, C_out]."""
    return sum(shift_frames(x, (2 - j) * d) @ v[:, :, j].T for j in range(3))


def wn_scale(v, g):
    return g.reshape(-1) / v.reshape(v.shape[0], -1).norm(dim=1)


def wn_conv(x, v, g, b, d):
    return conv_raw(x, v, d) * wn_scale(v, g) + b


def conv_products(x, v, dz, d):
    """The three products of one convolution on the raw weight: forward P, input gradient dX, weight gradient G."""
    x = x.detach().clone().requires_grad_(True)
    v = v.detach().clone().requires_grad_(True)
    p = conv_raw(x, v, d)
    p.backward(dz)
    return p.detach(), x.grad, v.grad


def fill_params(names_shapes):
    """oracle.synth.fill_state: unit-variance weight_v rows (|v_o| ~ 1), g uniform in +-sqrt(3), biases 0.1 u: the
    pre-activations stay of order one through all eight convolutions."""
    from oracle import synth
    return {n: torch.from_numpy(a) for n, a in synth.fill_state(names_shapes).items()}


def names_shapes(num_classes, anticipated_frames=8):
    out = []
    for i, ci, co, _ in LEVELS:
        pre = f"tcn_local.network.{i}."
        for c, cin in (("conv1", ci), ("conv2", co)):
            out += [(pre + c + ".bias", (co,)), (pre + c + ".weight_g", (co, 1, 1)), (pre + c + ".weight_v", (co, cin, 3))]
        if ci != co:
            out += [(pre + "downsample.weight", (co, ci, 1)), (pre + "downsample.bias", (co,))]
    out += [("regression.weight", (num_classes * anticipated_frames, CHANNELS[-1], 1)),
            ("regression.bias", (num_classes * anticipated_frames,))]
    return out


def forward(p, x, anticipated_frames=8, masks=None, drop_scale=1.0, capture=None):
    """model/tcn.py:74-80 for x [B, S, 2048] -> [B, anticipated_frames, num_classes].  masks: None or eight keep-masks
    [B, S, C] in the order of the dropouts.  capture: a list that receives (level, 'conv1' | 'conv2' | 'out', the ReLU's
    input) for the twelve ReLUs."""
    for i, ci, co, d in LEVELS:
        pre = f"tcn_local.network.{i}."
        a1 = wn_conv(x, p[pre + "conv1.weight_v"], p[pre + "conv1.weight_g"], p[pre + "conv1.bias"], d)
        y = F.relu(a1)
        if masks is not None:
            y = y * masks[2 * i] * drop_scale
        a2 = wn_conv(y, p[pre + "conv2.weight_v"], p[pre + "conv2.weight_g"], p[pre + "conv2.bias"], d)
        y = F.relu(a2)
        if masks is not None:
            y = y * masks[2 * i + 1] * drop_scale
        res = x if ci == co else x @ p[pre + "downsample.weight"][:, :, 0].T + p[pre + "downsample.bias"]
        x = F.relu(y + res)
        if capture is not None:
            capture += [(i, "conv1", a1.detach()), (i, "conv2", a2.detach()), (i, "out", (y + res).detach())]
    out = x @ p["regression.weight"][:, :, 0].T + p["regression.bias"]          # [B, S, Q * K]
    B, S, _ = out.shape
    return out.reshape(B, S, anticipated_frames, -1).mean(dim=1)


def kink_channels(capture):
    """ReLU units whose input is within rounding of zero in the oracle: an fp32 product may land on the other side of the
    kink, which flips that unit's share of its channel's bias / weight_g / weight_v gradient entirely.  Identified BY
    CONSTRUCTION from the oracle, by the rule of tests/helpers.ffn_kink_units: 0 < |u| <= 2e-6 max|u|, the size of the fp32
    accumulation error of a dot product (an input that is exactly zero has a zero on both sides: ReLU of two exact zeros).
    Returns {parameter name: set of channels} for the biases and weight_g a flip reaches directly."""
    out = {}
    for i, which, u in capture:
        near = ((u.abs() <= 2e-6 * float(u.abs().max())) & (u != 0)).reshape(-1, u.shape[-1]).any(dim=0).nonzero().flatten().tolist()
        pre = f"tcn_local.network.{i}."
        names = [pre + "conv1.bias", pre + "conv1.weight_g"] if which == "conv1" else [pre + "conv2.bias", pre + "conv2.weight_g"]
        if which == "out":
            names.append(pre + "downsample.bias")
        for n in names:
            out.setdefault(n, set()).update(near)
    return out


def loss_counts(out, target, pad_idx):
    """cal_performance(output.view(-1, C), target.view(-1), pad_idx): CE of the rows whose target != pad_idx (+ 2 where the
    arg-max is pad_idx), mean over ALL rows; n_correct, n_total over the unmasked rows."""
    C = out.shape[-1]
    pred, gold = out.reshape(-1, C), target.reshape(-1).long()
    mask = gold != pad_idx
    lse = torch.logsumexp(pred, dim=1)
    picked = pred.gather(1, torch.where(mask, gold, torch.zeros_like(gold)).unsqueeze(1)).squeeze(1)
    base = torch.where(mask, lse - picked, torch.zeros_like(lse))
    arg = pred.argmax(dim=1)
    loss = (base + 2.0 * ((arg == pad_idx) & mask).to(base.dtype)).mean()
    return loss, int(((arg == gold) & mask).sum()), int(mask.sum())


class Trainer:
    """forward + loss + autograd backward + AdamW over a parameter dict (float64 by default)."""

    def __init__(self, params, pad_idx, lr=1e-3, wd=5e-3, dtype=torch.float64, anticipated_frames=8):
        self.p = {n: t.detach().to(dtype).clone().requires_grad_(True) for n, t in params.items()}
        self.m = {n: torch.zeros_like(t) for n, t in self.p.items()}
        self.v = {n: torch.zeros_like(t) for n, t in self.p.items()}
        self.pad_idx, self.lr, self.wd, self.dtype, self.t, self.Q = pad_idx, lr, wd, dtype, 0, anticipated_frames

    def step(self, feats, target, apply=True):
        for q in self.p.values():
            q.grad = None
        out = forward(self.p, feats.to(self.dtype), self.Q)
        loss, nc, nt = loss_counts(out, target, self.pad_idx)
        loss.backward()
        if apply:
            self.t += 1
            with torch.no_grad():
                for k, q in self.p.items():
                    O.adamw_step(q, q.grad, self.m[k], self.v[k], self.t, self.lr, self.wd)
        return loss.detach(), nc, nt, out.detach()
