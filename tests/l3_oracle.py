"""Restatement of the L3 query model's own pieces, written from their formulas, in float64 and -- for the tolerances of
tests/l3_cases.py -- in float32.

Cross-clip attention.  qkv [B, S, 3 H] is an in-projection output, columns [q | k | v], head h at columns h dh of each part.
The reference calls nn.MultiheadAttention(batch_first=True) on the activations after 'b t c -> t b c', so for each frame t
and head h the B rows of the batch attend to one another, without mask or dropout:
    s[t, h] = q[:, t, h] k[:, t, h]^T / sqrt(dh)   [B, B],    p = softmax over the key clip,    o[:, t, h] = p v[:, t, h].
Adjoint, written out:  dv = p^T d_o,  dp = d_o v^T,  ds = p (dp - rowsum(p dp)),  dq = ds k / sqrt(dh),  dk = ds^T q / sqrt(dh).

Mix (train/train_unsupervised.py:357-362 of the reference).  l2_correct[r] = [label[r] != pad and argmax(seg[r]) == label[r]],
the arg-max being the first index of the maximum; m = mean_r (l3_correct[r] and l2_correct[r] ? 1 : 5) formed as torch forms a
float32 mean (the float32 sum over N);
    a = (1 - 1/m)(1 - wf),  b = (1 - 1/m) wf,  c = 1/m,  total = (1 - 1/m)((1 - wf) L_3 + wf L_c) + (1/m)(L_act + L_dur + L_seg),
and the gradients that reach the seg logits and the anticipation heads are scaled by c."""
import numpy as np
import torch


def _parts(qkv, heads):
    """qkv [B, S, 3 H] -> q, k, v as [S, heads, B, dh]"""
    B, S, W = qkv.shape
    H = W // 3
    dh = H // heads
    return [qkv[..., i * H:(i + 1) * H].reshape(B, S, heads, dh).permute(1, 2, 0, 3) for i in range(3)]


def _rows(x):
    """[S, heads, B, dh] -> [B, S, H]"""
    S, heads, B, dh = x.shape
    return x.permute(2, 0, 1, 3).reshape(B, S, heads * dh)


def xclip_probs(qkv, heads):
    q, k, _ = _parts(qkv, heads)
    return torch.softmax(q @ k.transpose(-1, -2) / np.sqrt(q.shape[-1]), dim=-1)


def xclip_fwd(qkv, heads, dtype=torch.float64):
    """o [B, S, H], every operation in `dtype`"""
    qkv = qkv.to(dtype)
    return _rows(xclip_probs(qkv, heads) @ _parts(qkv, heads)[2])


def xclip_bwd(qkv, d_o, heads, dtype=torch.float64):
    """d_qkv [B, S, 3 H] by the adjoint written out above (no autograd), every operation in `dtype`"""
    qkv, d_o = qkv.to(dtype), d_o.to(dtype)
    B, S, W = qkv.shape
    H = W // 3
    q, k, v = _parts(qkv, heads)
    g = d_o.reshape(B, S, heads, H // heads).permute(1, 2, 0, 3)
    p = xclip_probs(qkv, heads)
    dv = p.transpose(-1, -2) @ g
    dp = g @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    scale = 1.0 / np.sqrt(H // heads)
    dq, dk = ds @ k * scale, ds.transpose(-1, -2) @ q * scale
    return torch.cat([_rows(dq), _rows(dk), _rows(dv)], dim=-1)


def xclip_orders(qkv, d_o, heads):
    """The float32 restatement in two summation orders: as given, and with the clips and the head columns reversed (the same
    sums, taken from the other end).  Yields (o, d_qkv) in the argument's layout."""
    yield xclip_fwd(qkv, heads, torch.float32), xclip_bwd(qkv, d_o, heads, torch.float32)
    B, S, W = qkv.shape
    H = W // 3
    dh = H // heads
    flip = lambda x, n: x.reshape(B, S, n, heads, dh).flip(0, 4).reshape(B, S, n * H)      # noqa: E731
    o = xclip_fwd(flip(qkv, 3), heads, torch.float32)
    d = xclip_bwd(flip(qkv, 3), flip(d_o, 1), heads, torch.float32)
    yield flip(o, 1), flip(d, 3)


def first_argmax(x):
    """the first index of each row's maximum (x [N, K])"""
    x = np.asarray(x)
    return (x == x.max(axis=1, keepdims=True)).argmax(axis=1)


def top_two_gap(x):
    """each row's gap between its two largest entries (0 for a tie; inf for one column)"""
    x = np.sort(np.asarray(x, np.float64), axis=1)
    return x[:, -1] - x[:, -2] if x.shape[1] > 1 else np.full(x.shape[0], np.inf)


def mix(seg, label, pad_idx, l3_correct, L3, Lc, Lseg, Lact, Ldur, wf, dtype=np.float64):
    """dict(l2_correct, m, a, b, c, total).  m is the float32 torch computes whatever `dtype`; the rest runs in `dtype`."""
    label = np.asarray(label)
    l2 = (label != pad_idx) & (first_argmax(seg) == label)
    both = l2 & np.asarray(l3_correct, bool)
    N = len(label)
    m32 = np.float32(np.where(both, 1.0, 5.0).astype(np.float32).sum(dtype=np.float64)) / np.float32(N)
    t = dtype
    m, wf = t(m32), t(wf)
    c = t(1) / m
    r = t(1) - c
    total = r * ((t(1) - wf) * t(L3) + wf * t(Lc)) + c * (t(Lact) + t(Ldur) + t(Lseg))
    return dict(l2_correct=l2, m=m32, a=r * (t(1) - wf), b=r * wf, c=c, total=total)


# ---------------------------------------------------------------------------------------------------------------------
# the whole model and step (model/futr_unsupervised_temp3.py:72-143, train/train_unsupervised.py:300-362), dropout omitted
# ---------------------------------------------------------------------------------------------------------------------
L3_PAD, L3_EXCLUDE = 47, 48
LIVE_PREFIXES = ("input_embed.", "l3_attention.", "transformer.decoder.", "pos_embedding", "fc_seg.", "fc.", "fc_len.",
                 "fc_l3.")


def forward(p, inputs, mode, pad_idx, n_head=8, n_layers=1, n_query=8):
    """p: {name: tensor}, every tensor of one dtype (float64: the oracle; float32: the restatement the tolerances come from).
    Returns (outputs, aux)."""
    import torch.nn.functional as F
    from oracle import futr_oracle as O
    if mode == "train":
        src, src_label = inputs
        kpm = src_label == pad_idx
    else:
        src, kpm = (inputs[0] if isinstance(inputs, (tuple, list)) else inputs), None
    dt = p["input_embed.weight"].dtype
    src = src.to(dt)
    B, S, _ = src.shape
    H = p["input_embed.weight"].shape[0]
    pe = O.sinusoid_table(max(S, 1), H)[:, :S].to(dt)
    mem = F.relu(F.linear(src, p["input_embed.weight"], p["input_embed.bias"])) + pe
    qkv = F.linear(mem, p["l3_attention.in_proj_weight"], p["l3_attention.in_proj_bias"])
    o = _rows(xclip_probs(qkv, n_head) @ _parts(qkv, n_head)[2])
    l3 = F.linear(o, p["l3_attention.out_proj.weight"], p["l3_attention.out_proj.bias"]) + pe     # (the same sinusoid, :63-69)
    qpos = F.adaptive_avg_pool1d(l3.permute(0, 2, 1), n_query).permute(0, 2, 1)
    tgt = O.decoder(p, mem, p["pos_embedding"][:, :S], qpos, kpm, n_head, n_layers)
    out = {"action": F.linear(tgt, p["fc.weight"], p["fc.bias"]),
           "duration": F.linear(tgt, p["fc_len.weight"], p["fc_len.bias"]).squeeze(2),
           "seg": F.linear(mem, p["fc_seg.weight"], p["fc_seg.bias"]),
           "l3": F.linear(l3, p["fc_l3.weight"], p["fc_l3.bias"])}
    return out, dict(memory=mem, l3=l3, qpos=qpos, tgt=tgt)


def step_losses(out, past_label, trans_dur_future, trans_future_target, query_label, pad_idx, wf):
    """dict(L3, Lc, Lseg, Lact, Ldur, m, a, b, c, total (differentiable), l3_correct, l2_correct, counts) in the outputs' dtype"""
    import torch.nn.functional as F
    from oracle import futr_oracle as O
    from tests import temporal_oracle as TO
    l3, seg, act = out["l3"], out["seg"], out["action"]
    B, S, C = l3.shape
    K = seg.shape[-1]
    Lc = TO.loop_cluster(l3, TO.intervals(query_label))
    ql = query_label.reshape(-1)
    L3, l3_correct = TO.loop_focal(l3.reshape(-1, C), ql, L3_PAD, L3_EXCLUDE)
    l3_live = (ql != L3_PAD) & (ql != L3_EXCLUDE)
    # cal_loss with exclude_class_idx None: mask = gold != pad; + 2.0 [argmax == pad and unmasked]; mean over all rows
    gold = past_label.reshape(-1)
    mask = gold != pad_idx
    g = gold.clone()
    g[~mask] = -1
    segr = seg.reshape(-1, K)
    base = F.cross_entropy(segr, g, ignore_index=-1, reduction="none")
    arg = torch.from_numpy(first_argmax(segr.detach().numpy()))
    Lseg = (base + 2.0 * ((arg == pad_idx) & mask).to(base.dtype)).mean()
    l2_correct = arg == g
    # cal_weighted_loss with exclude None
    tg = trans_future_target.reshape(-1)
    tm = tg != pad_idx
    t2 = tg.clone()
    t2[~tm] = -1
    actr = act.reshape(-1, K)
    wts = torch.where(O.last_non_padding_labels(past_label, pad_idx) == trans_future_target[:, 0], 1.0, 10.0).to(base.dtype)
    Lact = (F.cross_entropy(actr, t2, ignore_index=-1, reduction="none") * wts.repeat_interleave(actr.shape[0] // B)).mean()
    dur_mask = (trans_dur_future != pad_idx).long()
    od = O.normalize_duration(out["duration"], dur_mask)
    td = (trans_dur_future * dur_mask * dur_mask).to(base.dtype)
    Ldur = torch.sum((od - td) ** 2) / torch.sum(dur_mask)
    how = torch.where(l3_correct & l2_correct, torch.tensor(1.0), torch.tensor(5.0))
    m = how.mean().to(base.dtype)                                  # (the float32 mean the loop forms)
    total = (1 - 1 / m) * ((1 - wf) * L3 + wf * Lc) + (1 / m) * (Lact + Ldur + Lseg)
    aarg = actr.argmax(1)
    return dict(L3=L3, Lc=Lc, Lseg=Lseg, Lact=Lact, Ldur=Ldur, m=m, a=(1 - 1 / m) * (1 - wf), b=(1 - 1 / m) * wf, c=1 / m,
                total=total, l3_correct=l3_correct, l2_correct=l2_correct,
                counts=[int(l2_correct.sum()), int(mask.sum()), int(((aarg == tg) & tm).sum()), int(tm.sum())],
                l3_counts=[int((l3_correct & l3_live).sum()), int(l3_live.sum())])


def step(params, batch, pad_idx, wf, n_head, n_layers, n_query, dtype=torch.float64):
    """One forward + loss + backward: (outputs, losses, {name: grad or None}); batch = (features, past_label,
    trans_dur_future, trans_future_target, query_label)."""
    p = {n: v.detach().to(dtype).clone().requires_grad_(True) for n, v in params.items()}
    feats, past_label, dur, target, query_label = batch
    out, _ = forward(p, (feats, past_label), "train", pad_idx, n_head, n_layers, n_query)
    res = step_losses(out, past_label, dur, target, query_label, pad_idx, wf)
    res["total"].backward()
    return out, res, {n: v.grad for n, v in p.items()}
