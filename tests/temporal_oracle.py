"""Restatement of the temporal auxiliary losses and of run detection, written from their formulas.

Runs.  A run of clip b starts at t = 0 and wherever labels[b, t] != labels[b, t - 1].

Cluster.  Run r of clip b has n_r frames and mean m_r; R_b runs in clip b, total = sum_b R_b:
    intra = sum_{b,r} mean_{t in r, c} (x - m_r)^2 / total
    inter = sum_{b: R_b > 1} sum_{i<j} 1 / (1e-5 + |m_i - m_j|) / (M (n_last - 1)),  M = #{b : R_b > 1}, n_last = R_b of the last
            such clip; 0 when M = 0.

Contrastive.  Per clip z = x / max(|x|, 1e-12), p = softmax(z z^T / tau) over all columns.  Frame t of run (st, en) has
    P(t) = {c : st <= c <= en, c != t - st};  loss = sum_b sum_r [sum_{t in r} sum_{P(t)} -log(p_tc + 1e-5)] / (|P_r| + 1e-5) / B.

Focal.  A row is masked when gold is pad, the excluded class, or outside [0, C).  CE = -log softmax(pred)[gold], p = exp(-CE):
    loss = sum over unmasked rows of alpha (1 - p)^gamma CE + penalty [argmax == pad], divided by N.

``cluster`` / ``contrastive`` / ``focal`` compute in float64 whatever they are given and are differentiable, so autograd gives the
gradients the kernels are compared with.  The ``loop_*`` functions are the same losses in the form a user of the reference runs
today -- one small torch call per run or pair, run detection by a per-frame host loop, in the dtype and on the device of their
input: tools/temporal_loss_speed.py times them."""
import torch
import torch.nn.functional as F

EPS = 1e-5


def intervals(labels):
    """labels [B, T] -> list (per clip) of lists of (start, end)"""
    lab = labels.cpu()
    B, T = lab.shape
    out = []
    for b in range(B):
        cut = [0] + (1 + (lab[b, 1:] != lab[b, :-1]).nonzero().flatten()).tolist() + [T]
        out.append([(cut[i], cut[i + 1] - 1) for i in range(len(cut) - 1)])
    return out


def frame_runs(iv, T):
    """(first [B, T], last [B, T], count [B]) as int64 tensors"""
    B = len(iv)
    first, last = torch.empty(B, T, dtype=torch.int64), torch.empty(B, T, dtype=torch.int64)
    for b, clip in enumerate(iv):
        for s, e in clip:
            first[b, s:e + 1], last[b, s:e + 1] = s, e
    return first, last, torch.tensor([len(c) for c in iv])


def cluster(x, iv):
    x = x.double()
    intra, inter, total, M, n_last = 0.0, 0.0, 0, 0, 0
    for b, clip in enumerate(iv):
        means = torch.stack([x[b, s:e + 1].mean(0) for s, e in clip])
        for r, (s, e) in enumerate(clip):
            intra = intra + ((x[b, s:e + 1] - means[r]) ** 2).mean()
        total += len(clip)
        if len(clip) > 1:
            i, j = torch.triu_indices(len(clip), len(clip), 1)
            inter = inter + (1.0 / (EPS + (means[i] - means[j]).norm(dim=1))).sum()
            M, n_last = M + 1, len(clip)
    loss = intra / total
    if M:
        loss = loss + inter / (M * (n_last - 1))
    return loss


def positive_mask(clip, T):
    m = torch.zeros(T, T, dtype=torch.bool)
    for s, e in clip:
        m[s:e + 1, s:e + 1] = True
        for i in range(e - s + 1):
            m[s + i, i] = False
    return m


def contrastive(x, iv, temperature=0.07, stats=False):
    """the loss; with stats=True also (lse [B, T], Q [B, T]) detached"""
    x = x.double()
    B, T, _ = x.shape
    loss, lse_all, q_all = 0.0, [], []
    for b, clip in enumerate(iv):
        z = x[b] / x[b].norm(dim=1, keepdim=True).clamp_min(1e-12)
        s = z @ z.t() / temperature
        lse = torch.logsumexp(s, dim=1, keepdim=True)
        p = torch.exp(s - lse)
        mask = positive_mask(clip, T)
        term = -torch.log(p + EPS) * mask
        for st, en in clip:
            loss = loss + term[st:en + 1].sum() / (mask[st:en + 1].sum().double() + EPS)
        lse_all.append(lse[:, 0].detach())
        q_all.append((p / (p + EPS) * mask).sum(1).detach())
    loss = loss / B
    return (loss, torch.stack(lse_all), torch.stack(q_all)) if stats else loss


def focal(pred, gold, pad, exclude=None, alpha=1.0, gamma=2.0, penalty=0.0):
    """(loss, flags [N] bool, n_correct, n_word)"""
    pred = pred.double()
    N, C = pred.shape
    live = (gold != pad) & (gold >= 0) & (gold < C)
    if exclude is not None:
        live &= gold != exclude
    logp = F.log_softmax(pred, dim=1)
    ce = -logp[torch.arange(N), gold.clamp(0, C - 1)]
    arg = pred.argmax(1)
    row = alpha * (1.0 - torch.exp(-ce)) ** gamma * ce + penalty * (arg == pad).double()
    loss = (row * live).sum() / N
    flags = live & (arg == gold)
    return loss, flags, int(flags.sum()), int(live.sum())


def with_grad(fn, x, *args, **kw):
    """(fn(x, ...) detached, d / d x) in float64; fn returns the loss or a tuple that starts with it"""
    xr = x.detach().double().requires_grad_(True)
    out = fn(xr, *args, **kw)
    loss = out[0] if isinstance(out, tuple) else out
    if loss.requires_grad:
        loss.backward()
    g = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    return loss.detach(), g


# ---------------------------------------------------------------------------------------------------------------------
# the loop form: what a user of the reference runs today (tools/temporal_loss_speed.py)
# ---------------------------------------------------------------------------------------------------------------------
def loop_intervals(gt):
    """per-frame host loop: one device-to-host read per frame"""
    B, T = gt.shape
    out = []
    for b in range(B):
        runs, start, cur = [], 0, gt[b, 0].item()
        for t in range(1, T):
            v = gt[b, t].item()
            if v != cur:
                runs.append((start, t - 1))
                start, cur = t, v
        runs.append((start, T - 1))
        out.append(runs)
    return out


def loop_cluster(x, iv):
    intra, inter, kept, total = 0.0, 0.0, [], 0
    for b, clip in enumerate(iv):
        means = []
        for s, e in clip:
            rows = x[b, s:e + 1]
            m = rows.mean(dim=0, keepdim=True)
            means.append(m)
            intra = intra + F.mse_loss(rows, m.expand_as(rows))
        if len(means) > 1:
            kept.append(torch.cat(means, dim=0))
        total += len(clip)
    n = 0
    for means in kept:
        n = means.shape[0]
        for i in range(n):
            for j in range(i + 1, n):
                inter = inter + 1.0 / (EPS + torch.norm(means[i] - means[j], p=2))
    loss = intra / total
    if kept:
        loss = loss + inter / (len(kept) * (n - 1))
    return loss


def loop_contrastive(x, iv, temperature=0.07):
    loss = 0.0
    for b, clip in enumerate(iv):
        z = F.normalize(x[b], p=2, dim=1)
        for s, e in clip:
            sim = z[s:e + 1] @ z.t() / temperature
            ex = torch.exp(sim)
            mask = torch.zeros_like(sim)
            mask[:, s:e + 1] = 1
            mask.fill_diagonal_(0)
            term = -torch.log(ex / ex.sum(dim=1, keepdim=True) + EPS)
            loss = loss + (term * mask).sum() / (mask.sum() + EPS)
    return loss / len(iv)


def loop_focal(pred, gold, pad, exclude=None, alpha=1.0, gamma=2.0, penalty=0.0):
    mask = gold != pad
    if exclude is not None:
        mask = mask & (gold != exclude)
    tgt = gold.clone()
    tgt[~mask] = -1
    ce = F.cross_entropy(pred, tgt, ignore_index=-1, reduction="none")
    flags = pred.argmax(dim=-1) == tgt
    p = F.softmax(pred, dim=1)[torch.arange(pred.shape[0], device=pred.device), gold]
    row = alpha * (1 - p) ** gamma * ce + penalty * ((pred.argmax(dim=1) == pad) & mask).float()
    return row.mean(), flags
