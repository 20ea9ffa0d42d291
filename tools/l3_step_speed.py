#!/usr/bin/env python3
"""Timings of the L3 query model (model/futr_unsupervised_temp3.py) at hidden 128, 8 heads, query_num 49 and (B, S) = (8, 16),
(16, 256), (8, 1142); alternating rounds in one process, medians after a warm-up, device events, every round kept:

  (a) the cross-clip attention kernel (r3d_xclip_fwd, and fwd + r3d_xclip_bwd) against the composed form of the same
      arithmetic: transpose().contiguous() of the [B, S, 3H] in-projection output to [S, B, 3H], r3d_mha_core_* with batch S and
      length B, and a transposed copy back (the backward: d_o transposed in, d_qkv transposed out);
  (b) the graphed training step (engine_l3.L3Engine.train_step_graphed) against an eager PyTorch restatement of the same model
      written here -- nn.MultiheadAttention for both attentions' arithmetic, torch.optim.AdamW, the loop-form losses of
      tests/temporal_oracle.py (loop_intervals / loop_cluster / loop_focal: what a user of the reference runs) -- on the same
      GPU and batches.  A shape the engine refuses is recorded as refused, with the reason.

Prints one JSON line and writes it to --out.
    python tools/l3_step_speed.py [--steps 50] [--rounds 7] [--out profiles/l3_step_speed.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

K, H, D, HEADS, C, Q = 17, 128, 2048, 8, 49, 8
PAD = K + 1
SHAPES = ((8, 16), (16, 256), (8, 1142))
WD = 5e-3


def _timed(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def _rounds(fns, steps, rounds):
    """{name: (median, [rounds])} with the candidates alternating inside every round"""
    for f in fns.values():
        _timed(f, max(steps // 2, 5))
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            ms[k].append(_timed(f, steps))
    return {k: (statistics.median(v), [round(x, 5) for x in v]) for k, v in ms.items()}


def make_batch(B, S, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    feats = torch.randn(B, S, D, generator=g)
    lab = torch.randint(0, K - 1, (B, S), generator=g)
    lab[1::2, S - max(S // 8, 1):] = PAD
    tgt = torch.randint(0, K - 1, (B, Q), generator=g)
    dur = torch.rand(B, Q, generator=g) + 0.05
    dur = dur / dur.sum(1, keepdim=True)
    run = max(4, S // 12)                                 # about 12 label runs per clip (the loop-form cluster loss visits every pair)
    ql = torch.randint(0, 47, (B, (S + run - 1) // run), generator=g).repeat_interleave(run, dim=1)[:, :S].contiguous()
    return [t.to(dev) for t in (feats, lab, dur, tgt, ql)]


# ---------------------------------------------------------------------------------------------------------------------
# (a) the attention alone
# ---------------------------------------------------------------------------------------------------------------------
def time_xclip(B, S, dev, steps, rounds):
    from r3d_amd import ops
    dh = H // HEADS
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + S)
    qkv = torch.randn(B * S, 3 * H, generator=g).to(dev)
    d_o = torch.randn(B * S, H, generator=g).to(dev)
    o, d_qkv = torch.empty(B * S, H, device=dev), torch.empty(B * S, 3 * H, device=dev)
    row = {"frame_run": ops.xclip_frame_run(B, S, HEADS, dh, False), "frame_run_bwd": ops.xclip_frame_run(B, S, HEADS, dh, True)}
    fns = {"xclip_fwd": lambda i: ops.xclip_fwd(qkv, o, B, S, HEADS)}

    def both(i):
        ops.xclip_fwd(qkv, o, B, S, HEADS)
        ops.xclip_bwd(qkv, d_o, d_qkv, B, S, HEADS)
    fns["xclip_fwd_bwd"] = both
    if ops.mha_core_supported(B, B, dh, True):
        probs = torch.empty(S, HEADS, B, B, device=dev)
        ot, dt = torch.empty(S * B, H, device=dev), torch.empty(S * B, 3 * H, device=dev)
        o2, d2 = torch.empty(B * S, H, device=dev), torch.empty(B * S, 3 * H, device=dev)

        def comp_fwd(i):
            t = qkv.view(B, S, 3 * H).transpose(0, 1).contiguous().view(S * B, 3 * H)
            ops.mha_core_fwd(t[:, :H], t[:, H:2 * H], t[:, 2 * H:], probs, ot, S, HEADS, B, B, dh)
            o2.view(B, S, H).copy_(ot.view(S, B, H).transpose(0, 1))
            return t

        def comp_both(i):
            t = comp_fwd(i)
            gt = d_o.view(B, S, H).transpose(0, 1).contiguous().view(S * B, H)
            ops.mha_core_bwd(t[:, :H], t[:, H:2 * H], t[:, 2 * H:], probs, gt, dt[:, :H], dt[:, H:2 * H], dt[:, 2 * H:], S, HEADS,
                             B, B, dh)
            d2.view(B, S, 3 * H).copy_(dt.view(S, B, 3 * H).transpose(0, 1))
        fns["composed_fwd"], fns["composed_fwd_bwd"] = comp_fwd, comp_both
        both(0), comp_both(0)
        torch.cuda.synchronize()
        row["max_abs_diff_o"] = float((o - o2).abs().max())
        row["max_abs_diff_d_qkv"] = float((d_qkv - d2).abs().max())
    else:
        row["composed"] = "refused: r3d_mha_core does not take this (length, head width)"
    for k, (med, rs) in _rounds(fns, steps, rounds).items():
        row[k + "_ms"], row[k + "_rounds"] = round(med, 5), rs
    return row


# ---------------------------------------------------------------------------------------------------------------------
# (b) the training step
# ---------------------------------------------------------------------------------------------------------------------
def _model_args():
    return argparse.Namespace(input_dim=D, seg=True, anticipate=True, max_pos_len=2000, input_type="i3d_transcript")


class TorchL3(torch.nn.Module):
    """The model's live path in PyTorch's own layers (dropout omitted, as in the timed engine): the yardstick, not the product."""

    def __init__(self):
        super().__init__()
        L, M = torch.nn.Linear, torch.nn.MultiheadAttention
        self.input_embed, self.l3_attention = L(D, H), M(H, HEADS, batch_first=True)
        self.sa, self.ca = M(H, HEADS), M(H, HEADS)
        self.l1, self.l2 = L(H, 4 * H), L(4 * H, H)
        self.n1, self.n2, self.n3, self.nf = (torch.nn.LayerNorm(H) for _ in range(4))
        self.fc_seg, self.fc, self.fc_len, self.fc_l3 = L(H, K), L(H, K), L(H, 1), L(H, C)
        self.pos_embedding = torch.nn.Parameter(torch.randn(1, 2000, H) * 0.02)
        pos = torch.arange(2000).unsqueeze(1)
        div = torch.exp(torch.arange(0, H, 2) * -(torch.log(torch.tensor(10000.0)) / H))
        pe = torch.zeros(2000, H)
        pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
        self.register_buffer("pe", pe)

    def forward(self, src, lab):
        B, S, _ = src.shape
        mem = (F.relu(self.input_embed(src)) + self.pe[:S]).transpose(0, 1)                 # [S, B, H]
        l3 = self.l3_attention(mem, mem, mem)[0].transpose(0, 1) + self.pe[:S]              # batch = frames, sequence = clips
        qp = F.adaptive_avg_pool1d(l3.permute(0, 2, 1), Q).permute(2, 0, 1)                 # [Q, B, H]
        kv = mem + self.pos_embedding[0, :S].unsqueeze(1)
        t = self.n1(self.sa(qp, qp, qp)[0])                                                  # (tgt = 0)
        t = self.n2(t + self.ca(t + qp, kv, kv, key_padding_mask=lab == PAD)[0])
        t = self.nf(self.n3(t + self.l2(F.relu(self.l1(t))))).transpose(0, 1)
        return dict(action=self.fc(t), duration=self.fc_len(t).squeeze(2), seg=self.fc_seg(mem.transpose(0, 1)), l3=self.fc_l3(l3))


def torch_step(model, opt, batch, wf, TO):
    feats, lab, dur, tgt, ql = batch
    out = model(feats, lab)
    B, S, _ = out["l3"].shape
    Lc = TO.loop_cluster(out["l3"], TO.loop_intervals(ql))
    L3, l3c = TO.loop_focal(out["l3"].reshape(B * S, C), ql.reshape(-1), 47, 48)
    seg, g = out["seg"].reshape(B * S, K), torch.where(lab == PAD, -1, lab).reshape(-1)
    Ls = (F.cross_entropy(seg, g, ignore_index=-1, reduction="none") + 2.0 * ((seg.argmax(1) == PAD) & (g >= 0)).float()).mean()
    l2c = seg.argmax(1) == g
    keep = lab != PAD
    last = lab.gather(1, ((keep * torch.arange(1, S + 1, device=lab.device)).max(1).values - 1).clamp_min(0).unsqueeze(1)).squeeze(1)
    wts = torch.where(last == tgt[:, 0], 1.0, 10.0).repeat_interleave(Q)
    La = (F.cross_entropy(out["action"].reshape(B * Q, K), torch.where(tgt == PAD, -1, tgt).reshape(-1), ignore_index=-1,
                          reduction="none") * wts).mean()
    m = (dur != PAD).float()
    Ld = ((F.normalize(torch.exp(out["duration"]) * m, p=1, dim=-1) - dur * m) ** 2).sum() / m.sum()
    how = torch.where(l3c & l2c, 1.0, 5.0).mean()
    loss = (1 - 1 / how) * ((1 - wf) * L3 + wf * Lc) + (1 / how) * (La + Ld + Ls)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    return loss


def time_step(B, S, dev, steps, rounds):
    sys.path.insert(0, ROOT)
    from tests import temporal_oracle as TO
    from r3d_amd.model.futr_unsupervised_temp3 import FUTR
    batches = [make_batch(B, S, dev, seed=s) for s in range(4)]
    wf = 0.5
    row = {}
    torch.manual_seed(1)
    model = FUTR(K, H, PAD, dev, _model_args(), n_query=Q, n_head=HEADS, num_encoder_layers=2, num_decoder_layers=1,
                 query_num=C).to(dev)
    model.r3d_dropout_enabled = False
    fns = {}
    try:
        eng = model.engine()
        acc = (torch.zeros(6, dtype=torch.float64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev))

        def hip(i):
            b = batches[i % 4]
            eng.train_step_graphed(b[0], b[1], b[2], b[3], b[4], 1e-3, WD, wf, True, (0.9, 0.999), 1e-8, acc)
        hip(0)
        torch.cuda.synchronize()
        row["loss_first_step"] = float(acc[0][0])
        fns["hip_graphed"] = hip
    except ValueError as e:
        row["hip_graphed"] = f"refused: {e}"[:300]
    torch.manual_seed(1)
    tm = TorchL3().to(dev)
    opt = torch.optim.AdamW(tm.parameters(), 1e-3, weight_decay=WD)
    fns["torch_eager"] = lambda i: torch_step(tm, opt, batches[i % 4], wf, TO)
    slow = max(2, steps // 10) if S > 64 else steps                   # (loop_intervals reads every frame label back)
    out = {}
    if "hip_graphed" in fns:
        out.update(_rounds({"hip_graphed": fns["hip_graphed"]}, steps, rounds))
    out.update(_rounds({"torch_eager": fns["torch_eager"]}, slow, max(3, rounds // 2)))
    for k, (med, rs) in out.items():
        row[k + "_ms_per_step"], row[k + "_rounds"] = round(med, 4), rs
    if "hip_graphed" in out:
        row["torch_over_hip"] = round(out["torch_eager"][0] / out["hip_graphed"][0], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"H": H, "heads": HEADS, "query_num": C, "K": K, "steps": a.steps, "rounds": a.rounds,
           "what": "medians over rounds, device events; (a) attention kernel vs composed transposes + mha_core, alternating; "
                   "(b) graphed step vs eager torch restatement with loop-form losses (dropout off on both)"}
    for B, S in SHAPES:
        res[f"B{B}_S{S}"] = {"attention": time_xclip(B, S, dev, a.steps, a.rounds), "step": time_step(B, S, dev, a.steps, a.rounds)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
