#!/usr/bin/env python3
"""Generates tests/golden/vary_*.npz by IMPORTING THE REFERENCE's activation-magnitude fuser variant
(model/futr_safuser_tokenfusion_vary.py) on CPU -- build container only.  Same conventions and the same single shim as
make_golden.py (the mask's .to('cuda') becomes a no-op); dropout probabilities are set to 0 (RNG parity is impossible).
Parameters: the analytic oracle.synth fill (fuser.alpha in [0.5, 0.95]: never 1, so the scale is exercised); the tiny
case also makes 20 RGB embedding channels dead (zero weight row, bias -1), more than k = C // 4 = 16, so the selection
among exact-zero score ties follows the CPU topk rule.  Per case: a train-mode step (outputs, losses, counters, selected
index sets + the relative gap at the selection boundary, gradient statistics, d alpha in full, post-AdamW statistics)
and a val-mode forward.  Every value is cross-checked against tests/vary_oracle.py; the script aborts on a mismatch."""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
sys.path[:0] = ["/root/reference", "/root/reference/train"]

from oracle import synth  # noqa: E402
from opts import parser  # noqa: E402
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402   (helpers: ref_losses, stats, check_close, t_batch)
from tests import vary_oracle as V  # noqa: E402


class _CpuMask(torch.Tensor):
    def to(self, *a, **k):
        return self.as_subclass(torch.Tensor)


M = importlib.import_module("model.futr_safuser_tokenfusion_vary")
_orig = M.CMFuser.__dict__["generate_cross_attention_mask"].__func__
M.CMFuser.generate_cross_attention_mask = staticmethod(lambda sz: _orig(sz).as_subclass(_CpuMask))
LR, WD = 1e-3, 5e-3


def build(H, n_class, n_dec, dead):
    args = parser.parse_args([])
    args.hidden_dim, args.n_head, args.n_decoder_layer, args.n_query = H, 8, n_dec, 8
    pad_idx = n_class + 1
    model = M.FUTR(n_class, H, device=torch.device("cpu"), args=args, src_pad_idx=pad_idx, n_query=8, n_head=8,
                   num_encoder_layers=args.n_encoder_layer, num_decoder_layers=n_dec)
    names_shapes = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    state = synth.fill_state(names_shapes)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[n]))
        if dead:
            model.input_embed.weight[dead] = 0.0
            model.input_embed.bias[dead] = -1.0
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    return model, pad_idx, names_shapes


def run_ref(model, feats, lab, depth, mode):
    holder, sel, real_topk = {}, [], torch.topk
    hook = model.fuser.register_forward_hook(lambda m, i, o: holder.__setitem__("fused", o))

    def spy(inp, *a, **k):
        r = real_topk(inp, *a, **k)
        sel.append((inp.detach().reshape(-1).clone(), r[1].reshape(-1).clone()))
        return r
    torch.topk = spy
    try:
        out = model((feats, lab), depth, mode)
    finally:
        torch.topk = real_topk
        hook.remove()
    return out, holder["fused"], sel


def case(tag, H, B, S, n_class, seed, dead=()):
    dead = list(dead)
    model, pad_idx, names_shapes = build(H, n_class, 1, dead)
    batch = G.t_batch(synth.make_batch(B, S, n_class, pad_idx, seed))
    feats, depth, lab, dur, tgt = batch
    meta = dict(tag=tag, H=H, B=B, S=S, n_class=n_class, pad_idx=pad_idx, n_dec=1, seed=seed, n_head=8, n_query=8,
                depth_hw=[224, 224], dead_rgb=dead, variant="vary", lr=LR, wd=WD, torch=torch.__version__)
    fx = {"param_names": json.dumps([n for n, _ in names_shapes]),
          "param_shapes": json.dumps([list(s) for _, s in names_shapes])}
    # ---- val-mode forward (no gradient), then the train-mode step
    model.eval()
    with torch.no_grad():
        vout, vfused, vsel = run_ref(model, feats, lab, depth, "val")
    model.train()
    out, fused, sel = run_ref(model, feats, lab, depth, "train")
    res = G.ref_losses(out, lab, dur, tgt, pad_idx)
    res["loss"].backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    live = list(grads)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.grad is not None], lr=LR, weight_decay=WD)
    opt.step()
    post = {n: p.detach().clone() for n, p in model.named_parameters() if n in grads}
    fx.update({
        "meta": json.dumps(meta),
        "out_action": out["action"].detach().numpy(), "out_duration": out["duration"].detach().numpy(),
        "out_seg": out["seg"].detach().numpy(), "fused": fused.detach().numpy(),
        "val_action": vout["action"].numpy(), "val_duration": vout["duration"].numpy(), "val_seg": vout["seg"].numpy(),
        "idx_rgb": np.sort(sel[0][1].numpy()), "idx_dep": np.sort(sel[1][1].numpy()),
        "val_idx_rgb": np.sort(vsel[0][1].numpy()), "val_idx_dep": np.sort(vsel[1][1].numpy()),
        "losses": np.array([float(res[k].detach()) for k in ("loss_seg", "loss_action", "loss_dur", "loss")], np.float64),
        "counts": np.array([res[k] for k in ("seg_correct", "seg_total", "act_correct", "act_total")], np.int64),
        "live_names": json.dumps(live),
        "grad_stats": np.stack([G.stats(grads[n]) for n in live]),
        "post_stats": np.stack([G.stats(post[n]) for n in live]),
    })
    for n in ("fuser.alpha", "fuser.norm.weight", "depth_layernorm.weight", "input_embed.bias"):
        fx["grad::" + n] = grads[n].numpy()
    for nm, j in (("rgb", 0), ("dep", 1)):
        s = np.sort(sel[j][0].numpy())
        k = H // 4
        fx["gap_" + nm] = np.array([(s[k] - s[k - 1]) / s[k] if s[k] > 0 else 0.0])       # 0: a tie at exactly 0
    # ---- restatement cross-check --------------------------------------------------------------------------------------
    p0 = V.vary_params(dict(meta=meta, param_names=[n for n, _ in names_shapes],
                            param_shapes=[list(s) for _, s in names_shapes]))
    tr = V.Trainer(p0, pad_idx, 8, 1, lr=LR, wd=WD)
    with torch.no_grad():
        vo, vaux = V.forward(tr.p, (feats, lab), depth, "val", pad_idx, 8, 1)
    for k in ("action", "duration", "seg"):
        G.check_close(f"{tag}/val/{k}", vo[k], vout[k])
    assert np.array_equal(np.sort(vaux["idx_rgb"].numpy()), fx["val_idx_rgb"])
    ores, oout, oaux = tr.step(batch, apply=True)
    for k in ("action", "duration", "seg"):
        G.check_close(f"{tag}/out/{k}", oout[k], out[k])
    G.check_close(f"{tag}/fused", oaux["fused"], fused)
    assert np.array_equal(np.sort(oaux["idx_rgb"].numpy()), fx["idx_rgb"]), (oaux["idx_rgb"], fx["idx_rgb"])
    assert np.array_equal(np.sort(oaux["idx_dep"].numpy()), fx["idx_dep"])
    for k in ("loss_seg", "loss_action", "loss_dur", "loss"):
        G.check_close(f"{tag}/{k}", ores[k], res[k])
    assert sorted(live) == sorted(n for n, q in tr.p.items() if q.grad is not None), "live set"
    # (tr.step applied AdamW: the gradients are still in .grad)
    for n in live:
        g = grads[n]
        G.check_close(f"{tag}/grad/{n}", tr.p[n].grad, g, tol=5e-5 * max(1.0, float(g.abs().max())))
        # (AdamW's first step moves every element by ~lr * sign(g): elements whose gradient is rounding noise -- the
        #  exactly-zero Q/K gradients of the masked 2-token attention -- may move either way, so they are not compared)
        keep = g.abs() > 1e-6 * max(1.0, float(g.abs().max()))
        G.check_close(f"{tag}/post/{n}", tr.p[n].detach()[keep], post[n][keep], tol=1e-5)
    if dead:
        zeros = int((sel[0][0] == 0).sum())
        assert zeros == len(dead) > H // 4, zeros
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **fx)
    print(f"[golden-vary] {tag}: loss={float(res['loss']):.6f} gap_rgb={fx['gap_rgb'][0]:.2e} "
          f"gap_dep={fx['gap_dep'][0]:.2e} live={len(live)} -> {os.path.getsize(path)/1024:.1f} KB")


if __name__ == "__main__":
    case("vary_tiny", 64, 2, 6, 17, 5, dead=range(3, 63, 3))
    case("vary_cfg2", 128, 8, 16, 17, 9)
    case("vary_k122", 128, 4, 16, 122, 13)
