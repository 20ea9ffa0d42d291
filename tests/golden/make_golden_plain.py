#!/usr/bin/env python3
"""Generates tests/golden/plain_*.npz by IMPORTING THE REFERENCE's plain SA-Fuser model (model/futr_safuser_depth.py)
on CPU -- build container only.  Same conventions and the same single shim as make_golden_vary.py (the mask's
.to('cuda') becomes a no-op); dropout probabilities are set to 0 (RNG parity is impossible).  Parameters: the analytic
oracle.synth fill (fuser.modality_token included); depth maps of 120 x 160 (the module's 160 * 120 projection).  Per case:
a train-mode step (outputs, losses, counters, gradient statistics, d modality_token in full, post-AdamW statistics), a
val-mode forward with the bare feature tensor (futr_safuser_depth.py:145), the state_dict key list and per-parameter
checksums of a torch.manual_seed(1) init.  Every value is cross-checked against tests/plain_oracle.py; the script aborts
on a mismatch."""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("R3D_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
sys.path[:0] = [REF, os.path.join(REF, "train")]

from oracle import synth  # noqa: E402
from opts import parser  # noqa: E402
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402   (helpers: ref_losses, stats, check_close, t_batch)
from tests import plain_oracle as PO  # noqa: E402


class _CpuMask(torch.Tensor):
    def to(self, *a, **k):
        return self.as_subclass(torch.Tensor)


M = importlib.import_module("model.futr_safuser_depth")
_orig = M.CMFuser.__dict__["generate_cross_attention_mask"].__func__
M.CMFuser.generate_cross_attention_mask = staticmethod(lambda sz: _orig(sz).as_subclass(_CpuMask))
LR, WD = 1e-3, 5e-3
DEPTH_HW = (120, 160)


def _new(H, n_class, n_dec):
    args = parser.parse_args([])
    args.hidden_dim, args.n_head, args.n_decoder_layer, args.n_query = H, 8, n_dec, 8
    pad_idx = n_class + 1
    model = M.FUTR(n_class, H, device=torch.device("cpu"), args=args, src_pad_idx=pad_idx, n_query=8, n_head=8,
                   num_encoder_layers=args.n_encoder_layer, num_decoder_layers=n_dec)
    return model, pad_idx


def build(H, n_class, n_dec):
    model, pad_idx = _new(H, n_class, n_dec)
    names_shapes = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    state = synth.fill_state(names_shapes)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[n]))
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    return model, pad_idx, names_shapes


def init_checksums(H, n_class, n_dec):
    """(sum, sum of squares) in float64 of every parameter of a torch.manual_seed(1) init, in named_parameters order."""
    torch.manual_seed(1)
    model, _ = _new(H, n_class, n_dec)
    return np.array([[float(p.detach().double().sum()), float((p.detach().double() ** 2).sum())]
                     for _, p in model.named_parameters()], np.float64)


def run_ref(model, inputs, depth, mode):
    holder = {}
    hook = model.fuser.register_forward_hook(lambda m, i, o: holder.__setitem__("fused", o[0]))
    try:
        out = model(inputs, depth, mode)
    finally:
        hook.remove()
    return out, holder["fused"]


def case(tag, H, B, S, n_class, n_dec, seed):
    model, pad_idx, names_shapes = build(H, n_class, n_dec)
    batch = G.t_batch(synth.make_batch(B, S, n_class, pad_idx, seed, depth_hw=DEPTH_HW))
    feats, depth, lab, dur, tgt = batch
    meta = dict(tag=tag, H=H, B=B, S=S, n_class=n_class, pad_idx=pad_idx, n_dec=n_dec, seed=seed, n_head=8, n_query=8,
                depth_hw=list(DEPTH_HW), variant="plain", lr=LR, wd=WD, torch=torch.__version__)
    fx = {"param_names": json.dumps([n for n, _ in names_shapes]),
          "param_shapes": json.dumps([list(s) for _, s in names_shapes]),
          "state_keys": json.dumps(list(model.state_dict().keys())),
          "init_sums": init_checksums(H, n_class, n_dec)}
    # ---- val-mode forward (no gradient, the bare feature tensor), then the train-mode step
    model.eval()
    with torch.no_grad():
        vout, vfused = run_ref(model, feats, depth, "val")
    model.train()
    out, fused = run_ref(model, (feats, lab), depth, "train")
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
        "val_fused": vfused.numpy(),
        "losses": np.array([float(res[k].detach()) for k in ("loss_seg", "loss_action", "loss_dur", "loss")], np.float64),
        "counts": np.array([res[k] for k in ("seg_correct", "seg_total", "act_correct", "act_total")], np.int64),
        "live_names": json.dumps(live),
        "grad_stats": np.stack([G.stats(grads[n]) for n in live]),
        "post_stats": np.stack([G.stats(post[n]) for n in live]),
    })
    for n in ("fuser.modality_token", "fuser.norm.weight", "depth_layernorm.weight", "input_embed.bias"):
        fx["grad::" + n] = grads[n].numpy()
    # ---- restatement cross-check --------------------------------------------------------------------------------------
    p0 = PO.plain_params(dict(meta=meta, param_names=[n for n, _ in names_shapes],
                              param_shapes=[list(s) for _, s in names_shapes]))
    tr = PO.Trainer(p0, pad_idx, 8, n_dec, lr=LR, wd=WD)
    with torch.no_grad():
        vo, vaux = PO.forward(tr.p, feats, depth, "val", pad_idx, 8, n_dec)
    for k in ("action", "duration", "seg"):
        G.check_close(f"{tag}/val/{k}", vo[k], vout[k])
    G.check_close(f"{tag}/val/fused", vaux["fused"], vfused)
    ores, oout, oaux = tr.step(batch, apply=True)
    for k in ("action", "duration", "seg"):
        G.check_close(f"{tag}/out/{k}", oout[k], out[k])
    G.check_close(f"{tag}/fused", oaux["fused"], fused)
    for k in ("loss_seg", "loss_action", "loss_dur", "loss"):
        G.check_close(f"{tag}/{k}", ores[k], res[k])
    for k, j in (("seg_correct", 0), ("seg_total", 1), ("act_correct", 2), ("act_total", 3)):
        assert int(ores[k]) == int(fx["counts"][j]), (tag, k)
    assert sorted(live) == sorted(n for n, q in tr.p.items() if q.grad is not None), "live set"
    assert "fuser.modality_token" in live and not any(n.startswith("fuser.projection") for n in live)
    for n in live:
        g = grads[n]
        G.check_close(f"{tag}/grad/{n}", tr.p[n].grad, g, tol=5e-5 * max(1.0, float(g.abs().max())))
        # (the exactly-zero Q/K gradients of the masked 2-token attention are rounding noise: AdamW may move them either way)
        keep = g.abs() > 1e-6 * max(1.0, float(g.abs().max()))
        G.check_close(f"{tag}/post/{n}", tr.p[n].detach()[keep], post[n][keep], tol=1e-5)
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **fx)
    print(f"[golden-plain] {tag}: loss={float(res['loss']):.6f} |d token|={float(grads['fuser.modality_token'].norm()):.3e} "
          f"live={len(live)} -> {os.path.getsize(path)/1024:.1f} KB")


if __name__ == "__main__":
    case("plain_tiny", 64, 2, 6, 17, 1, 5)
    case("plain_cfg2", 128, 8, 16, 17, 1, 9)
    case("plain_k122", 128, 4, 16, 122, 2, 13)
