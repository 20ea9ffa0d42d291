#!/usr/bin/env python3
"""Generates tests/golden/afft_*.npz by IMPORTING THE REFERENCE's AFFT baseline (model/afft.py) on CPU -- build container
only.  Same conventions and the same single shim as make_golden_plain.py (the mask's .to('cuda') becomes a no-op); dropout
probabilities are set to 0 (RNG parity is impossible); args.seg is off (the model has no 'seg' output, and the reference's
loop raises KeyError with it on).  Parameters: the analytic oracle.synth fill; depth maps of 224 x 224; n_query 8.  Per
case: a train-mode step (outputs, fused, the two losses composed from the reference's own functions, counters, gradient
and post-AdamW statistics, the live-name list), a val-mode forward with the bare feature tensor (afft.py:146), the
state_dict key lists (args.seg off and on) and per-parameter checksums of a torch.manual_seed(1) init.  Every value is
cross-checked against tests/afft_oracle.py; the script aborts on a mismatch."""
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
import make_golden as G  # noqa: E402   (helpers: stats, check_close, t_batch; the reference's utils as G.RU, its loop as G.T)
from tests import afft_oracle as AO  # noqa: E402


class _CpuMask(torch.Tensor):
    def to(self, *a, **k):
        return self.as_subclass(torch.Tensor)


M = importlib.import_module("model.afft")
_orig = M.CMFuser.__dict__["generate_cross_attention_mask"].__func__
M.CMFuser.generate_cross_attention_mask = staticmethod(lambda sz: _orig(sz).as_subclass(_CpuMask))
LR, WD = 1e-3, 5e-3
DEPTH_HW = (224, 224)
N_DEC = 1


def _new(H, n_class, seg=False):
    args = parser.parse_args([])
    args.hidden_dim, args.n_head, args.n_decoder_layer, args.n_query, args.seg = H, 8, N_DEC, 8, seg
    pad_idx = n_class + 1
    model = M.FUTR(n_class, H, device=torch.device("cpu"), args=args, src_pad_idx=pad_idx, n_query=8, n_head=8,
                   num_encoder_layers=args.n_encoder_layer, num_decoder_layers=N_DEC)
    return model, pad_idx, args


def build(H, n_class):
    model, pad_idx, args = _new(H, n_class)
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
    return model, pad_idx, names_shapes, args


def init_checksums(H, n_class):
    """(sum, sum of squares) in float64 of every parameter of a torch.manual_seed(1) init, in named_parameters order."""
    torch.manual_seed(1)
    model, _, _ = _new(H, n_class)
    return np.array([[float(p.detach().double().sum()), float((p.detach().double() ** 2).sum())]
                     for _, p in model.named_parameters()], np.float64)


def ref_losses(out, lab, dur, tgt, pad_idx):
    """The reference's loss composition with args.seg off (train_proposed_depth.py:184-213), from its own functions."""
    crit = torch.nn.MSELoss(reduction="none")
    dur_mask = (dur != pad_idx).long()
    target_dur = dur * dur_mask
    act = out["action"]
    B, Tq, C = act.size()
    first = G.T.get_last_non_padding_labels(lab, pad_idx)
    l_act, ac, at, _ = G.RU.cal_performance(act.view(-1, C), tgt.contiguous().view(-1), pad_idx, exclude_class_idx=47,
                                            reference=first, target_ref=tgt[:, 0])
    od = G.RU.normalize_duration(out["duration"], dur_mask)
    l_dur = torch.sum(crit(od, target_dur * dur_mask)) / torch.sum(dur_mask)
    return dict(loss_action=l_act, loss_dur=l_dur, loss=l_act + l_dur, act_correct=ac, act_total=at)


def run_ref(model, inputs, depth, mode):
    holder = {}
    hook = model.fuser.register_forward_hook(lambda m, i, o: holder.__setitem__("fused", o[0]))
    try:
        out = model(inputs, depth, mode)
    finally:
        hook.remove()
    return out, holder["fused"]


def case(tag, H, B, S, n_class, seed):
    model, pad_idx, names_shapes, args = build(H, n_class)
    batch = G.t_batch(synth.make_batch(B, S, n_class, pad_idx, seed, depth_hw=DEPTH_HW))
    feats, depth, lab, dur, tgt = batch
    meta = dict(tag=tag, H=H, B=B, S=S, n_class=n_class, pad_idx=pad_idx, n_dec=N_DEC, seed=seed, n_head=8, n_query=8,
                depth_hw=list(DEPTH_HW), variant="afft", lr=LR, wd=WD, max_pos_len=int(args.max_pos_len),
                input_dim=int(args.input_dim), n_encoder_layer=int(args.n_encoder_layer), torch=torch.__version__)
    fx = {"param_names": json.dumps([n for n, _ in names_shapes]),
          "param_shapes": json.dumps([list(s) for _, s in names_shapes]),
          "state_keys": json.dumps(list(model.state_dict().keys())),
          "state_keys_seg": json.dumps(list(_new(H, n_class, seg=True)[0].state_dict().keys())),
          "init_sums": init_checksums(H, n_class)}
    model.eval()
    with torch.no_grad():
        vout, vfused = run_ref(model, feats, depth, "val")
    assert sorted(vout) == ["action", "duration"]
    model.train()
    out, fused = run_ref(model, (feats, lab), depth, "train")
    assert sorted(out) == ["action", "duration"]
    res = ref_losses(out, lab, dur, tgt, pad_idx)
    res["loss"].backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    live = list(grads)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.grad is not None], lr=LR, weight_decay=WD)
    opt.step()
    post = {n: p.detach().clone() for n, p in model.named_parameters() if n in grads}
    fx.update({
        "meta": json.dumps(meta),
        "out_action": out["action"].detach().numpy(), "out_duration": out["duration"].detach().numpy(),
        "fused": fused.detach().numpy(),
        "val_action": vout["action"].numpy(), "val_duration": vout["duration"].numpy(), "val_fused": vfused.numpy(),
        "losses": np.array([0.0] + [float(res[k].detach()) for k in ("loss_action", "loss_dur", "loss")], np.float64),
        "counts": np.array([0, 0, res["act_correct"], res["act_total"]], np.int64),
        "live_names": json.dumps(live),
        "grad_stats": np.stack([G.stats(grads[n]) for n in live]),
        "post_stats": np.stack([G.stats(post[n]) for n in live]),
    })
    for n in ("fuser.modality_token", "fuser.norm.weight", "depth_layernorm.weight", "input_embed.bias", "fc.bias",
              "fc_len.weight"):
        fx["grad::" + n] = grads[n].numpy()
    # ---- restatement cross-check --------------------------------------------------------------------------------------
    from tests.helpers import fixture_params
    p0 = fixture_params(dict(param_names=[n for n, _ in names_shapes], param_shapes=[list(s) for _, s in names_shapes]))
    tr = AO.Trainer(p0, pad_idx, 8, 8, lr=LR, wd=WD)
    with torch.no_grad():
        vo, vaux = AO.forward(tr.p, feats, depth, "val", pad_idx, 8, 8)
    for k in ("action", "duration"):
        G.check_close(f"{tag}/val/{k}", vo[k], vout[k])
    G.check_close(f"{tag}/val/fused", vaux["fused"], vfused)
    ores, oout, oaux = tr.step(batch, apply=True)
    for k in ("action", "duration"):
        G.check_close(f"{tag}/out/{k}", oout[k], out[k])
    G.check_close(f"{tag}/fused", oaux["fused"], fused)
    G.check_close(f"{tag}/pooled", oaux["pooled"],
                  torch.nn.functional.adaptive_avg_pool1d(fused.detach().permute(0, 2, 1), 8).permute(0, 2, 1))
    for k in ("loss_action", "loss_dur", "loss"):
        G.check_close(f"{tag}/{k}", ores[k], res[k])
    for k, j in (("act_correct", 2), ("act_total", 3)):
        assert int(ores[k]) == int(fx["counts"][j]), (tag, k)
    assert sorted(live) == sorted(n for n, q in tr.p.items() if q.grad is not None), "live set"
    assert sorted(live) == sorted(n for n, _ in names_shapes if AO.is_live(n)), "live set against the prefix rule"
    for n in live:
        g = grads[n]
        G.check_close(f"{tag}/grad/{n}", tr.p[n].grad, g, tol=5e-5 * max(1.0, float(g.abs().max())))
        keep = g.abs() > 1e-6 * max(1.0, float(g.abs().max()))
        G.check_close(f"{tag}/post/{n}", tr.p[n].detach()[keep], post[n][keep], tol=1e-5)
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **fx)
    print(f"[golden-afft] {tag}: loss={float(res['loss']):.6f} live={len(live)} -> {os.path.getsize(path)/1024:.1f} KB")


if __name__ == "__main__":
    case("afft_tiny", 64, 2, 6, 17, 5)
    case("afft_cfg2", 128, 8, 16, 17, 9)
    case("afft_odd", 136, 3, 37, 122, 13)
