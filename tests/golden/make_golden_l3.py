#!/usr/bin/env python3
"""Generates tests/golden/l3_*.npz by IMPORTING THE REFERENCE's L3 query model (model/futr_unsupervised_temp3.py) and the
loss functions its loop calls (utils.py, train/train_unsupervised.py) on CPU -- build container only.

Same conventions as make_golden_unsup.py: hash-generated inputs / analytic parameters (oracle/synth.py), the module in eval()
state with mode='train' (RNG-free: dropout of the PositionalEncoding and of the decoder is off), the reference's own loss
functions called in the order of train/train_unsupervised.py:300-362, backward, one torch AdamW step.  Every value is
cross-checked against tests/l3_oracle.py (float64) and the script aborts on a mismatch.  A step is taken at the warm-up factors
wf in {0, 1/30, 1}: the forward is the same, the total and the gradients differ.

The seed of a case is the first one, counting up from its start, at which the float64 oracle's gap between the two largest
logits of EVERY row -- seg and l3 -- exceeds 4 x the case's logit tolerance (8 x the float32 restatement's error): the GPU
tests compare flags and m exactly, with no row left out."""
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
import make_golden as G  # noqa: E402   (helpers: stats, check_close, t_batch)
import utils as RU  # noqa: E402
import train_unsupervised as TU  # noqa: E402
from tests import l3_oracle as LO, l3_cases as SC  # noqa: E402

M = importlib.import_module("model.futr_unsupervised_temp3")
WFS = SC.WFS


def build(c):
    args = parser.parse_args([])
    args.hidden_dim, args.n_head, args.n_decoder_layer, args.n_query = c["H"], c["n_head"], c["n_dec"], 8
    model = M.FUTR(c["n_class"], c["H"], device=torch.device("cpu"), args=args, src_pad_idx=SC.pad_idx(c), n_query=8,
                   n_head=c["n_head"], num_encoder_layers=args.n_encoder_layer, num_decoder_layers=c["n_dec"],
                   query_num=c["query_num"])
    names_shapes = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    state = synth.fill_state(names_shapes)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[n]))
    return model, names_shapes


def ref_losses(out, batch, pad_idx, wf):
    """the reference's functions in the order of train_unsupervised.py:300-362"""
    feats, lab, dur, tgt, ql = batch
    l3 = out["l3"]
    B, T, C = l3.size()
    Lc = RU.temporal_cluster_loss(l3, TU.get_cluster_intervals(ql))
    L3, n3c, n3t, l3_correct = RU.cal_performance_focal(l3.view(-1, C), ql.view(-1), 47, 48, reference=None, target_ref=None)
    seg = out["seg"]
    K = seg.size(-1)
    Lseg, sc, st, l2_correct = RU.cal_performance(seg.view(-1, K), lab.view(-1), pad_idx, exclude_class_idx=None,
                                                  reference=None, target_ref=None)
    act = out["action"]
    first = TU.get_last_non_padding_labels(lab, pad_idx)
    Lact, ac, at, _ = RU.cal_performance(act.view(-1, K), tgt.contiguous().view(-1), pad_idx, exclude_class_idx=None,
                                         reference=first, target_ref=tgt[:, 0])
    mask = (dur != pad_idx).long()
    od = RU.normalize_duration(out["duration"], mask)
    Ldur = torch.sum(torch.nn.MSELoss(reduction="none")(od, dur * mask * mask)) / torch.sum(mask)
    how = torch.where(l3_correct & l2_correct, torch.tensor(1.0), torch.tensor(5.0))
    total = (1 - 1 / how.mean()) * ((1 - wf) * L3 + wf * Lc) + (1 / how.mean()) * (Lact + Ldur + Lseg)
    return dict(L3=L3, Lc=Lc, Lseg=Lseg, Lact=Lact, Ldur=Ldur, m=how.mean(), total=total, l3_correct=l3_correct,
                l2_correct=l2_correct, counts=[sc, st, ac, at], l3_counts=[n3c, n3t])


def admissible(c, seed, p0):
    """the tie condition on the float64 oracle's logits, against 4 x the case's logit tolerances"""
    out64, tol = SC.forward_tolerances(c, SC.batch(c, seed), p0)
    return SC.tie_margin(out64, tol) > 1.0, out64


def case(c):
    model, names_shapes = build(c)
    model.eval()
    p0 = {n: torch.from_numpy(synth.fill_value(n, s, j)) for j, (n, s) in enumerate(names_shapes)}
    seed = c["seed"]
    ok, out64 = admissible(c, seed, p0)
    while not ok:
        seed += 1
        ok, out64 = admissible(c, seed, p0)
    batch = SC.relabel(c, SC.batch(c, seed), out64)
    feats, lab, dur, tgt, ql = batch
    pad_idx, S = SC.pad_idx(c), c["S"]
    full = c["tag"] == "l3_tiny"
    fx = {"param_names": json.dumps([n for n, _ in names_shapes]),
          "param_shapes": json.dumps([list(s) for _, s in names_shapes]),
          "state_keys": json.dumps(list(model.state_dict().keys())),
          "state_shapes": json.dumps([list(v.shape) for v in model.state_dict().values()])}
    live = None
    for wi, wf in enumerate(WFS):
        model.zero_grad(set_to_none=True)
        out = model((feats, lab), ql)
        res = ref_losses(out, batch, pad_idx, wf)
        res["total"].backward()
        grads = {n: p.grad for n, p in model.named_parameters()}
        live_w = [n for n, g in grads.items() if g is not None]
        live = live if live is not None else live_w
        assert live == live_w and sorted(live) == sorted(n for n, _ in names_shapes if n.startswith(LO.LIVE_PREFIXES))
        # ---- oracle cross-check
        oout, ores, ograds = LO.step(p0, batch, pad_idx, wf, c["n_head"], c["n_dec"], 8)
        for k in ("action", "duration", "seg", "l3"):
            G.check_close(f"{c['tag']}/out/{k}", oout[k], out[k])
        for k in ("L3", "Lc", "Lseg", "Lact", "Ldur", "total"):
            G.check_close(f"{c['tag']}/wf{wi}/{k}", ores[k], res[k])
        assert float(ores["m"]) == float(res["m"])
        assert torch.equal(ores["l3_correct"], res["l3_correct"]) and torch.equal(ores["l2_correct"], res["l2_correct"])
        assert ores["counts"] == list(res["counts"]) and ores["l3_counts"] == list(res["l3_counts"]), (ores["counts"], res["counts"])
        for n in live:
            G.check_close(f"{c['tag']}/wf{wi}/grad/{n}", ograds[n], grads[n], tol=5e-5 * max(1.0, float(grads[n].abs().max())))
        assert all(ograds[n] is None or float(ograds[n].abs().max()) == 0.0 for n in ograds if n not in live)
        if wi == 0:
            for k in ("action", "duration", "seg", "l3"):
                fx["out_" + k] = out[k].detach().numpy() if full or k in ("action", "duration") else G.stats(out[k])
            fx["l3_correct"], fx["l2_correct"] = res["l3_correct"].numpy(), res["l2_correct"].numpy()
            fx["counts"] = np.array(list(res["counts"]) + list(res["l3_counts"]), np.int64)
            fx["m"] = np.array(float(res["m"]), np.float32)
        fx[f"losses_wf{wi}"] = np.array([float(res[k].detach()) for k in ("L3", "Lc", "Lseg", "Lact", "Ldur", "total")], np.float64)
        fx[f"grad_stats_wf{wi}"] = np.stack([G.stats(grads[n]) for n in live])
        if full and wi == 1:                                           # full gradients at wf = 1/30, statistics at the others
            for n in live:
                g = grads[n]
                fx[f"grad_wf{wi}::" + n] = (g[0, :S] if n == "pos_embedding" else g).numpy()
        if wi == 1:                                                    # one AdamW step at wf = 1/30 (main_darai.py:135)
            opt = torch.optim.AdamW(model.parameters(), c["lr"], weight_decay=c["wd"])
            opt.step()
            post = dict(model.named_parameters())
            fx["post_stats"] = np.stack([G.stats(post[n]) for n in live])
            dead = [n for n in post if n not in live]
            fx["dead_unchanged"] = np.array([bool(torch.equal(post[n].detach(), p0[n])) for n in dead])
            with torch.no_grad():
                for n, p in model.named_parameters():
                    p.copy_(p0[n])
    with torch.no_grad():
        test = model(feats, ql, mode="test")
    otest, _ = LO.forward({n: v.double() for n, v in p0.items()}, feats, "test", pad_idx, c["n_head"], c["n_dec"], 8)
    for k in ("action", "duration", "seg", "l3"):
        G.check_close(f"{c['tag']}/test/{k}", otest[k], test[k])
        fx["test_" + k] = test[k].numpy() if full or k in ("action", "duration") else G.stats(test[k])
    fx["past_label"], fx["query_label"] = lab.numpy(), ql.numpy()
    fx["live_names"] = json.dumps(live)
    fx["meta"] = json.dumps(dict(c, seed=seed, pad_idx=pad_idx, wfs=list(WFS), torch=torch.__version__))
    path = os.path.join(HERE, f"{c['tag']}.npz")
    np.savez_compressed(path, **fx)
    print(f"[golden] {c['tag']}: seed {seed} total(wf=1/30)={fx['losses_wf1'][5]:.6f} m={float(fx['m'])} live={len(live)} -> "
          f"{os.path.getsize(path) / 1024:.1f} KB")


def no_dropout(model):
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0


class NoSched:
    def step(self):
        pass


def case_train_loop(tag, c, epochs=3):
    """The reference's own train() (train_unsupervised.py:208) over `epochs` epochs of a tiny batch list (wf = 0, 1/30, 2/30),
    dropout p = 0, torch AdamW, a no-op scheduler, its validate() after every epoch and its checkpoint writes.  The float64
    oracle runs the same steps (SC.loop_tie_margins): the script aborts unless the tie condition holds at every step and every
    validation forward and the oracle's final parameters equal the reference's."""
    import contextlib
    import io
    import tempfile
    seed = c["seed"]
    train, val = SC.loop_data(c, seed)
    crit = torch.nn.MSELoss(reduction="none")

    def run(val):
        model, names_shapes = build(c)
        no_dropout(model)
        args = model.args
        args.epochs = epochs
        buf = io.StringIO()
        with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(buf):
            TU.train(args, model, train, torch.optim.AdamW(model.parameters(), c["lr"], weight_decay=c["wd"]), NoSched(), crit,
                     d, SC.pad_idx(c), torch.device("cpu"), val, seed)
            files = sorted(os.listdir(d))
            keys = list(torch.load(os.path.join(d, files[0]), weights_only=True).keys()) if files else []
        return model, names_shapes, buf.getvalue(), files, keys
    # With the analytic fill the trained model anticipates none of the synthetic future labels and the loop saves a checkpoint
    # only when a validation accuracy rises above 0: a first run (training does not read the validation batch) tells which
    # classes the trained model anticipates, and the validation batch's future labels are set to them where the decision is
    # clear (top-two gap > 0.01) and the class is not padding.
    m0, _, _, _, _ = run(val)
    with torch.no_grad():
        act = m0((val[0][0], val[0][1]), val[0][4])["action"]
    top = act.topk(2, -1)
    for b in range(act.shape[0]):
        for q in range(act.shape[1]):
            k = int(top.indices[b, q, 0])
            if int(val[0][3][b, q]) != SC.pad_idx(c) and float(top.values[b, q, 0] - top.values[b, q, 1]) > 1e-2:
                val[0][3][b, q] = k
    model, names_shapes, out, files, keys = run(val)
    with contextlib.redirect_stdout(io.StringIO()):
        vres = TU.validate(model, val, crit, SC.pad_idx(c), torch.device("cpu"))
    live = [n for n, p in model.named_parameters() if p.grad is not None]
    fx = {"meta": json.dumps(dict(c, tag=tag, pad_idx=SC.pad_idx(c), epochs=epochs, torch=torch.__version__)),
          "param_names": json.dumps([n for n, _ in names_shapes]),
          "param_shapes": json.dumps([list(s) for _, s in names_shapes]),
          "live_names": json.dumps(live), "post_stats": np.stack([G.stats(p) for n, p in model.named_parameters() if n in live]),
          "val_result": np.array([float(x) for x in vres], np.float64), "ckpt_files": json.dumps(files),
          "ckpt_keys": json.dumps(keys), "stdout": json.dumps(out), "val_target": val[0][3].numpy()}
    assert files, "the loop saved no checkpoint: pick other batches"
    # the float64 oracle runs the same six steps: the tie condition at every step and validation forward, and its final
    # parameters against the reference's
    p0 = {n: torch.from_numpy(synth.fill_value(n, s, j)) for j, (n, s) in enumerate(names_shapes)}
    margins, pfin = SC.loop_tie_margins(c, train, val, p0, epochs)
    for what, mg in margins:
        if not mg > 1.0:
            raise SystemExit(f"{tag}: {what}: a row's top-two logit gap is within 4 x the logit tolerance (margin {mg}): pick another seed")
    # (a softmax is blind to a shift of all its scores, and normalize_duration to a shift of all durations: the key third of
    #  every in_proj_bias and fc_len.bias have a zero true gradient, the reference's float32 holds rounding noise there, and
    #  AdamW moves such an element by up to lr per step in any implementation -- those elements are bounded by steps * lr)
    H, steps = c["H"], len(margins) - epochs
    for n, q in model.named_parameters():
        a, b = pfin[n].detach(), q.detach().double()
        if n.endswith("in_proj_bias"):
            G.check_close(f"{tag}/final/{n}[k]", a[H:2 * H], b[H:2 * H], tol=steps * c["lr"])
            a, b = torch.cat([a[:H], a[2 * H:]]), torch.cat([b[:H], b[2 * H:]])
        G.check_close(f"{tag}/final/{n}", a, b, tol=steps * c["lr"] if n == SC.ZERO_GRAD else 5e-5)
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **fx)
    print(f"[golden] {tag}: val={fx['val_result'].round(4).tolist()} ckpts={files} -> {os.path.getsize(path) / 1024:.1f} KB")
    print(out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    if "--loop-only" not in sys.argv:
        for c in SC.STEP_CASES:
            case(c)
    case_train_loop("l3_train_loop", SC.STEP_BY_TAG["l3_tiny"])
