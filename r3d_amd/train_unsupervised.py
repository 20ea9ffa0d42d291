"""Drop-in for the reference's ``train/train_unsupervised.py`` (``from train_unsupervised import train``, main_darai.py:40):
``train(args, model, train_loader, optimizer, scheduler, criterion, model_save_path, pad_idx, device, val_loader, seed)`` and
``validate(model, val_loader, criterion, pad_idx, device)`` with the reference's signatures, skip rule, loss composition, prints
and checkpoint names, driving r3d_amd.model.futr_unsupervised_temp3.FUTR -- the one model of the reference's L3 family whose
outputs this loop accepts.  Each batch is one replay of the fused step (forward + five losses + the mix + backward + AdamW,
engine_l3.L3Engine.train_step_graphed) with no device->host transfer; epoch statistics are read back once per epoch.

The loss (:300-362): L_c = temporal cluster loss and L_3 = focal loss (pad 47, excluded 48) on the l3 logits; L_seg through
cal_loss with exclude_class_idx None; L_act weighted, L_dur; m = mean over all rows of (l3_correct & l2_correct ? 1 : 5);
wf = get_warmup_factor(epoch, 0, 30, 60);  loss = (1 - 1/m)((1 - wf) L_3 + wf L_c) + (1/m)(L_act + L_dur + L_seg).
wf is written to a device scalar once per epoch, so a new epoch needs no new capture (the dropout state is part of the
graph key: one capture while the model trains with dropout, one after validate() has left it in eval()).

Kept from the reference: batches with fewer than 8 clips are skipped (:248); the epoch averages divide by (i + 1) (:388); the
``l3 loss / l3 acc`` line (:406); validate() calls the model in 'train' mode with the labels (:146), uses focal pad 48 (:157),
adds the UNWEIGHTED cal_loss action loss and no duration loss (:179,193-196); validate() leaves the model in eval(), and
train() never switches back, so dropout is off from the second epoch on; the checkpoint rule and file names (:413-425).
The reference raises a NameError with args.seg or args.anticipate off (:357,362 read l2_correct / loss / loss_dur
unconditionally): both are refused here with a ValueError that says so."""
import torch
import torch.distributed as dist

from .engine_l3 import VAL_L3_PAD
from .loss.temporal import get_cluster_intervals  # noqa: F401
from .model.futr_unsupervised_temp3 import FUTR
from .optim import FlatAdamW
from .train_common import save_best, unwrap
from . import ops


def get_warmup_factor(epoch, start_epoch, peak_epoch, end_epoch):
    """0 before start_epoch, rising linearly to 1 at peak_epoch, falling linearly to 0 at end_epoch, 0 after (:10-32)."""
    if epoch < start_epoch or epoch >= end_epoch:
        return 0.0
    if epoch < peak_epoch:
        return (epoch - start_epoch) / (peak_epoch - start_epoch)
    return 1.0 - (epoch - peak_epoch) / (end_epoch - peak_epoch)


def get_last_non_padding_labels(past_label, pad_value):
    """[B]: each clip's last label that is not pad_value (pad_value for a clip that is all padding) (:86-108)."""
    keep = past_label != pad_value
    S = past_label.shape[1]
    last = (keep * torch.arange(1, S + 1, device=past_label.device)).max(dim=1).values
    picked = past_label.gather(1, (last - 1).clamp_min(0).unsqueeze(1)).squeeze(1)
    return torch.where(last > 0, picked, torch.full_like(picked, pad_value))


def weighted_accuracy(pred, gold, pad_idx, t_n_labels, weight_same=1.0, weight_different=10.0):
    """(:67-84) ONE weight for the whole batch, from its first row: weight_different if gold[0] != t_n_labels[0]; every
    non-padded row counts with it, so the result is the plain accuracy over the non-padded rows (0 without any)."""
    arg = pred.max(1)[1]
    keep = gold.ne(pad_idx)
    weight = weight_different if bool(gold[0] != t_n_labels[0]) else weight_same
    n = int(keep.sum())
    return (weight * int((arg.eq(gold) & keep).sum())) / (weight * n) if n > 0 else 0


def _unwrap(model):
    return unwrap(model, FUTR, "r3d_amd.train_unsupervised drives r3d_amd.model.futr_unsupervised_temp3.FUTR")


def _to_dev(data, device):
    features, past_label, trans_dur_future, trans_future_target, query_label = data
    return (features.to(device=device, dtype=torch.float32).contiguous(), past_label.to(device).long().contiguous(),
            trans_dur_future.to(device=device, dtype=torch.float32).contiguous(),
            trans_future_target.to(device).long().contiguous(), query_label.to(device).long().contiguous())


def check_args(args):
    """The refusals of this loop, before anything is enqueued."""
    if not getattr(args, "seg", True) or not getattr(args, "anticipate", True):
        raise ValueError("train_unsupervised needs args.seg and args.anticipate on: the reference's loop reads l2_correct, loss "
                         "and loss_dur unconditionally (train_unsupervised.py:357,362) and raises a NameError without them")
    if float(getattr(args, "erank_weight", 0.0) or 0.0) != 0.0:
        raise ValueError("--erank_weight: the effective-rank penalty is defined on a fuser's token matrix; this model has none")
    if getattr(args, "measure_rank", False) or getattr(args, "erank_report", None):
        raise ValueError("--measure_rank / --erank_report: there is no fused token matrix to measure in this model")
    if float(getattr(args, "supcon_weight", 0.0) or 0.0) != 0.0:
        raise ValueError("--supcon_weight: this loop's auxiliary losses are the focal and temporal cluster losses; the "
                         "supervised contrastive term belongs to train_unimodal")
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError("train_unsupervised trains on one GPU: the cross-clip attention and m couple the clips of a batch, "
                         "so a data-parallel split would change the loss")


def validate(model, val_loader, criterion, pad_idx, device):
    core = _unwrap(model)
    model.eval()
    eng = core.engine()
    val_loss = 0.0
    val_class_correct = val_class_total = val_seg_correct = val_seg_total = total_l3 = total_l3_correct = 0
    val_weighted_accuracy_total = 0
    with torch.no_grad():
        for data in val_loader:
            features, past_label, dur, target, query_label = _to_dev(data, eng.device)
            out = eng.forward(features, past_label, "train", training=False, need_grad=False)           # (:146)
            w, K, B, S, Q = eng.last["w"], eng.K, features.shape[0], features.shape[1], eng.Q
            ops.focal_rows(w.l3log, query_label.view(-1), VAL_L3_PAD, exclude_idx=VAL_L3_PAD, ws=w.focal_ws, loss_out=w.loss_l3,
                           flags=w.l3_flags, counts=w.l3_counts)                                          # (:157)
            l3v, c3 = w.loss_l3.clone(), w.l3_counts.clone()
            # cal_loss on the seg rows, then on the action rows (the loss launch's frame-row unit with the Q action rows of
            # each clip as its frames: the unweighted CE + pad penalty, mean over all rows, :172-180)
            ops.losses_fwd_bwd_kseg(w.seg, w.actdur[:, :K], w.actdur[:, K:], K + 1, past_label, target, dur, B, S, Q, K, eng.Kseg,
                                    pad_idx, -1, w.loss3, w.counts, ws=w.loss_ws)
            segv, cs = w.loss3.clone(), w.counts.clone()
            ops.losses_fwd_bwd_kseg(w.actdur[:, :K], w.actdur[:, :K], w.actdur[:, K:], K + 1, target, target, dur, B, Q, Q, K, K,
                                    pad_idx, -1, w.loss3, w.counts, ws=w.loss_ws_q)
            lv = torch.cat([l3v, segv[:1], w.loss3[:1]]).cpu()                      # one read-back per validation batch
            cv = torch.cat([c3, cs[:2], w.counts[:2]]).cpu()
            val_loss += float(lv[0] + lv[1] + lv[2])
            total_l3_correct += int(cv[0])
            total_l3 += int(cv[1])
            val_seg_correct += int(cv[2])
            val_seg_total += int(cv[3])
            val_class_correct += int(cv[4])
            val_class_total += int(cv[5])
            val_weighted_accuracy_total += weighted_accuracy(
                out["action"].reshape(-1, K).cpu(), target.view(-1).cpu(), pad_idx,
                get_last_non_padding_labels(past_label, pad_idx).cpu())
    val_loss /= len(val_loader)
    l3_accuracy = total_l3_correct / total_l3 if total_l3 else 0
    val_accuracy = val_class_correct / val_class_total if val_class_total else 0
    val_seg_accuracy = val_seg_correct / val_seg_total if val_seg_total else 0
    val_weighted_accuracy = val_weighted_accuracy_total / len(val_loader)
    print(f"Validation Loss: {val_loss:.3f}, l3 accuracy: {l3_accuracy}, Class Accuracy: {val_accuracy:.3f}, Segmentation Accuracy: "
          f"{val_seg_accuracy:.3f}, Weighted Accuracy: {val_weighted_accuracy:.3f}")
    return val_loss, val_accuracy, val_weighted_accuracy


def train(args, model, train_loader, optimizer, scheduler, criterion, model_save_path, pad_idx, device, val_loader, seed):
    core = _unwrap(model)
    check_args(args)
    model.to(device)
    model.train()
    eng = core.engine()
    print("Training Start")
    best_val_acc = 0
    best_weight_acc = 0
    acc = (torch.zeros(6, dtype=torch.float64, device=eng.device), torch.zeros(6, dtype=torch.int64, device=eng.device))
    graph_steps = bool(getattr(args, "graph_steps", True))
    for epoch in range(args.epochs):
        acc[0].zero_()
        acc[1].zero_()
        wf = get_warmup_factor(epoch, start_epoch=0, peak_epoch=30, end_epoch=60)
        eng.set_wf(wf)                                              # once per epoch, as the learning rate: no new capture
        i = -1
        for i, data in enumerate(train_loader):
            if len(data[0]) < 8:                                    # (:248)
                continue
            batch = _to_dev(data, eng.device)
            g = optimizer.param_groups[0]
            if isinstance(optimizer, FlatAdamW):
                step = eng.train_step_graphed if graph_steps else eng.train_step
                step(*batch, g["lr"], g["weight_decay"], wf, model.training, tuple(g["betas"]), g["eps"], acc)
                continue
            eng.forward(batch[0], batch[1], "train", training=model.training)       # any other torch optimiser
            out = eng.losses(batch[1], batch[3], batch[2], batch[4])
            eng.backward()
            eng.arena.attach_grads(core.named_parameters())
            optimizer.step()
            acc[0][0:1] += out[0][4:5]
            acc[0][1:2] += out[2]
            acc[0][2:5] += out[1][:3]
            acc[0][5:6] += out[3]
            acc[1][:4] += out[4]
            acc[1][4:] += out[5]
        lsum, csum = acc[0].cpu(), acc[1].cpu()                     # the single device->host read of the epoch
        denom = i + 1                                               # the reference divides by (i + 1), skipped or not
        avg = lambda k: float(lsum[k]) / denom if denom else 0.0    # noqa: E731
        print("Epoch [", (epoch + 1), "/", args.epochs, "] Loss : %.3f" % avg(0))
        accuracy = int(csum[2]) / int(csum[3]) if int(csum[3]) else 0.0
        print("Training Acc :%.3f" % accuracy, "CE loss :%.3f" % avg(3))
        if args.task == "long":
            print("dur loss: %.5f" % avg(4))
        acc_seg = int(csum[0]) / int(csum[1]) if int(csum[1]) else 0.0
        print("seg loss :%.3f" % avg(2), ", seg acc : %.5f" % acc_seg)
        acc_l3 = int(csum[4]) / int(csum[5]) if int(csum[5]) else 0.0
        print("l3 loss :%.3f" % avg(1), ", l3 acc : %.5f" % acc_l3)
        scheduler.step()
        val_loss, val_acc, weight_acc = validate(model, val_loader, criterion, pad_idx, device)
        if val_acc > best_val_acc or weight_acc > best_weight_acc:
            best_val_acc, best_weight_acc = val_acc, weight_acc
            save_best(model, model_save_path, seed, epoch, val_loss)
    return model
