"""Drop-in for the reference's ``train/train_tcn.py``: ``train(args, model, train_loader, val_loader, optimizer, scheduler,
criterion, model_save_path, pad_idx, device)`` and ``validate(model, val_loader, pad_idx, device, model_save_path, epoch,
best_accuracy)`` with the reference's signatures, prints and checkpoint writes, driving r3d_amd.model.tcn.MustafaNet1DTCN.
With ``torch.optim.AdamW`` or ``FlatAdamW`` each batch is one replay of the fused step (forward + loss + backward + AdamW,
one hipGraph per batch shape) with no device->host sync; epoch statistics are read back once per epoch.

The reference's file cannot run as it stands: ``cal_performance`` returns four values and both loops unpack three
(train_tcn.py:27,84).  This loop follows the unambiguous reading (the fourth value, ``l2_correct``, is unused).  Kept from the
reference, each checkable against the cited line:
  * batches are 5-tuples ``(features, past_label, trans_dur_future, trans_future_target, _)`` (:14,66); only the features
    and the future targets are read; no batch is skipped for being small;
  * the loss is ``cal_performance(output.view(-1, C), target.view(-1), pad_idx)``: the mean over ALL rows (:84);
  * the epoch averages divide by (i + 1) (:97,100); accuracy is n_correct / n_total over the epoch (:99);
  * ``validate`` writes ``checkpoint{epoch}.ckpt`` on a strict accuracy improvement and creates the directory only
    afterwards (:43-50); it leaves the model in eval(): the reference never switches back, so from the second epoch on
    the loop trains with dropout off (:7,105).
"""
import os

import torch

from .model.tcn import MustafaNet1DTCN
from .optim import FlatAdamW
from .opts import refuse_supcon_weight
from .train_common import GraphedSteps, adamw_hyper, unwrap


def _unwrap(model):
    return unwrap(model, MustafaNet1DTCN, "r3d_amd.train_tcn drives r3d_amd.model.tcn.MustafaNet1DTCN")


def _to_dev(data, device):
    features, _past_label, _dur, trans_future_target, _ = data
    return (features.to(device=device, dtype=torch.float32).contiguous(), trans_future_target.to(device).long().contiguous())


class _TcnSteps(GraphedSteps):
    """GraphedSteps over the pair (features, trans_future_target)."""

    def __init__(self, eng, acc_loss, acc_cnt, pad_idx=None, graph=True):
        super().__init__(eng, acc_loss, acc_cnt, graph)
        self.pad_idx = pad_idx

    def _enqueue(self, buf, lr, hyper, training):
        feats, tgt = buf
        wd, betas, eps = hyper
        loss, counts = self.eng.train_step(feats, tgt, self.pad_idx, lr, wd, training=training, betas=betas, eps=eps)
        self.acc_loss += loss
        self.acc_cnt += counts


def validate(model, val_loader, pad_idx, device, model_save_path, epoch, best_accuracy):
    core = _unwrap(model)
    model.eval()
    eng = core.engine()
    acc_loss = torch.zeros(4, dtype=torch.float64, device=eng.device)
    acc_cnt = torch.zeros(4, dtype=torch.int64, device=eng.device)
    i = -1
    with torch.no_grad():
        for i, data in enumerate(val_loader):
            features, target = _to_dev(data, eng.device)
            eng.forward(features, training=False, need_grad=False)
            loss, counts = eng.losses(target, pad_idx, with_grad=False)
            acc_loss += loss
            acc_cnt += counts
        lsum, csum = acc_loss.cpu(), acc_cnt.cpu()                  # the single device->host read of the validation
        accuracy = int(csum[2]) / int(csum[3])
        epoch_loss_class = float(lsum[1]) / (i + 1)
        print("Validation Acc :%.3f" % accuracy, "CE loss :%.3f" % epoch_loss_class)
        save_path = os.path.join(model_save_path)
        if accuracy > best_accuracy:
            best_accuracy = accuracy
            save_file = os.path.join(save_path, "checkpoint" + str(epoch) + ".ckpt")
            torch.save(model.state_dict(), save_file)
            print("saved --- epoch ", epoch)
        if not os.path.exists(save_path):
            os.makedirs(save_path)
    return best_accuracy


def train(args, model, train_loader, val_loader, optimizer, scheduler, criterion, model_save_path, pad_idx, device):
    refuse_supcon_weight(args, "train_tcn")
    core = _unwrap(model)
    model.to(device)
    model.train()
    eng = core.engine()
    print("Training Start")
    best_accuracy = 0
    acc_loss = torch.zeros(4, dtype=torch.float64, device=eng.device)
    acc_cnt = torch.zeros(4, dtype=torch.int64, device=eng.device)
    fused_opt = isinstance(optimizer, FlatAdamW) or type(optimizer) is torch.optim.AdamW
    steps = _TcnSteps(eng, acc_loss, acc_cnt, pad_idx=pad_idx, graph=getattr(args, "graph_steps", True))
    for epoch in range(args.epochs):
        acc_loss.zero_()
        acc_cnt.zero_()
        i = -1
        for i, data in enumerate(train_loader):
            features, target = _to_dev(data, eng.device)
            g = optimizer.param_groups[0]
            if fused_opt and len(optimizer.param_groups) == 1 and not g.get("amsgrad", False) and not g.get("maximize", False):
                steps.step([features, target], g["lr"], adamw_hyper(g), model.training)
                continue
            optimizer.zero_grad()                                   # any other optimiser: expose the arena gradients to it
            eng.forward(features, training=model.training)
            loss, counts = eng.losses(target, pad_idx)
            eng.backward()
            eng.arena.attach_grads(core.named_parameters())
            optimizer.step()
            acc_loss += loss
            acc_cnt += counts
        lsum, csum = acc_loss.cpu(), acc_cnt.cpu()                  # the single device->host read of the epoch
        epoch_loss = float(lsum[3]) / (i + 1)
        print("Epoch [", (epoch + 1), "/", args.epochs, "] Loss : %.3f" % epoch_loss)
        accuracy = int(csum[2]) / int(csum[3])
        print("Training Acc :%.3f" % accuracy, "CE loss :%.3f" % (float(lsum[1]) / (i + 1)))
        scheduler.step()
        best_accuracy = validate(model, val_loader, pad_idx, device, model_save_path, epoch, best_accuracy)
    return model
