"""Drop-in for the reference's ``train/train_unimodal.py`` (``from train_unimodal import train``, main_nturgbd.py:32):
``train(args, model, train_loader, optimizer, scheduler, criterion, model_save_path, pad_idx, device, val_loader, seed)``
and ``validate(model, val_loader, criterion, pad_idx, device)`` with the reference's signatures, skip rules, loss
composition, prints and checkpoint names, driving either unimodal baseline (r3d_amd.model.rnn.FUTR or
r3d_amd.model.cnn.FUTR; the shape check dispatches on the model, everything else is shared).  Each batch is one replay of
the fused step (forward + 3 losses + backward + AdamW, train_common.GraphedSteps) with no device->host sync;
epoch statistics are read back once per epoch.

It is train_proposed_depth's loop except where the reference's differs (each can be checked against the cited line):
  * the model is called without depth, ``model(inputs)`` (:186); the 5-tuple's depth tensor is never read or uploaded;
  * the excluded class is 120 (NTU's UNDEFINED) for the seg, action and validation losses (:102,198,212);
  * the per-epoch ``seg loss / seg acc`` line is printed (:245-248);
  * ``model.train()`` runs after validate() (:270), so a later epoch trains in train mode (there is no dropout anyway);
  * validate() calls the model in train mode with the (features, labels) tuple (:91).
Kept from the shared loop: batches with fewer than 8 clips are skipped (:163), the epoch averages divide by (i + 1) (:234),
validate() compares the normalised duration with the UNMASKED target and skips the seg loss (:86-113).  Multi-rank
torch.distributed runs are refused (the reference's nn.DataParallel wrapper, main_nturgbd.py:131, is unwrapped).

Build-defined addition: ``--supcon_weight W`` (default 0.0: none of the following is launched) adds W * SupConLoss(
temperature=args.temperature, normalize=True, ignore_index=pad_idx) over the B * S rows of ``outputs['supcon']`` with the
labels ``past_label.view(-1)`` -- the use main_nturgbd.py:137 prepares and the reference's loop leaves commented out --
to the step's loss, inside the step (the engine's losses / backward; the CNN model's rows are x, hidden <= 256); the epoch's ``Loss`` includes it and one
``supcon loss`` line follows the ``seg loss`` line.  validate() is unchanged.  ``--wide_supcon`` runs the term through the
kernel's wide route, which admits it at hidden > 256 (RNN with --wide_rnn, and CNN, up to 1024).
"""
import torch
import torch.distributed as dist

from .model.rnn import FUTR
from .model.cnn import FUTR as FUTRCnn
from .optim import FlatAdamW
from .engine_rnn import check_rnn_shape
from .engine_cnn import check_cnn_shape
from . import train_common
from .train_common import (GraphedSteps, adamw_hyper, get_last_non_padding_labels, print_epoch, save_best,  # noqa: F401
                           unwrap, weighted_accuracy)


def _unwrap(model):
    return unwrap(model, (FUTR, FUTRCnn), "r3d_amd.train_unimodal drives r3d_amd.model.rnn.FUTR or r3d_amd.model.cnn.FUTR")


def _check_shape(core, erank_weight, supcon_weight=0.0, wide_supcon=False):
    """The model's own admission rule, on the host, before anything is enqueued."""
    if isinstance(core, FUTRCnn):
        check_cnn_shape(core.hidden_dim, core.n_query, core.n_class, erank_weight, input_dim=core.input_embed.in_features)
    else:
        check_rnn_shape(core.hidden_dim, core.n_query, erank_weight, wide=getattr(core, "r3d_wide_rnn", False),
                        supcon_weight=supcon_weight, wide_supcon=wide_supcon)


def _to_dev(data, device):
    """(features, past_label, trans_dur_future, trans_future_target) on the device; the depth tensor stays where it is."""
    features, _depth, past_label, trans_dur_future, trans_future_target = data
    return (features.to(device=device, dtype=torch.float32).contiguous(), past_label.to(device).long().contiguous(),
            trans_dur_future.to(device=device, dtype=torch.float32).contiguous(),
            trans_future_target.to(device).long().contiguous())


class _UnimodalSteps(GraphedSteps):
    """GraphedSteps over the 4-tuple (features, past_label, trans_dur_future, trans_future_target): no depth buffer.
    acc_sc: the epoch's sum of the supervised contrastive loss (--supcon_weight > 0), accumulated inside the step."""

    def __init__(self, eng, acc_loss, acc_cnt, acc_sc=None, graph=True):
        super().__init__(eng, acc_loss, acc_cnt, graph)
        self.acc_sc = acc_sc

    def _enqueue(self, buf, lr, hyper, training):
        eng = self.eng
        feats, lab, dur, tgt = buf
        wd, betas, eps = hyper
        eng.forward(feats, None, lab, "train", training=training)
        loss, counts = eng.losses(lab, tgt, dur, tick=True)
        eng.backward()
        eng.adamw(lr, wd, betas=betas, eps=eps, ticked=True)
        self.acc_loss += loss
        self.acc_cnt += counts
        if eng.supcon_weight and self.acc_sc is not None:
            self.acc_sc += eng.last["w"].sc_loss


def validate(model, val_loader, criterion, pad_idx, device):
    def forward(eng, batch):                                                                             # (:91)
        return (eng.forward(batch[0], None, batch[1], "train", training=False, need_grad=False),) + batch[1:]
    return train_common.validate(model, _unwrap(model), val_loader, pad_idx, _to_dev, forward)


def train(args, model, train_loader, optimizer, scheduler, criterion, model_save_path, pad_idx, device, val_loader, seed):
    core = _unwrap(model)
    wide_supcon = bool(getattr(args, "wide_supcon", False))
    _check_shape(core, float(getattr(args, "erank_weight", 0.0) or 0.0), float(getattr(args, "supcon_weight", 0.0) or 0.0),
                 wide_supcon)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("r3d_amd.train_unimodal trains its model on one GPU; multi-rank torch.distributed "
                                  "runs of it are not supported")
    model.to(device)
    model.train()
    eng = core.engine()
    # --supcon_weight: the supervised contrastive term on the 'supcon' output, part of every step (graphed or eager)
    eng.wide_supcon = wide_supcon          # (before the weight: the RNN engine's setter checks the shape against it)
    eng.supcon_weight = float(getattr(args, "supcon_weight", 0.0) or 0.0)
    eng.supcon_temperature = float(getattr(args, "temperature", 0.07))
    min_batch = getattr(args, "min_batch", 8)
    print("Training Start")
    best_val_acc = 0
    best_weight_acc = 0
    acc_loss = torch.zeros(4, dtype=torch.float64, device=eng.device)
    acc_cnt = torch.zeros(4, dtype=torch.int64, device=eng.device)
    acc_sc = torch.zeros(1, dtype=torch.float64, device=eng.device)
    steps = _UnimodalSteps(eng, acc_loss, acc_cnt, acc_sc, graph=getattr(args, "graph_steps", True))
    for epoch in range(args.epochs):
        acc_loss.zero_()
        acc_cnt.zero_()
        acc_sc.zero_()
        i = -1
        for i, data in enumerate(train_loader):
            if data is None:
                continue
            if len(data[0]) < min_batch:
                continue
            features, past_label, trans_dur_future, trans_future_target = _to_dev(data, eng.device)
            g = optimizer.param_groups[0]
            if isinstance(optimizer, FlatAdamW):
                steps.step([features, past_label, trans_dur_future, trans_future_target], g["lr"], adamw_hyper(g),
                           model.training)
                continue
            eng.forward(features, None, past_label, "train", training=model.training)    # any other torch optimiser:
            loss, counts = eng.losses(past_label, trans_future_target, trans_dur_future)
            eng.backward()
            eng.arena.attach_grads(core.named_parameters())                              # expose the arena gradients to it
            optimizer.step()
            acc_loss += loss
            acc_cnt += counts
            if eng.supcon_weight:
                acc_sc += eng.last["w"].sc_loss
        print_epoch(args, epoch, i, acc_loss, acc_cnt, acc_sc if eng.supcon_weight else None, seg_line=args.seg)
        scheduler.step()
        val_loss, val_acc, weight_acc = validate(model, val_loader, criterion, pad_idx, device)
        if val_acc > best_val_acc or weight_acc > best_weight_acc:
            best_val_acc, best_weight_acc = val_acc, weight_acc
            save_best(model, model_save_path, seed, epoch, val_loss)
        model.train()
    return model
