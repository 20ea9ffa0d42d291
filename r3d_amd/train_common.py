"""What the drop-in training loops (train_proposed_depth, train_unimodal, train_unsupervised, train_tcn) share: the
shape-keyed step runner that replays a fused training step as one hipGraph per batch shape, and the parts of the reference's
loops that its files repeat verbatim -- the accuracy helpers, validate()'s body, the epoch read-back with its prints and the
checkpoint writes.  Each loop file keeps what belongs to its own reference file (signatures, skip rules, batch layout, the
step's launch sequence) and imports this module; this module imports none of them, no model and no engine.
"""
import os

import torch


def unwrap(model, classes, message):
    """The model of one of `classes` inside any nesting of .module wrappers (nn.DataParallel, DDP); TypeError(message)
    when there is none."""
    m = model
    while hasattr(m, "module") and not isinstance(m, classes):
        m = m.module
    if not isinstance(m, classes):
        raise TypeError(message)
    return m


def adamw_hyper(group):
    """(weight_decay, betas, eps) of an optimiser's parameter group: the AdamW hyper-parameters a captured step holds as
    constants (lr lives in device memory)."""
    return (group["weight_decay"], tuple(group["betas"]), group["eps"])


def get_last_non_padding_labels(past_label, pad_value):
    """train_proposed_depth.py:28-50 (train_unimodal.py:28-50 is the same text), without the per-clip python loop / host
    sync."""
    S = past_label.size(1)
    pos = torch.arange(S, device=past_label.device).expand_as(past_label)
    last = torch.where(past_label != pad_value, pos, torch.full_like(pos, -1)).max(dim=1).values
    out = past_label.gather(1, last.clamp_min(0).unsqueeze(1)).squeeze(1)
    return torch.where(last >= 0, out, torch.full_like(out, pad_value))


def weighted_accuracy(pred, gold, pad_idx, t_n_labels, weight_same=1.0, weight_different=10.0):
    """train_proposed_depth.py:9-26 (train_unimodal.py:9-26 is the same text; the weight cancels in the ratio; kept for
    signature parity)."""
    pred = pred.max(1)[1]
    mask = gold.ne(pad_idx)
    total = int(mask.sum())
    return float((pred.eq(gold) & mask).sum()) / total if total > 0 else 0


def _graph_key(eng, hyper):
    """What a captured step depends on besides its batch shape: the AdamW hyper-parameters and the engine's high-water
    mark of pos_embedding gradient rows (a step clears rows [S, mark) as the mark stood AT CAPTURE, so a longer batch seen
    since then forces a re-capture)."""
    return (hyper, eng.pos_grad_rows)


class GraphedSteps:
    """Replays a fused training step (forward + losses + backward + AdamW + epoch accumulators) as ONE hipGraph per
    batch shape.  Enqueued launch by launch from Python the fusion model's 36-launch step is bound by the host (measured
    1.68 ms/step against 0.29 ms replayed), so the loop keeps static device buffers per batch shape, copies each batch into
    them (device-to-device, or straight from the loader when it is given these buffers) and replays.  The first step of a
    shape runs eagerly (allocations, planner), the second one is captured; lr lives in device memory and may change
    between replays, the other AdamW hyper-parameters are part of the capture (a change re-captures).

    A subclass supplies _enqueue(buf, lr, hyper, training): the step's launches on the tensors of buf.  graph=False: every
    step is that enqueue on the caller's own tensors -- no static buffers, no copies, no capture."""

    def __init__(self, eng, acc_loss, acc_cnt, graph=True):
        self.eng, self.acc_loss, self.acc_cnt, self.graph = eng, acc_loss, acc_cnt, graph
        self.shapes = {}

    def step(self, batch, lr, hyper, training):
        eng = self.eng
        if not self.graph:
            eng.set_lr(lr)
            self._enqueue(batch, lr, hyper, training)
            return
        key = tuple(tuple(t.shape) for t in batch) + (bool(training), float(eng.erank_weight),
                                                      str(eng.erank_route), str(eng.erank_fold))
        st = self.shapes.get(key)
        if st is None:
            st = self.shapes[key] = dict(buf=[torch.empty_like(t) for t in batch], seen=0, graph=None, hyper=None)
        for dst, src in zip(st["buf"], batch):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        eng.set_lr(lr)
        self._step(st, lr, hyper, training)

    def _step(self, st, lr, hyper, training):
        """One step on the static buffers of the record st: replay, or eager (first of its shape, or the graph key has
        changed), or capture and replay."""
        gkey = _graph_key(self.eng, hyper)
        if st["graph"] is not None and st["hyper"] == gkey:
            st["graph"].replay()
            return
        self.eng._drop_ready = None
        if st["seen"] == 0 or st["hyper"] not in (None, gkey):
            self._run(st, lr, hyper, training)                              # eager: sizes every workspace
            st["seen"], st["hyper"], st["graph"] = 1, gkey, None
            return
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            self._run(st, lr, hyper, training)
        st["graph"], st["hyper"] = g, gkey
        g.replay()

    def _run(self, st, lr, hyper, training):
        """What one graph holds."""
        self._enqueue(st["buf"], lr, hyper, training)

    def _accumulate(self, loss, counts):
        self.acc_loss += loss
        self.acc_cnt += counts


def validate(model, core, val_loader, pad_idx, to_dev, forward):
    """The body of validate() in train_proposed_depth.py:52-108 and train_unimodal.py:52-125: the action CE and the duration
    loss (normalised duration against the UNMASKED target) per batch, no seg loss; leaves the model in eval().
    to_dev(data, device) -> the batch on the device; forward(eng, batch) -> (the model's outputs, past_label,
    trans_dur_future, trans_future_target)."""
    model.eval()
    eng = core.engine()
    val_loss = 0.0
    val_class_correct = 0
    val_class_total = 0
    val_seg_correct = 0
    val_seg_total = 0
    val_weighted_accuracy_total = 0
    with torch.no_grad():
        for data in val_loader:
            if data is None:
                continue
            out, past_label, trans_dur_future, trans_future_target = forward(eng, to_dev(data, eng.device))
            loss, counts = eng.losses(past_label, trans_future_target, trans_dur_future, with_grad=False, val_mode=True)
            lv, cv = loss.cpu(), counts.cpu()                       # one readback per validation clip
            val_loss += float(lv[1] + lv[2])                        # action CE + duration
            val_class_correct += int(cv[2])
            val_class_total += int(cv[3])
            val_weighted_accuracy_total += weighted_accuracy(
                out["action"].reshape(-1, out["action"].size(-1)), trans_future_target.view(-1), pad_idx,
                get_last_non_padding_labels(past_label, pad_idx))
    val_loss /= len(val_loader)
    val_accuracy = val_class_correct / val_class_total if val_class_total else 0
    val_seg_accuracy = val_seg_correct / val_seg_total if val_seg_total else 0
    val_weighted_accuracy = val_weighted_accuracy_total / len(val_loader)
    print(f"Validation Loss: {val_loss:.3f}, Class Accuracy: {val_accuracy:.3f}, Segmentation Accuracy: "
          f"{val_seg_accuracy:.3f}, Weighted Accuracy: {val_weighted_accuracy:.3f}")
    return val_loss, val_accuracy, val_weighted_accuracy


def print_epoch(args, epoch, i, acc_loss, acc_cnt, acc_sc=None, seg_line=False):
    """The single device->host read of an epoch and its lines.  acc_loss: the sums of (seg, action CE, duration, total);
    acc_cnt: (seg correct, seg rows, action correct, action rows); i: the index of the epoch's last batch.
    seg_line: train_unimodal's ``seg loss`` line; acc_sc (the sum of its supervised contrastive term, or None) travels in
    the same transfer and gives the ``supcon loss`` line."""
    lsum, csum = (acc_loss if acc_sc is None else torch.cat([acc_loss, acc_sc])).cpu(), acc_cnt.cpu()
    denom = i + 1                                                # the reference divides by (i+1), skipped or not
    avg = lambda k: float(lsum[k]) / denom if denom else 0.0     # noqa: E731
    print("Epoch [", (epoch + 1), "/", args.epochs, "] Loss : %.3f" % avg(3))
    if args.anticipate:
        accuracy = int(csum[2]) / int(csum[3]) if int(csum[3]) else 0.0
        print("Training Acc :%.3f" % accuracy, "CE loss :%.3f" % avg(1))
        if args.task == "long":
            print("dur loss: %.5f" % avg(2))
    if seg_line:
        acc_seg = int(csum[0]) / int(csum[1]) if int(csum[1]) else 0.0
        print("seg loss :%.3f" % avg(0), ", seg acc : %.5f" % acc_seg)
    if acc_sc is not None:
        print("supcon loss :%.3f" % avg(4))


def save_best(model, model_save_path, seed, epoch, val_loss):
    """The reference's checkpoint writes on an accuracy improvement (the caller's condition): seed_{seed}_checkpoint{epoch}
    .ckpt, then seed_{seed}_best.ckpt anew, then its line."""
    save_path = os.path.join(model_save_path)
    save_file = os.path.join(save_path, "seed_" + str(seed) + "_checkpoint" + str(epoch) + ".ckpt")
    torch.save(model.state_dict(), save_file)
    best_save_file = os.path.join(save_path, "seed_" + str(seed) + "_best.ckpt")
    if os.path.exists(best_save_file):
        os.remove(best_save_file)
    torch.save(model.state_dict(), best_save_file)
    print(f"Best model saved with validation loss: {val_loss:.3f}")
