"""Seeded case table of the loss launches (r3d_losses_fwd_bwd / r3d_losses_fwd_bwd_kseg), shared by tests/test_loss_optim_cpu.py
(the table against the project's oracle, and that every edge it lists really occurs) and tests/test_loss_optim_gpu.py.

A case names its shape, its options and, per clip, a label layout and a count of live durations:

    labels   "F"   no pad anywhere                   "L<k>"  last observed label at position k, pads behind it
             "M"   pads in the middle, none at the tail      "A"     every label is the pad
    durs     None  a random count 1 .. Q of live durations, the rest padded      0   every duration padded      k   k live

Rows are then edited, each edit on a row of its own (seg rows and anticipation rows alike):

    ties (i, j)   one value, larger than the rest of the row, copied to columns i and j -- once on a row labelled min(i, j)
                  (correct under the first-index rule only) and once on a row labelled max(i, j) (wrong under that rule only)
    last_max      the maximum at the last column, on a row with that label
    pad_argmax    (pad_idx inside the logits) the maximum at column pad_idx, on a live row (the +2 penalty of the seg loss)
                  and on an ignored one (no penalty)

`seg_ties` / `act_ties` replace `ties` on one side; act_edits=False leaves the anticipation rows alone (Q = 1: every row is a
clip's first target, which the weights are built on).

Excluded labels go into both label tensors whenever exclude_idx is inside [0, K); `oob` puts labels outside [0, classes) into
both (the `_kseg` cases always carry seg labels >= Kseg).  Logits are float32 normals; ties are exact copies.

Margins are the project's own (losses rtol 1e-4 / atol 1e-6 as test_decoder_tail_losses_one_launch, gradients 1e-3 of the tensor's
scale as close_rel, counters exact); no case needed a measured one."""
import torch


def _c(name, B, S, Q, K, pad, labels, durs=None, **kw):
    assert len(labels) == B and (durs is None or len(durs) == B)
    c = dict(name=name, B=B, S=S, Q=Q, K=K, pad=pad, labels=tuple(labels), durs=tuple(durs) if durs else (None,) * B,
             exclude=47, Kseg=None, val_mode=False, seg=True, grads=True, dur_den=None, grad_scale=1.0, layout="inter",
             ties=(), seg_ties=None, act_ties=None, act_edits=True, last_max=False, pad_argmax=False, oob=False, first_pad=False)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    return c


T64, T65, TK = ((3, 40),), ((0, 64), (64, 1)), ((5, 69), (70, 6))

CASES = [
    # class counts and ties
    _c("k1", 1, 1, 1, 1, 2, ["F"], [1]),                                                            # 3 units
    _c("k2_tie", 1, 7, 8, 2, 3, ["F"], ties=((0, 1),), last_max=True),                              # 16 units
    _c("k17_clips", 3, 7, 8, 17, 18, ["F", "M", "A"], [6, 0, 1], last_max=True),
    _c("k17_pad_inside", 3, 7, 8, 17, 5, ["L0", "M", "F"], exclude=3, pad_argmax=True, layout="sep"),
    _c("k63_ties", 3, 64, 8, 63, 64, ["L63", "L0", "M"], ties=T64, last_max=True, layout="sep"),
    _c("k64_ties_pad_inside", 1, 65, 9, 64, 10, ["L64"], ties=T64, pad_argmax=True, last_max=True),  # 75 units
    _c("k65_ties", 3, 65, 1, 65, 66, ["L64", "L63", "F"], [1, 0, 1], ties=T65, last_max=True, act_edits=False),  # 201 units
    _c("k122_ties", 3, 7, 8, 122, 123, ["F", "M", "A"], [8, 1, 0], ties=TK, last_max=True, first_pad=True),
    _c("k128_ties_pad_inside", 1, 130, 70, 128, 100, ["L64"], ties=TK, pad_argmax=True, last_max=True, layout="sep"),
    _c("k129_ties_b9", 9, 7, 8, 129, 130, ["F", "M", "A", "L0", "F", "M", "L3", "F", "L6"], ties=TK, last_max=True,
       exclude=128),
    # clip layouts, long clips, many queries
    _c("s130_q70", 3, 130, 70, 17, 18, ["L129", "L63", "L64"], [None, 0, 1], layout="sep"),         # 603 units
    _c("s1_q9_b9", 9, 1, 9, 17, 18, ["F", "A", "F", "F", "A", "F", "F", "F", "F"], [None, 0, 1, None, None, 9, None, 2, None]),
    _c("s65_q1_b9", 9, 65, 1, 17, 3, ["L64", "L0", "M", "A", "F", "L63", "L1", "M", "F"], [1, 0, 1, 1, 0, 1, 1, 1, 0],
       exclude=5, pad_argmax=True, oob=True, act_edits=False),
    # modes
    _c("val_noseg", 3, 7, 8, 17, 18, ["F", "M", "A"], [None, 0, 1], val_mode=True, seg=False, grads=False),
    _c("val_noseg_long", 3, 65, 70, 122, 123, ["L64", "M", "A"], [None, 0, 1], val_mode=True, seg=False, grads=False,
       dur_den=7.25, ties=TK),
    _c("val_seg", 3, 7, 8, 17, 18, ["F", "M", "A"], [6, 0, 1], val_mode=True, last_max=True),
    _c("val_seg_nograds", 1, 64, 9, 65, 20, ["L63"], [9], val_mode=True, grads=False, ties=T65, pad_argmax=True, layout="sep"),
    _c("durden_gs", 3, 7, 8, 17, 18, ["F", "M", "A"], [None, 0, 1], dur_den=5.5, grad_scale=0.25),
    _c("durden_gs_k122", 1, 7, 8, 122, 123, ["F"], [8], dur_den=0.75, grad_scale=0.25, ties=TK, seg_ties=((70, 6),),
       layout="sep"),
    _c("gs_pad_inside_q9", 3, 7, 9, 63, 62, ["F", "L0", "A"], [9, 9, 0], grad_scale=0.25, exclude=7, ties=T64,
       pad_argmax=True, oob=True),
    # seg logits of Kseg = K - 1 classes (labels >= Kseg among the seg labels)
    _c("kseg_k2", 1, 7, 8, 2, 3, ["F"], Kseg=1),
    _c("kseg_k17", 3, 7, 8, 17, 18, ["F", "M", "A"], [5, 0, 1], Kseg=16, last_max=True, layout="sep"),
    _c("kseg_k65", 3, 65, 8, 65, 66, ["L64", "M", "L0"], Kseg=64, ties=T65, seg_ties=T64, last_max=True),
    _c("kseg_k129_pad_inside", 3, 7, 9, 129, 77, ["F", "M", "L3"], Kseg=128, ties=TK, pad_argmax=True, last_max=True,
       grad_scale=0.25, dur_den=3.0, layout="sep"),
    _c("kseg_k122_val", 1, 64, 1, 122, 123, ["L63"], Kseg=121, val_mode=True, grads=False, ties=TK, act_edits=False),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def units(c):
    return c["B"] * (c["S"] + c["Q"] + 1)


def in_oracle_subset(c):
    """what oracle.futr_oracle.losses can express: training mode, seg of K classes, class 47 excluded, no label outside the logits"""
    return (not c["val_mode"]) and c["Kseg"] is None and c["seg"] and c["exclude"] == 47 and not c["oob"]


def _seed(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"])) % 100003


def _clip_labels(spec, S, K, pad, g):
    lab = torch.randint(0, K, (S,), generator=g)
    lab[lab == pad] = (pad + 1) % K if K > 1 else 0
    if spec == "A":
        lab[:] = pad
    elif spec == "M":
        if S >= 3:
            lab[1:S - 1:2] = pad
    elif spec.startswith("L"):
        lab[int(spec[1:]) + 1:] = pad
    else:
        assert spec == "F"
    return lab


def _edit_rows(x, gold, C, pad, exclude, ties, last_max, pad_argmax, keep):
    """x [rows, C] logits, gold [rows] labels (both edited in place); rows in `keep` are left alone"""
    def live(r):
        t = int(gold[r])
        return t != pad and t != exclude and 0 <= t < C
    free = [r for r in range(x.shape[0]) if live(r) and r not in keep]
    ignored = [r for r in range(x.shape[0]) if int(gold[r]) == pad and r not in keep]

    def take():
        assert free, "the case has too few live rows for its edits"
        return free.pop(len(free) // 2)
    for (i, j) in ties:
        assert i < C and j < C and pad not in (i, j) and exclude not in (i, j)
        for lab in (min(i, j), max(i, j)):
            r = take()
            x[r, i] = x[r].max() + 1.0
            x[r, j] = x[r, i]
            gold[r] = lab
    if last_max and C - 1 not in (pad, exclude):
        r = take()
        x[r, C - 1] = x[r].max() + 1.0
        gold[r] = C - 1
    if pad_argmax:
        assert 0 <= pad < C
        r = take()
        x[r, pad] = x[r].max() + 1.0
        if ignored:
            r = ignored[len(ignored) // 2]
            x[r, pad] = x[r].max() + 1.0


def make(c):
    """-> dict of CPU tensors: seg [B, S, Kseg or K] float32 (None without seg), act [B, Q, K], dur [B, Q], past_label [B, S],
    target [B, Q] int64, target_dur [B, Q] float32"""
    B, S, Q, K, pad, exclude = c["B"], c["S"], c["Q"], c["K"], c["pad"], c["exclude"]
    Ks = c["Kseg"] or K
    g = torch.Generator().manual_seed(_seed(c))
    seg = torch.randn(B * S, Ks, generator=g)
    act = torch.randn(B * Q, K, generator=g)
    dur = 0.5 * torch.randn(B, Q, generator=g)
    lab = torch.stack([_clip_labels(s, S, K, pad, g) for s in c["labels"]])
    tgt = torch.randint(0, K, (B, Q), generator=g)
    tgt[tgt == pad] = (pad + 1) % K if K > 1 else 0
    td = torch.rand(B, Q, generator=g) + 0.05
    for b in range(B):
        k = c["durs"][b]
        k = 1 + int(torch.randint(0, Q, (1,), generator=g)) if k is None else k
        tgt[b, max(k, 1):] = pad                      # (a clip without live durations keeps its first target)
        td[b, :k] = td[b, :k] / td[b, :k].sum() if k else td[b, :k]
        td[b, k:] = float(pad)
    # the per-clip weight: even clips continue their last observed label (weight 1), odd clips do not (weight 10)
    for b in range(B):
        nz = (lab[b] != pad).nonzero().flatten()
        last = int(lab[b, nz[-1]]) if nz.numel() else pad
        if b % 2 == 0:
            tgt[b, 0] = last
        elif int(tgt[b, 0]) == last:
            tgt[b, 0] = (last + 1) % K if (last + 1) % K != pad else (last + 2) % K
        if c["labels"][b] == "A" and not c["first_pad"] and int(tgt[b, 0]) == pad:
            tgt[b, 0] = (pad + 1) % K                 # an all-pad clip whose first target is live: weight 10
    lab, tgt = lab.reshape(-1), tgt.reshape(-1)
    # excluded and out-of-range labels, on rows the weights do not depend on
    keep_seg = set()
    for b in range(B):
        nz = (lab[b * S:(b + 1) * S] != pad).nonzero().flatten()
        if nz.numel():
            keep_seg.add(b * S + int(nz[-1]))
    keep_act = {b * Q for b in range(B)}

    def sprinkle(gold, keep, value, at):
        rows = [r for r in range(gold.numel()) if int(gold[r]) != pad and r not in keep]
        for r in rows[at::5][:3]:
            gold[r] = value
            keep.add(r)
    if 0 <= exclude < K:
        sprinkle(lab, keep_seg, exclude, 0)
        sprinkle(tgt, keep_act, exclude, 0)
    if c["Kseg"]:
        sprinkle(lab, keep_seg, Ks, 1)                # K - 1: a class of the anticipation head only
    if c["oob"]:
        sprinkle(lab, keep_seg, K + 5, 2)
        sprinkle(tgt, keep_act, K + 5, 2)
        sprinkle(tgt, keep_act, -3, 3)
    seg_ties = c["ties"] if c["seg_ties"] is None else c["seg_ties"]
    _edit_rows(seg, lab, Ks, pad, exclude, seg_ties, c["last_max"], c["pad_argmax"] and 0 <= pad < Ks, keep_seg)
    if c["act_edits"]:
        act_ties = c["ties"] if c["act_ties"] is None else c["act_ties"]
        _edit_rows(act, tgt, K, pad, exclude, act_ties, c["last_max"], c["pad_argmax"] and 0 <= pad < K, keep_act)
    return dict(seg=seg.view(B, S, Ks) if c["seg"] else None, act=act.view(B, Q, K), dur=dur, past_label=lab.view(B, S),
                target=tgt.view(B, Q), target_dur=td)
