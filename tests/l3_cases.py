"""Cases and tolerances of the L3 query model's kernels (csrc/attention_xclip.hip, csrc/l3mix.hip) for tests/test_l3_cpu.py
and tests/test_l3_gpu.py.

Cross-clip attention.  The cross B in {1, 2, 8, 13, 33, 64} x S in {1, 5, 64, 200} x (H, heads) in {(8, 8), (64, 4), (128, 8),
(136, 4), (1024, 8)} (head widths 1, 16, 16, 34, 128), thinned: every (B, width) pair runs at S = 1 (at most one workgroup's frame run), every other pair also at S = 5 (a partial
last run wherever the run is 2 to 4 frames), and every pair at one long clip (the longest of 200, 64, 5
whose qkv stays below 3M floats; always several workgroups along the frames, test_l3_cpu.py asserts both).  Inputs are
standard normal float32 values, so the scores are of order one.

A tolerance is 8 times the error of the float32 restatement (tests/l3_oracle.py with dtype float32, in the two summation
orders of l3_oracle.xclip_orders) against the float64 one ON THAT CASE'S INPUTS, max |f32 - f64| / max |f64|.  It is computed
from the oracle alone, here, at first use; no kernel result enters it.

Mix.  N in {1, 63, 64, 65, 4097}; all rows correct (m = 1, a = b = 0 exactly), none correct (m = 5), padded rows (a padded
row whose arg-max is the pad class included: masked, so wrong), Kseg in {2, 18, 123}, wf in {0, 0.5, 1}, and one case with
arg-max ties built from bit-equal floats (the first index wins).  Outside the constructed ties every row's top two logits
differ (the logits are the kernel's input, so any non-zero gap decides the arg-max).  Flags and m are exact.  c = 1 / m lies in
[0.2, 1] and a, b in [0, 0.8]; each is at most four float32 roundings of quantities of scale one away from its float64 value,
so each is held to 4 float32 epsilon ABSOLUTE (1 - c cancels, so a relative bound on a and b would not follow); the total to
4 epsilon of the sum of the five losses' magnitudes; a scaled gradient is one rounding of d * c with c itself rounded, held to
2 epsilon of |d| element-wise."""
import numpy as np
import torch

from tests import l3_oracle as LO

EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 8
WIDTHS = [(8, 8), (64, 4), (128, 8), (136, 4), (1024, 8)]
CLIPS = [1, 2, 8, 13, 33, 64]
BUDGET = 3_000_000


def _xclip_table():
    rows = []
    for bi, B in enumerate(CLIPS):
        for wi, (H, heads) in enumerate(WIDTHS):
            short = (1, 5) if (bi + wi) % 2 else (1,)
            long_ = next(S for S in (200, 64, 5) if B * S * 3 * H <= BUDGET or S == 5)
            for S in sorted(set(short + (long_,))):
                rows.append(dict(name=f"B{B}_S{S}_H{H}_h{heads}", B=B, S=S, H=H, heads=heads, seed=1000 * bi + 10 * wi + S))
    return rows


XCLIP = _xclip_table()
XCLIP_BY_NAME = {c["name"]: c for c in XCLIP}


def xclip_inputs(case):
    """(qkv [B, S, 3 H], d_o [B, S, H]) float32"""
    g = torch.Generator().manual_seed(case["seed"])
    B, S, H = case["B"], case["S"], case["H"]
    return torch.randn(B, S, 3 * H, generator=g), torch.randn(B, S, H, generator=g)


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


_XREF = {}


def xclip_reference(name):
    """dict(o, d_qkv: float64; tol_o, tol_d: 8 x the float32 restatement's error), computed once per case"""
    if name not in _XREF:
        case = XCLIP_BY_NAME[name]
        qkv, d_o = xclip_inputs(case)
        o, d = LO.xclip_fwd(qkv, case["heads"]), LO.xclip_bwd(qkv, d_o, case["heads"])
        eo = ed = 0.0
        for o32, d32 in LO.xclip_orders(qkv, d_o, case["heads"]):
            eo, ed = max(eo, rel_err(o32, o)), max(ed, rel_err(d32, d))
        _XREF[name] = dict(o=o, d_qkv=d, err_o=eo, err_d=ed, tol_o=MARGIN * eo, tol_d=MARGIN * ed)
    return _XREF[name]


# ---------------------------------------------------------------------------------------------------------------------
# mix
# ---------------------------------------------------------------------------------------------------------------------
def _mix(name, N, Kseg, wf, kind="mixed", pad_rows=0.0, ties=False, seed=0):
    return dict(name=name, N=N, Kseg=Kseg, wf=wf, kind=kind, pad_rows=pad_rows, ties=ties, seed=seed)


MIX = [
    _mix("n1", 1, 18, 0.5, seed=1), _mix("n63", 63, 18, 0.5, seed=2), _mix("n64", 64, 18, 0.5, seed=3),
    _mix("n65", 65, 18, 0.5, seed=4), _mix("n4097", 4097, 18, 0.5, pad_rows=0.2, seed=5),
    _mix("all_correct", 65, 18, 0.5, kind="all", seed=6), _mix("none_correct", 65, 18, 0.5, kind="none", seed=7),
    _mix("n1_correct", 1, 2, 0.0, kind="all", seed=8),
    _mix("padded", 200, 18, 0.5, pad_rows=0.4, seed=9), _mix("k2", 130, 2, 0.5, pad_rows=0.1, seed=10),
    _mix("k123", 67, 123, 0.5, pad_rows=0.1, seed=11), _mix("wf0", 65, 18, 0.0, seed=12), _mix("wf1", 65, 18, 1.0, seed=13),
    _mix("ties", 66, 18, 0.5, ties=True, seed=14), _mix("ties_k123", 66, 123, 0.5, ties=True, seed=15),
]
MIX_BY_NAME = {c["name"]: c for c in MIX}
MIX_Q, MIX_K = 8, 10                    # the anticipation gradient of a mix case is [ceil(N / 16) * Q, K + 1]


def mix_inputs(case):
    """dict(seg f32 [N, Kseg], label int64 [N], pad, l3 bool [N], tie_rows, losses f32 (L3, Lc, Lseg, Lact, Ldur), d_seg, d_actdur)"""
    r = np.random.RandomState(case["seed"])
    N, K = case["N"], case["Kseg"]
    pad = K - 1
    seg = r.randn(N, K).astype(np.float32)
    arg = seg.argmax(1)
    kind = case["kind"]
    if kind == "all":
        seg[np.arange(N), pad] = -10.0                            # (no row's arg-max is the pad class)
        arg = seg.argmax(1)
        label, l3 = arg.copy(), np.ones(N, bool)
    elif kind == "none":
        label, l3 = arg.copy(), np.zeros(N, bool)
    else:
        label = np.where(r.rand(N) < 0.6, arg, r.randint(0, K, N))
        l3 = r.rand(N) < 0.7
    padded = r.rand(N) < case["pad_rows"]
    label = np.where(padded, pad, label)
    if case["pad_rows"] > 0 and N > 2:                            # a padded row whose arg-max is the pad class
        seg[1, pad], label[1], l3[1] = 9.0, pad, True
    tie_rows = []
    if case["ties"]:
        # rows 0..3: the maximum twice, bit-equal, at columns (lo, hi); the label is lo (correct) on even rows, hi on odd
        for row, (lo, hi) in enumerate([(0, 1), (0, 1), (3, K - 2), (3, K - 2)]):
            seg[row, lo] = seg[row, hi] = np.float32(7.25)
            label[row], l3[row] = (lo if row % 2 == 0 else hi), True
            tie_rows.append(row)
        assert all(seg[t, a].tobytes() == seg[t, b].tobytes() for t, (a, b) in zip(tie_rows, [(0, 1), (0, 1), (3, K - 2), (3, K - 2)]))
    losses = (0.25 + r.rand(5)).astype(np.float32)
    R = -(-N // 16) * MIX_Q
    return dict(seg=seg, label=label.astype(np.int64), pad=pad, l3=l3, tie_rows=tie_rows, losses=losses,
                d_seg=r.randn(N, K).astype(np.float32), d_actdur=r.randn(R, MIX_K + 1).astype(np.float32))


def mix_reference(case):
    """the float64 mix of a case (l3_oracle.mix) with its inputs"""
    c = mix_inputs(case)
    L3, Lc, Lseg, Lact, Ldur = (float(v) for v in c["losses"])
    ref = LO.mix(c["seg"], c["label"], c["pad"], c["l3"], L3, Lc, Lseg, Lact, Ldur, case["wf"])
    return c, ref


SCALAR_TOL = 4 * EPS32
GRAD_TOL = 2 * EPS32


# ---------------------------------------------------------------------------------------------------------------------
# whole step: the fixtures of tests/golden/make_golden_l3.py
# ---------------------------------------------------------------------------------------------------------------------
WFS = (0.0, 1.0 / 30.0, 1.0)


def _step(tag, B, S, H, n_head, n_class, seed, n_dec=1, query_num=49, ragged=False):
    return dict(tag=tag, B=B, S=S, H=H, n_head=n_head, n_class=n_class, n_dec=n_dec, query_num=query_num, seed=seed,
                ragged=ragged, lr=1e-3, wd=5e-3)


STEP_CASES = [_step("l3_tiny", 8, 5, 16, 2, 7, 1), _step("l3_cfg", 8, 16, 128, 8, 17, 1),
              _step("l3_odd", 13, 37, 136, 4, 17, 1, ragged=True)]
STEP_BY_TAG = {c["tag"]: c for c in STEP_CASES}


def pad_idx(c):
    return c["n_class"] + 1


def batch(c, seed):
    """(features, past_label, trans_dur_future, trans_future_target, query_label) as torch tensors.  query_label: runs of 2 to 6
    frames over the classes [0, 47), with the pad (47) and excluded (48) labels on a few frames; ragged: every clip ends in
    1 .. S // 3 padded frames (past_label = pad_idx there)."""
    from oracle import synth
    B, S = c["B"], c["S"]
    pad = pad_idx(c)
    feats, _, lab, dur, tgt = synth.make_batch(B, S, c["n_class"], pad, seed, depth_hw=(1, 1))
    base = ((seed & 0xFFFFFF) << 8) + 0x40
    if c["ragged"]:
        tail = 1 + synth.randint(B, max(1, S // 3), base + 1)
        for b in range(B):
            lab[b, S - int(tail[b]):] = pad
    run_len = 2 + synth.randint(B * S, 5, base + 2)
    run_lab = synth.randint(B * S, 47, base + 3)
    special = synth.randint(B * S, 23, base + 4)
    ql = np.zeros((B, S), np.int64)
    k = 0
    for b in range(B):
        t = 0
        while t < S:
            v = int(run_lab[k])
            if special[k] == 0:
                v = 47
            elif special[k] == 1:
                v = 48
            ql[b, t:t + int(run_len[k])] = v
            t += int(run_len[k])
            k += 1
    return [torch.from_numpy(np.ascontiguousarray(x)) for x in (feats, lab, dur, tgt, ql)]


def adamw_first_step(p, g, lr, wd, dtype):
    """torch.optim.AdamW's first step from zero moments, in `dtype`"""
    p, g = p.to(dtype), g.to(dtype)
    m, v = (1 - 0.9) * g, (1 - 0.999) * g * g
    return p * (1 - lr * wd) - lr * (m / (1 - 0.9)) / ((v / (1 - 0.999)).sqrt() + 1e-8)


def post_tolerance(p, g, grad_tol_abs, lr):
    """Element-wise absolute tolerance of a parameter after AdamW's first step, by propagating the gradient's tolerance.  The
    first step moves an element by u(g) = lr g / (|g| + 1e-8), whose slope lr 1e-8 / (|g| + 1e-8)^2 reaches lr / 1e-8 at
    g = 0: an element whose gradient is rounding noise moves by up to +-lr in any float32 implementation, so a bound relative
    to the tensor would not follow from the gradient's.  Allowed: the steepest slope of u within grad_tol_abs of g times
    grad_tol_abs, at most 2 lr (|u| <= lr), plus 8 float32 epsilon of |p| + lr for the update's own roundings."""
    g = g.detach().double().abs()
    slope = lr * 1e-8 / ((g - grad_tol_abs).clamp_min(0.0) + 1e-8) ** 2
    return (slope * grad_tol_abs).clamp_max(2 * lr) + 8 * EPS32 * (p.detach().double().abs() + lr)


ZERO_GRAD = "fc_len.bias"
_STEP_REF = {}


def relabel(c, b, out64):
    """The batch with labels a model at these parameters gets partly right, so that m lies strictly between 1 and 5: on about
    half of the unpadded frames past_label becomes the float64 oracle's seg arg-max, and on about two thirds of the frames
    query_label becomes its l3 arg-max where that is a class below 47.  Neither set of logits depends on these labels (the
    padded positions, which make the decoder's key mask, stay).  The fixture stores both label arrays."""
    from oracle import synth
    feats, lab, dur, tgt, ql = [t.clone() for t in b]
    B, S = lab.shape
    pad = pad_idx(c)
    seg_arg = torch.from_numpy(LO.first_argmax(out64["seg"].detach().reshape(B * S, -1).numpy())).reshape(B, S)
    l3_arg = torch.from_numpy(LO.first_argmax(out64["l3"].detach().reshape(B * S, -1).numpy())).reshape(B, S)
    pick2 = torch.from_numpy(synth.randint(B * S, 2, 0x77000 + c["seed"])).reshape(B, S) == 0
    pick3 = torch.from_numpy(synth.randint(B * S, 3, 0x78000 + c["seed"])).reshape(B, S) != 0
    lab = torch.where(pick2 & (lab != pad) & (seg_arg < c["n_class"] - 1), seg_arg, lab)
    ql = torch.where(pick3 & (l3_arg < 47), l3_arg, ql)
    return [feats, lab.contiguous(), dur, tgt, ql.contiguous()]


def step_reference(c, b, p0, wf):
    """dict(out, res, grads, post: float64; tol: {quantity: 8 x the float32 restatement's error}) of a step on the batch b,
    computed once per (case, wf).  The quantities: the four outputs, the five losses and the total, "grad::name" and
    "post::name" of every live parameter."""
    key = (c["tag"], wf)
    if key in _STEP_REF:
        return _STEP_REF[key]
    pad = pad_idx(c)
    out, res, grads = LO.step(p0, b, pad, wf, c["n_head"], c["n_dec"], 8, torch.float64)
    o32, r32, g32 = LO.step(p0, b, pad, wf, c["n_head"], c["n_dec"], 8, torch.float32)
    tol = {}
    for k in out:
        tol[k] = MARGIN * rel_err(o32[k].detach(), out[k].detach())
    for k in ("L3", "Lc", "Lseg", "Lact", "Ldur", "total"):
        tol[k] = MARGIN * rel_err(r32[k].detach(), res[k].detach())
    live = [n for n in grads if n.startswith(LO.LIVE_PREFIXES)]
    post = {}
    for n in live:
        S = c["S"]
        g64, g_32 = grads[n], g32[n]
        if n == "pos_embedding":
            g64, g_32, pn = g64[:, :S], g_32[:, :S], p0[n][:, :S]
        else:
            pn = p0[n]
        tol["grad::" + n] = MARGIN * rel_err(g_32, g64)
        if n == ZERO_GRAD:
            # its true gradient is 0 (normalize_duration divides exp(duration) by its sum over the clip's queries: a shift of
            # every duration cancels), so what any float32 step holds there is the rounding of a cancelling sum over the B Q
            # rows of the duration column of d_actdur.  fc.bias sums the other columns over the same rows: the bound is 64
            # float32 epsilon of fc.bias's largest gradient, expressed relative to this tensor's own (tiny) float64 scale.
            tol["grad::" + n] = 64 * EPS32 * float(grads["fc.bias"].abs().max()) / max(float(g64.abs().max()), 1e-30)
        post[n] = adamw_first_step(pn, g64, c["lr"], c["wd"], torch.float64)
        tol["post::" + n] = post_tolerance(pn, g64, tol["grad::" + n] * float(g64.abs().max()), c["lr"])
    _STEP_REF[key] = dict(out=out, res=res, grads=grads, post=post, tol=tol, live=live, flags32=(r32["l3_correct"], r32["l2_correct"]))
    return _STEP_REF[key]


def forward_tolerances(c, b, p0):
    """the output tolerances (relative to each tensor's largest magnitude): 8 x the float32 forward's error against float64"""
    pad = pad_idx(c)
    o64, _ = LO.forward({n: v.double() for n, v in p0.items()}, (b[0], b[1]), "train", pad, c["n_head"], c["n_dec"], 8)
    o32, _ = LO.forward({n: v.float() for n, v in p0.items()}, (b[0], b[1]), "train", pad, c["n_head"], c["n_dec"], 8)
    return o64, {k: MARGIN * rel_err(o32[k], o64[k]) for k in o64}


def tie_margin(out64, tol):
    """the smallest, over the seg and l3 logits, of (a row's top-two gap) / (4 x the logit tolerance): admissible above 1"""
    worst = np.inf
    for k in ("seg", "l3"):
        x = out64[k].detach().reshape(-1, out64[k].shape[-1]).numpy()
        worst = min(worst, float(LO.top_two_gap(x).min()) / max(4 * tol[k] * float(np.abs(x).max()), 1e-300))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the loop fixture (tests/golden/l3_train_loop.npz): its batch lists, and the tie condition along the float64 oracle's run
# ---------------------------------------------------------------------------------------------------------------------
LOOP_EPOCHS = 3


def loop_data(c, seed):
    """(train, val): two training batches with one of 3 clips between them (skipped: fewer than 8), one validation batch of
    S + 1 frames.  The fixture stores the validation batch's future labels (its generator chose them); they feed no seg or l3
    logit."""
    train = [batch(c, seed), batch(dict(c, B=3), seed + 50), batch(c, seed + 1)]
    val = [batch(dict(c, S=c["S"] + 1), seed + 100)]
    return train, val


def warmup_factor(epoch):
    """get_warmup_factor(epoch, 0, 30, 60) of the loop"""
    return epoch / 30.0 if epoch < 30 else (1.0 - (epoch - 30) / 30.0 if epoch < 60 else 0.0)


def loop_tie_margins(c, train, val, p0, epochs=LOOP_EPOCHS):
    """The float64 oracle's run of the loop -- LO.step and torch's AdamW rule, step by step -- and, at every training step and
    at every validation forward, tie_margin of that forward's seg and l3 logits against 4 x the logit tolerances at the
    parameters of that moment (8 x the float32 forward's error there).  Returns [(what, margin)]: admissible where every margin
    exceeds 1, since the loop's flags feed m, the losses and the printed accuracies; and the oracle's final parameters."""
    from oracle import futr_oracle as O
    pad = pad_idx(c)
    p = {n: v.detach().double().clone() for n, v in p0.items()}
    live = [n for n in p if n.startswith(LO.LIVE_PREFIXES)]
    m1 = {n: torch.zeros_like(p[n]) for n in live}
    m2 = {n: torch.zeros_like(p[n]) for n in live}
    out, t = [], 0
    for epoch in range(epochs):
        for i, b in enumerate(train):
            if len(b[0]) < 8:
                continue
            o64, tol = forward_tolerances(c, b, p)
            out.append((f"epoch {epoch} step {i}", tie_margin(o64, tol)))
            _, _, grads = LO.step(p, b, pad, warmup_factor(epoch), c["n_head"], c["n_dec"], 8)
            t += 1
            with torch.no_grad():
                for n in live:
                    O.adamw_step(p[n], grads[n], m1[n], m2[n], t, c["lr"], c["wd"])
        for j, b in enumerate(val):
            o64, tol = forward_tolerances(c, b, p)
            out.append((f"epoch {epoch} validation {j}", tie_margin(o64, tol)))
    return out, p
