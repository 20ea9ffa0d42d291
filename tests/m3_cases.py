"""Cases and tolerances of the three-modality model (csrc/fuse3_seam.hip, r3d_amd/engine_m3.py) for tests/test_m3_cpu.py and
tests/test_m3_gpu.py.

Seam.  One case per (H, N) pair of H in {8, 72, 128, 136, 512, 520, 1024} (every EPL instance, on and off the 64-column grid)
x N in {1, 5, 64, 67}; the other factors -- gaze_dim in {1, 2, 5, 8}, the mask (empty, full, the k = H // 4 selection), with /
without a keep mask, ns_r in {0, 1, 3}, ns_d in {1, 4}, add2 present / absent -- cycle over the pairs so that every value of
every factor meets every EPL instance (test_m3_cpu.py asserts it).  Two more: "saturated" (a depth row and a gaze row that are
constant, so their LayerNorm variance is 0, and a token row the keep mask drops whole, so norm1's is) and "stride" (N = 1030 >
the forward's 1024 workgroups: the frame loop takes a second turn).  A case's seed is the first of its sequence at which no
pre-activation of the seam's three ReLUs lies within RELU_GUARD of zero in the float64 oracle (a float32 implementation gates
such an element either way, and a gate flips a whole gradient element).

Tolerance (a step's scalar losses: see SCALAR_FLOOR): 8 x the error of the float32 restatement (tests/m3_oracle.py on float32 copies, in the three summation orders of
`orders`) against the float64 one ON THAT CASE'S INPUTS, max |f32 - f64| / max |f64| per quantity.  Computed from the oracle
alone, here, at first use; no kernel result enters it.  Exchange outputs are compared with r3d_token_exchange3_fwd of the
kernel's own embeddings bit for bit, selected indices exactly.

Whole steps.  The shapes (B, S, H, heads, classes, decoder layers, depth pixels) of the issue -- the first one twice: with a
clip that is padded whole (m3_tiny: a NaN loss, see `batch`) and with ragged padding alone (m3_ragged: everything finite); parameters are oracle.synth's
analytic fill, batches its make_batch (zero-mean depth) plus a gaze track uniform in [-1, 1)."""
import numpy as np
import torch

from oracle import synth
from tests import m3_oracle as MO

EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 8
RELU_GUARD = 4e-6             # a few float32 roundings of a LayerNorm output of order one
DROP_SCALE = 1.0 / 0.9

WIDTHS = [8, 72, 128, 136, 512, 520, 1024]
FRAMES = [1, 5, 64, 67]
GAZES = [1, 2, 5, 8]
MASKS = ["k", "empty", "full"]


def epl_of(H):
    return 2 if H <= 128 else (8 if H <= 512 else 16)


def _seam_table():
    rows = []
    for hi, H in enumerate(WIDTHS):
        for ni, N in enumerate(FRAMES):
            i = hi * len(FRAMES) + ni
            rows.append(dict(name=f"H{H}_N{N}", H=H, N=N, G=GAZES[(hi + ni) % 4], mask=MASKS[(hi // 1 + 2 * ni) % 3],
                             keep=bool((hi + ni // 2) % 2), ns_r=[0, 1, 3][(i + hi) % 3], ns_d=[1, 4][(ni + hi // 2) % 2],
                             add2=bool((i // 2 + hi) % 2), flavour="", seed0=100 * i))
    rows.append(dict(name="saturated", H=136, N=5, G=2, mask="k", keep=True, ns_r=1, ns_d=4, add2=True, flavour="saturated",
                     seed0=5000))
    rows.append(dict(name="saturated_H8", H=8, N=3, G=1, mask="k", keep=True, ns_r=0, ns_d=1, add2=False, flavour="saturated",
                     seed0=5100))
    rows.append(dict(name="stride", H=72, N=1030, G=2, mask="k", keep=True, ns_r=3, ns_d=4, add2=True, flavour="",
                     seed0=5200))
    return rows


SEAM = _seam_table()
SEAM_BY_NAME = {c["name"]: c for c in SEAM}


def k_mask(H, seed):
    """[3, H] float32: H // 4 channels of each modality chosen by the seed"""
    m = torch.zeros(3, H)
    g = torch.Generator().manual_seed(seed)
    for r in range(3):
        m[r, torch.randperm(H, generator=g)[:H // 4]] = 1.0
    return m


def _seam_draw(case, seed):
    g = torch.Generator().manual_seed(seed)
    H, N, G, ns_r, ns_d = case["H"], case["N"], case["G"], case["ns_r"], case["ns_d"]
    rn = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    un = lambda *s: torch.rand(*s, generator=g) * 2 - 1           # noqa: E731
    d = dict(rgb_src=rn(ns_r, N, H) / max(ns_r, 1) ** 0.5 if ns_r > 0 else torch.relu(rn(N, H)),
             bias_r=0.1 * un(H) if ns_r > 0 else None,
             dep_src=rn(ns_d, N, H) / ns_d ** 0.5, bias_d=0.1 * un(H) if ns_d > 1 else None,
             lnd_g=1 + 0.25 * un(H), lnd_b=0.1 * un(H), gaze=torch.rand(N, G, generator=g), w_g=rn(H, G), b_g=0.1 * un(H),
             lng_g=1 + 0.25 * un(H), lng_b=0.1 * un(H), ln1_g=1 + 0.25 * un(H), ln1_b=0.1 * un(H),
             d_h1=rn(3 * N, H), add1=rn(3 * N, H), add2=rn(3 * N, H) if case["add2"] else None)
    d["mask"] = dict(k=k_mask(H, seed + 7), empty=torch.zeros(3, H), full=torch.ones(3, H))[case["mask"]]
    d["keep"] = (torch.rand(3 * N, H, generator=g) >= 0.1).to(torch.uint8) if case["keep"] else None
    if case["flavour"] == "saturated":
        # frame 1: a constant depth row (every slab the same dyadic constant, bias a dyadic constant: the sum and its mean are
        # exact in any order, so the variance is exactly 0) and a constant gaze row (W_g = 0, b_g dyadic); token row 3 * 1 + 0
        # dropped whole by the keep mask, so norm1 sees a zero row
        d["bias_d"] = torch.full((H,), 0.25) if d["bias_d"] is not None else None
        d["dep_src"][:, 1, :] = 0.125
        d["w_g"] = torch.zeros(H, G)
        d["b_g"] = torch.full((H,), 0.5)
        d["keep"][3, :] = 0
    return d


_SEAM_IN = {}


def seam_inputs(name):
    """the case's float32 inputs, at the first seed of its sequence that keeps every ReLU pre-activation RELU_GUARD from zero"""
    if name not in _SEAM_IN:
        case = SEAM_BY_NAME[name]
        for seed in range(case["seed0"], case["seed0"] + 50):
            d = _seam_draw(case, seed)
            fw = seam_fwd_of(d, case, torch.float64)
            if MO.relu_margin(fw, d["lnd_g"].double(), d["lnd_b"].double(), d["lng_g"].double(), d["lng_b"].double(),
                              case["ns_r"]) >= RELU_GUARD:
                _SEAM_IN[name] = (d, seed)
                break
        else:
            raise AssertionError(f"{name}: no seed keeps the ReLUs clear of zero")
    return _SEAM_IN[name][0]


def _cast(d, dt):
    return {k: (v.to(dt) if (v is not None and v.is_floating_point()) else v) for k, v in d.items()}


def seam_fwd_of(d, case, dt):
    c = _cast(d, dt)
    return MO.seam_forward(c["rgb_src"], case["ns_r"], c["bias_r"], c["dep_src"], c["bias_d"], c["lnd_g"], c["lnd_b"], c["gaze"],
                           c["w_g"], c["b_g"], c["lng_g"], c["lng_b"], c["mask"], c["keep"], DROP_SCALE if c["keep"] is not None else 1.0,
                           c["ln1_g"], c["ln1_b"])


def seam_bwd_of(d, fw, dt):
    c = _cast(d, dt)
    return MO.seam_backward(c["d_h1"], fw, c["add1"], c["add2"], c["keep"], DROP_SCALE if c["keep"] is not None else 1.0,
                            c["mask"], c["ln1_g"], c["lnd_g"], c["lnd_b"], c["lng_g"], c["lng_b"], c["gaze"])


COLUMN_KEYS = ("bias_r", "bias_d", "lnd_g", "lnd_b", "b_g", "lng_g", "lng_b", "ln1_g", "ln1_b", "mask")      # [..., H] vectors
ROW_KEYS = ("rgb_src", "dep_src", "d_h1", "add1", "add2", "keep")                                             # [..., H] matrices


def orders(H):
    """column permutations under which the float32 restatement is evaluated: as stored, reversed, evens then odds -- each
    changes the order of every sum over a row; the slabs are summed first-to-last and last-to-first"""
    idt = torch.arange(H)
    return [(idt, False), (idt.flip(0), True), (torch.cat([idt[0::2], idt[1::2]]), False)]


def _permuted(d, perm, flip_slabs, ns_r):
    out = dict(d)
    for k in COLUMN_KEYS + ROW_KEYS:
        if d[k] is not None:
            out[k] = d[k][..., perm]
    out["w_g"] = d["w_g"][perm]
    if flip_slabs:
        out["dep_src"] = out["dep_src"].flip(0)
        if ns_r > 0:
            out["rgb_src"] = out["rgb_src"].flip(0)
    return out


FWD_KEYS = ("rgb", "dep_pre", "dep", "gz_pre", "gz", "x0", "h1", "mean", "rstd")
BWD_KEYS = ("d_rgb_pre", "d_dep_pre", "d_gz_pre", "p_n1", "p_dep", "p_gz", "dg_n1", "dg_dep", "dg_gz", "d_w_g", "d_b_g")


def pooled(fw, bw):
    """the compared quantities: the row statistics of the three LayerNorms pooled into "mean" and "rstd", and the per-frame
    partials also summed over the frames (dg_*: [2, H] = what the finalize launch leaves in the gradient arena)"""
    q = {k: fw[k] for k in ("rgb", "dep_pre", "dep", "gz_pre", "gz", "x0", "h1")}
    q["mean"] = torch.cat([fw["mean_d"], fw["mean_g"], fw["m1"]])
    q["rstd"] = torch.cat([fw["rstd_d"], fw["rstd_g"], fw["r1"]])
    for k in ("d_rgb_pre", "d_dep_pre", "d_gz_pre", "p_n1", "p_dep", "p_gz", "d_w_g", "d_b_g"):
        q[k] = bw[k]
    for k in ("n1", "dep", "gz"):
        q["dg_" + k] = bw["p_" + k].sum(dim=0)
    return q


def rel_err(got, ref):
    """max |got - ref| over the elements where ref is finite, relative to the largest finite |ref|"""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    ok = torch.isfinite(ref)
    if not bool(ok.any()):
        return 0.0
    return float((got[ok] - ref[ok]).abs().max()) / max(float(ref[ok].abs().max()), 1e-30)


_SEAM_REF = {}


def seam_reference(name):
    """dict(q: the float64 quantities of `pooled`, tol: {quantity: 8 x the float32 restatement's error}), once per case"""
    if name not in _SEAM_REF:
        case = SEAM_BY_NAME[name]
        d = seam_inputs(name)
        fw = seam_fwd_of(d, case, torch.float64)
        q = pooled(fw, seam_bwd_of(d, fw, torch.float64))
        err = {k: 0.0 for k in q}
        for perm, flip in orders(case["H"]):
            dp = _permuted(d, perm, flip, case["ns_r"])
            f32 = seam_fwd_of(dp, case, torch.float32)
            q32 = pooled(f32, seam_bwd_of(dp, f32, torch.float32))
            inv = torch.argsort(perm)
            for k in q:
                v = q32[k]
                if k == "d_w_g":
                    v = v[inv]
                elif k not in ("mean", "rstd"):
                    v = v[..., inv]
                err[k] = max(err[k], rel_err(v, q[k]))
        _SEAM_REF[name] = dict(q=q, fw=fw, err=err, tol={k: MARGIN * e for k, e in err.items()})
    return _SEAM_REF[name]


# ---------------------------------------------------------------------------------------------------------------------
# whole steps
# ---------------------------------------------------------------------------------------------------------------------
def _step(tag, B, S, H, n_head, n_class, n_dec, pixels, seed, ragged=False, gaze_dim=2):
    return dict(tag=tag, B=B, S=S, H=H, n_head=n_head, n_class=n_class, n_dec=n_dec, pixels=pixels, seed=seed, ragged=ragged,
                gaze_dim=gaze_dim, lr=1e-3, wd=5e-3)


STEP_CASES = [_step("m3_tiny", 2, 5, 64, 4, 17, 1, 256, 11, ragged="all"), _step("m3_ragged", 2, 5, 64, 4, 17, 1, 256, 15, ragged="tail"),
              _step("m3_cfg", 8, 16, 128, 8, 17, 1, 224 * 224, 12),
              _step("m3_odd", 3, 7, 136, 8, 122, 2, 256, 13), _step("m3_wide", 2, 4, 1024, 8, 17, 1, 256, 14)]
STEP_BY_TAG = {c["tag"]: c for c in STEP_CASES}
SEAM_VS_COMPOSED = [(2, 5, 136), (2, 4, 1024)]
VAL_TAGS = ("m3_tiny", "m3_odd")


def pad_idx(c):
    return c["n_class"] + 1


def make_args(c, **kw):
    import argparse
    d = dict(input_dim=2048, seg=True, anticipate=True, max_pos_len=64, input_type="i3d_transcript")
    d.update(kw)
    return argparse.Namespace(**d)


def build_model(c, device="cpu", dropout=False):
    """the model with oracle.synth's analytic parameter fill (named_parameters order) -> (model, p0 on the CPU)"""
    from r3d_amd.model.futr_safuser_tokenfusion3 import FUTR
    model = FUTR(c["n_class"], c["H"], pad_idx(c), torch.device(device), make_args(c), n_query=8, n_head=c["n_head"],
                 num_encoder_layers=1, num_decoder_layers=c["n_dec"], query_num=49, depth_pixels=c["pixels"],
                 gaze_dim=c["gaze_dim"])
    p0 = params_of(c, model)
    model.load_state_dict(p0, strict=False)
    model.r3d_dropout_enabled = dropout
    return (model.to(device) if device != "cpu" else model), p0


def params_of(c, model):
    names = [(n, tuple(p.shape)) for n, p in model.named_parameters()]
    return {n: torch.from_numpy(v) for n, v in synth.fill_state(names).items()}


def batch(c, seed=None, B=None, S=None):
    """[features, depth, past_label, trans_dur_future, trans_future_target, gaze] as torch tensors.  ragged "all": clip 0 ends
    in two padded frames and clip 1's past labels are ALL padding -- every key of its cross-attention is masked, so its
    anticipation rows are NaN in the reference's arithmetic (softmax over an empty set) and in the kernels' alike, and so is the
    loss.  ragged "tail": the same shape with clips of different lengths and no clip padded whole (clip 0 ends in two padded
    frames, clip 1 in three): every quantity of the step is finite and compared."""
    seed = c["seed"] if seed is None else seed
    B, S = B or c["B"], S or c["S"]
    side = int(round(c["pixels"] ** 0.5))
    assert side * side == c["pixels"]
    pad = pad_idx(c)
    feats, depth, lab, dur, tgt = synth.make_batch(B, S, c["n_class"], pad, seed, depth_hw=(side, side), zero_mean_depth=True)
    if c["ragged"]:
        lab[0, S - 2:] = pad
        if c["ragged"] == "all":
            lab[1, :] = pad
        else:
            lab[1, S - 3:] = pad
            lab[1, :S - 3] = np.where(lab[1, :S - 3] == pad, 0, lab[1, :S - 3])
    # gaze coordinates centred on the image, in [-1, 1): a channel of the gaze embedding is then live on some frames and dead
    # on others, as the other two embeddings' are (a track in [0, 1) leaves over a quarter of the channels dead on EVERY frame,
    # and the validation scores of more than k channels tied at exactly zero)
    gaze = synth.symmetric(B * S * c["gaze_dim"], ((seed & 0xFFFFFF) << 8) + 0x51).reshape(B, S, c["gaze_dim"])
    return [torch.from_numpy(np.ascontiguousarray(x)) for x in (feats, depth, lab, dur, tgt, gaze)]


def adamw_first_step(p, g, lr, wd, dtype):
    """torch.optim.AdamW's first step from zero moments, in `dtype`"""
    p, g = p.to(dtype), g.to(dtype)
    m, v = (1 - 0.9) * g, (1 - 0.999) * g * g
    return p * (1 - lr * wd) - lr * (m / (1 - 0.9)) / ((v / (1 - 0.999)).sqrt() + 1e-8)


def post_tolerance(p, g, grad_tol_abs, lr):
    """Element-wise absolute tolerance of a parameter after AdamW's first step (the rule of tests/l3_cases.py): the first step
    moves an element by u(g) = lr g / (|g| + 1e-8), whose slope reaches lr / 1e-8 at g = 0, so the gradient's tolerance is
    propagated through the steepest slope of u within grad_tol_abs of g, at most 2 lr, plus 8 float32 epsilon of |p| + lr."""
    g = g.detach().double().abs()
    slope = lr * 1e-8 / ((g - grad_tol_abs).clamp_min(0.0) + 1e-8) ** 2
    return (slope * grad_tol_abs).clamp_max(2 * lr) + 8 * EPS32 * (p.detach().double().abs() + lr)


# A loss is ONE float32 number.  The error of its float32 restatement in a single evaluation lies anywhere between 0 and a few
# roundings -- measured here between 3e-9 and 1e-6 for the same quantity, depending on the case, the order of the clips and the
# host's BLAS threads -- and where it happens to fall below one rounding, 8 x it is a bound no float32 evaluation can be held
# to: the float32 nearest to the exact value is itself up to 2^-24 away.  So the restatement's error of a scalar counts as at
# least that one rounding (from the format, not from any kernel's figures; tests/erank_tall_cases.py sets its SIGMA_FLOOR the
# same way).  The NaN losses of the all-padding case are compared as NaN and take no tolerance.  Tensors take no floor.
SCALAR_FLOOR = 2.0 ** -24
ZERO_GRAD = "fc_len.bias"       # true gradient 0: normalize_duration divides exp(duration) by its sum over the clip's queries
LOSS_KEYS = ("loss_seg", "loss_action", "loss_dur", "loss")
_STEP_REF = {}


def step_reference(c, p0, erank_weight=0.0):
    """dict(out, res, grads, post: float64; tol: {quantity: 8 x the float32 restatement's error}; live), once per case.
    Quantities: the three outputs, the three losses and their sum, "grad::name" and "post::name" of every live parameter."""
    key = (c["tag"], erank_weight)
    if key in _STEP_REF:
        return _STEP_REF[key]
    b, pad = batch(c), pad_idx(c)
    out, res, grads, aux = MO.step(p0, b, pad, c["n_head"], c["n_dec"], torch.float64, erank_weight)
    # the float32 restatement in two summation orders: the clips as given and in reversed order (every mean over the batch's
    # rows and every weight gradient then adds its terms the other way round); the larger error of the two counts.  A scalar
    # such as a loss is ONE float32 number, whose error in a single evaluation is anything between 0 and a few roundings
    o32, r32, g32, _ = MO.step(p0, b, pad, c["n_head"], c["n_dec"], torch.float32, erank_weight)
    of, rf, gf, _ = MO.step(p0, [t.flip(0) for t in b], pad, c["n_head"], c["n_dec"], torch.float32, erank_weight)
    of = {k: v.flip(0) for k, v in of.items()}
    tol = {k: MARGIN * max(rel_err(o32[k], out[k]), rel_err(of[k], out[k])) for k in out}
    for k in LOSS_KEYS:
        tol[k] = MARGIN * max(rel_err(r32[k], res[k]), rel_err(rf[k], res[k]), SCALAR_FLOOR)
    live = [n for n in grads if n.startswith(MO.LIVE_PREFIXES)]
    post, tol_abs_of = {}, {}
    S = c["S"]
    for n in live:
        g64, g_32, pn = grads[n], g32[n], p0[n]
        if n == "pos_embedding":
            g64, g_32, pn = g64[:, :S], g_32[:, :S], pn[:, :S]
        g_f = gf[n][:, :S] if n == "pos_embedding" else gf[n]
        tol["grad::" + n] = MARGIN * max(rel_err(g_32, g64), rel_err(g_f, g64))
        finite = g64[torch.isfinite(g64)]
        gmax = float(finite.abs().max()) if finite.numel() else 0.0
        tol_abs = tol["grad::" + n] * gmax
        if n == ZERO_GRAD:
            # the rounding of a cancelling sum over the B Q duration rows: 64 float32 epsilon of fc.bias's largest gradient
            # (the same rows, the other columns) ABSOLUTE; as a relative bound it is expressed in this tensor's own (tiny)
            # float64 scale (the rule of tests/l3_cases.py)
            fb = grads["fc.bias"][torch.isfinite(grads["fc.bias"])]
            tol_abs = 64 * EPS32 * (float(fb.abs().max()) if fb.numel() else 0.0)
            tol["grad::" + n] = tol_abs / max(gmax, 1e-300)
        tol_abs_of[n] = tol_abs
        post[n] = adamw_first_step(pn, g64, c["lr"], c["wd"], torch.float64)
        tol["post::" + n] = post_tolerance(pn, torch.nan_to_num(g64), tol_abs, c["lr"])
    _STEP_REF[key] = dict(out=out, res=res, grads=grads, post=post, tol=tol, tol_abs=tol_abs_of, live=live, aux=aux, batch=b)
    return _STEP_REF[key]


def validation_reference(c, p0, S=None):
    """the float64 validation forward (mode 'val': mean |x| scores, no key padding mask) with the float32 restatement's
    tolerances and its selection scores"""
    b, pad = batch(c, S=S), pad_idx(c)
    p64 = {n: v.double() for n, v in p0.items()}
    p32 = {n: v.float() for n, v in p0.items()}
    with torch.no_grad():
        o64, a64 = MO.forward(p64, (b[0], b[2]), b[1], b[5], "val", pad, c["n_head"], c["n_dec"])
        o32, a32 = MO.forward(p32, (b[0], b[2]), b[1], b[5], "val", pad, c["n_head"], c["n_dec"])
    tol = {k: MARGIN * rel_err(o32[k], o64[k]) for k in o64}
    # the scores are column means of |embedding|: their tolerance is that of the float32 embeddings' scores against float64's
    s64 = [x.reshape(-1, c["H"]).abs().mean(dim=0) for x in (a64["rgb_embed"], a64["depth_embed"], a64["gaze_embed"])]
    s32 = [x.reshape(-1, c["H"]).abs().mean(dim=0) for x in (a32["rgb_embed"], a32["depth_embed"], a32["gaze_embed"])]
    score_tol = [MARGIN * rel_err(a, b_) * float(b_.max()) for a, b_ in zip(s32, s64)]
    return dict(out=o64, aux=a64, tol=tol, scores=s64, score_tol=score_tol, batch=b)


def selection_gap(ref, H):
    """the smallest, over the three modalities, of (k-th to (k+1)-th smallest score gap) / (4 x the score tolerance):
    admissible above 1 (a float32 implementation then selects the same k = H // 4 channels)"""
    k = H // 4
    worst = np.inf
    for s, t in zip(ref["scores"], ref["score_tol"]):
        v = torch.sort(s.double())[0]
        worst = min(worst, float(v[k] - v[k - 1]) / max(4 * t, 1e-300))
    return worst
