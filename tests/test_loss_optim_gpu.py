"""losses.hip and optim.hip against the float64 references of tests/loss_optim_oracle.py: the loss launches over the case table of
tests/loss_cases.py, the one-launch decoder tail at a long clip / with dur_den / deferred, the loss reduction on its own and as
a rider of the AdamW launches, AdamW (flat at every launch plan, with its riders, the 2-D shard) and the Philox keep-masks.
Every assertion compares with a float64 reference or, bit for bit, with a sibling entry point that is itself compared with one
here.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import loss_cases as LC  # noqa: E402
from tests import loss_optim_oracle as R  # noqa: E402
from tests.test_engine_gpu import close_rel  # noqa: E402

SENT = 777.0          # what gradient buffers hold before a launch
SEED = 0x1234567890ABCDEF


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


def dev(t):
    return None if t is None else t.to("cuda")


def i64(*v):
    return torch.tensor(list(v), dtype=torch.int64, device="cuda")


def assert_losses(got, want, what):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-6), (what, got.tolist(), want.tolist())


# ----------------------------------------------------------------------------------------------------------
# 2. the loss launches over the case table
# ----------------------------------------------------------------------------------------------------------
_CASE = {}


def _case(name):
    """(tensors, float64 reference) of a case: computed once, never modified"""
    if name not in _CASE:
        c = LC.BY_NAME[name]
        t = LC.make(c)
        _CASE[name] = (t, R.losses64(t["seg"], t["act"], t["dur"], t["past_label"], t["target"], t["target_dur"], c["pad"],
                                     c["exclude"], Kseg=c["Kseg"], val_mode=c["val_mode"], dur_den=c["dur_den"],
                                     grad_scale=c["grad_scale"]))
    return _CASE[name]


class _Bufs:
    """device operands of one case in its layout: "inter" = anticipation logits and durations in one [BQ, K + 1] buffer (as the
    engines lay them out), seg contiguous; "sep" = every operand in a buffer of its own whose rows are wider than the logits"""

    def __init__(self, c, t):
        B, S, Q, K = c["B"], c["S"], c["Q"], c["K"]
        self.Ks = Ks = c["Kseg"] or K
        N, BQ = B * S, B * Q
        wide = 3 if c["layout"] == "sep" else 0
        act, dur = t["act"].reshape(BQ, K), t["dur"].reshape(BQ, 1)
        if c["layout"] == "inter":
            comb = torch.cat([act, dur], 1).contiguous().cuda()
            self.act, self.dur, self.ld_dur = comb[:, :K], comb[:, K:], K + 1
        else:
            a = torch.full((BQ, K + wide), 1e3)
            a[:, :K] = act
            du = torch.full((BQ, 2), 1e3)
            du[:, :1] = dur
            self.act, self.dur, self.ld_dur = a.cuda()[:, :K], du.cuda(), 2
        self.seg = None
        if c["seg"]:
            s = torch.full((N, Ks + wide), 1e3)
            s[:, :Ks] = t["seg"].reshape(N, Ks)
            self.seg = s.cuda()[:, :Ks]
        self.lab, self.tgt, self.td = dev(t["past_label"]), dev(t["target"]), dev(t["target_dur"])
        self.dur_den = None if c["dur_den"] is None else torch.tensor([c["dur_den"]], device="cuda")
        # d_seg is K wide at least: the `_kseg` entry point leaves the columns from Kseg on alone
        self.wseg, self.wact = max(Ks + wide, K), K + 1 + wide
        self.c = c

    def launch(self, ops, ws, ticks, kseg=None):
        """one launch into fresh outputs -> dict of CPU tensors; kseg: go through r3d_losses_fwd_bwd_kseg with that Kseg"""
        c, Ks = self.c, self.Ks
        B, S, Q, K = c["B"], c["S"], c["Q"], c["K"]
        loss = torch.full((4,), float("nan"), device="cuda")
        counts = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        kw = dict(val_mode=c["val_mode"], dur_den=self.dur_den, grad_scale=c["grad_scale"], ws=ws, tick_a=ticks[0:1],
                  tick_b=ticks[1:2])
        dseg = dact = None
        if c["grads"]:
            dact = torch.full((B * Q, self.wact), SENT, device="cuda")
            kw.update(d_act=dact[:, :K], d_dur=dact[:, K:], ld_ddur=self.wact)
            if c["seg"]:
                dseg = torch.full((B * S, self.wseg), SENT, device="cuda")
                kw.update(d_seg=dseg[:, :Ks] if self.wseg > Ks else dseg)
        a = (self.seg, self.act, self.dur, self.ld_dur, self.lab, self.tgt, self.td, B, S, Q, K)
        if kseg is None:
            ops.losses_fwd_bwd(*a, c["pad"], c["exclude"], loss, counts, **kw)
        else:
            ops.losses_fwd_bwd_kseg(*a, kseg, c["pad"], c["exclude"], loss, counts, **kw)
        torch.cuda.synchronize()
        return dict(loss=loss.cpu(), counts=counts.cpu(), d_seg=None if dseg is None else dseg.cpu(),
                    d_act=None if dact is None else dact.cpu())


def _same_bits(a, b, what):
    for k in ("loss", "counts", "d_seg", "d_act"):
        if a[k] is None:
            assert b[k] is None
        elif a[k].dtype == torch.float32:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs"
        else:
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("name", [c["name"] for c in LC.CASES])
def test_loss_launch_matches_float64(ops, name):
    c = LC.BY_NAME[name]
    t, ref = _case(name)
    B, S, Q, K = c["B"], c["S"], c["Q"], c["K"]
    bufs = _Bufs(c, t)
    Ks = bufs.Ks
    nws = ops.losses_ws_floats(B, S, Q)
    assert nws == 4 * LC.units(c) + 4
    ws = torch.zeros(nws, device="cuda")
    ticks = i64(5, 11)
    one = bufs.launch(ops, ws, ticks, kseg=c["Kseg"])
    assert ticks.tolist() == [6, 12], f"{name}: ticks after one launch"
    # ---- against float64
    assert_losses(one["loss"], ref["loss"], f"{name}: losses")
    assert one["counts"].tolist() == ref["counts"], f"{name}: counters"
    if not c["seg"]:
        assert one["loss"][0].item() == 0.0 and one["counts"][:2].tolist() == [0, 0], f"{name}: seg terms without seg"
    if c["grads"]:
        close_rel(one["d_act"][:, :K], ref["d_act"].reshape(B * Q, K), f"{name}: d_act", rtol=1e-3)
        close_rel(one["d_act"][:, K], ref["d_dur"].reshape(B * Q), f"{name}: d_dur", rtol=1e-3)
        assert bool((one["d_act"][:, K + 1:] == SENT).all()), f"{name}: d_act / d_dur wrote past their columns"
        dead = (t["target_dur"] != c["pad"]).sum(1) == 0                  # a clip without live durations: gradient exactly 0
        assert float(one["d_act"][:, K].reshape(B, Q)[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0, name
        if c["seg"]:
            close_rel(one["d_seg"][:, :Ks], ref["d_seg"].reshape(B * S, Ks), f"{name}: d_seg", rtol=1e-3)
            assert bool((one["d_seg"][:, Ks:] == SENT).all()), f"{name}: d_seg wrote past its {Ks} columns"
            ignored = ~ref["info"]["seg_valid"]
            assert float(one["d_seg"][:, :Ks][ignored].abs().max() if bool(ignored.any()) else 0.0) == 0.0, name
    # ---- the same launch again on the same scratch: the arrival counter was reset, the ticks go on
    assert ws[4 * LC.units(c):].view(torch.int32).tolist() == [0, 0, 0, 0], f"{name}: arrival counter after a launch"
    two = bufs.launch(ops, ws, ticks, kseg=c["Kseg"])
    assert ticks.tolist() == [7, 13], f"{name}: ticks after two launches"
    _same_bits(one, two, f"{name}: second launch on the same scratch")
    # ---- the `_kseg` entry point with Kseg == K is the plain one
    if c["Kseg"] is None:
        other = bufs.launch(ops, torch.zeros(nws, device="cuda"), i64(0, 0), kseg=K)
        _same_bits(one, other, f"{name}: _kseg(Kseg = K) vs the plain entry point")


# ----------------------------------------------------------------------------------------------------------
# 3. the one-launch decoder tail: a long clip, dur_den + grad_scale, deferred reduction
# ----------------------------------------------------------------------------------------------------------
def _tail(ops, H, B, S, K, dur_den=None, grad_scale=1.0, defer=False):
    """-> (outputs of r3d_decoder_tail_losses, float64 reference of the same composition)"""
    from oracle import synth
    from tests.test_row_widths_gpu import rnd, keep_mask, ln64, d, dd
    Q, pad = 8, K + 1
    rows, N, nh = B * Q, B * S, K + 1
    assert ops.tail_losses_supported(H, nh, Q, rows)
    _, _, lab, dur, tgt = [torch.from_numpy(x) for x in synth.make_batch(B, S, K, pad, 5, depth_hw=(4, 4))]
    x = rnd(rows, H, seed=1)
    g3, b3, gF, bF = 1 + 0.2 * rnd(H, seed=2), 0.1 * rnd(H, seed=3), 1 + 0.2 * rnd(H, seed=4), 0.1 * rnd(H, seed=5)
    wh, bh = rnd(nh, H, seed=6, scale=H ** -0.5), 0.1 * rnd(nh, seed=7)
    seg = rnd(N, K, seed=8)
    keep = keep_mask(rows, H, seed=9)
    dsc = 1 / 0.9
    # float64: the tail, the loss block, the tail's adjoint
    xd, g3d, b3d, gFd, bFd = dd(x), dd(g3), dd(b3), dd(gF), dd(bF)
    out = ln64(ln64(xd, g3d, b3d), gFd, bFd) @ wh.double().t() + bh.double()
    o64 = out.detach()
    ref = R.losses64(seg.view(B, S, K), o64[:, :K].reshape(B, Q, K), o64[:, K].reshape(B, Q), lab, tgt, dur, pad, 47,
                     dur_den=dur_den, grad_scale=grad_scale)
    dout = torch.cat([ref["d_act"].reshape(rows, K), ref["d_dur"].reshape(rows, 1)], 1)
    out.backward(dout)
    ref.update(out=o64, d_out=dout, dx=xd.grad, dx2=xd.grad * keep.double() * dsc, dgF=gFd.grad, dbF=bFd.grad, dg3=g3d.grad,
               db3=b3d.grad)
    f = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731
    nws = max(ops.layernorm_bwd_ws_floats(rows, H), 4)
    o = dict(t3=f(rows, H), m3=f(rows), r3=f(rows), tgtF=f(rows, H), mF=f(rows), rF=f(rows), out=f(rows, nh), d_seg=f(N, K),
             d_out=f(rows, nh), loss=torch.full((4,), float("nan"), device="cuda"),
             counts=torch.full((4,), -1, dtype=torch.int64, device="cuda"), dx=f(rows, H), dx2=f(rows, H), wsF=f(nws),
             ws3=f(nws), dgF=f(H), dbF=f(H), dg3=f(H), db3=f(H), ticks=i64(5, 11), ws=f(ops.losses_ws_floats(B, S, Q)))
    o["dur_den"] = None if dur_den is None else torch.tensor([dur_den], device="cuda")
    ops.decoder_tail_losses(x=d(x), g3=d(g3), b3=d(b3), gF=d(gF), bF=d(bF), w_head=d(wh), b_head=d(bh), t3=o["t3"], m3=o["m3"],
                            r3=o["r3"], tgtF=o["tgtF"], mF=o["mF"], rF=o["rF"], out=o["out"], seg=d(seg), past_label=d(lab),
                            target=d(tgt), target_dur=d(dur), B=B, S=S, Q=Q, K=K, pad_idx=pad, exclude_idx=47,
                            dur_den=o["dur_den"], grad_scale=grad_scale, d_seg=o["d_seg"], d_out=o["d_out"], loss_out=o["loss"],
                            counts=o["counts"], tick_a=o["ticks"][0:1], tick_b=o["ticks"][1:2], drop=d(keep), drop_scale=dsc,
                            dx=o["dx"], dx2=o["dx2"], wsF=o["wsF"], ws3=o["ws3"], ws=o["ws"], defer_finalize=defer)
    ops.layernorm_bwd_finalize(o["wsF"], rows, H, o["dgF"], o["dbF"])
    ops.layernorm_bwd_finalize(o["ws3"], rows, H, o["dg3"], o["db3"])
    torch.cuda.synchronize()
    return o, ref


def _assert_tail(o, ref, tag, losses=True):
    close_rel(o["out"], ref["out"], f"{tag}: out", rtol=1e-4)
    if losses:
        assert_losses(o["loss"], ref["loss"], f"{tag}: losses")
        assert o["counts"].tolist() == ref["counts"], tag
    for k in ("d_seg", "d_out", "dx", "dx2", "dgF", "dbF", "dg3", "db3"):
        want = ref[k].reshape(o[k].shape) if k == "d_seg" else ref[k]
        close_rel(o[k], want, f"{tag}: {k}", rtol=1e-3)


@pytest.mark.parametrize("H", [128, 136])
def test_tail_losses_long_clip(ops, H):
    """S > 64 with B*Q <= 64: the strided label scan beside the one-lane-per-entry duration mask"""
    o, ref = _tail(ops, H, 2, 70, 17)
    _assert_tail(o, ref, f"H{H} S70")
    assert o["ticks"].tolist() == [6, 12]


@pytest.mark.parametrize("H", [128, 136])
def test_tail_losses_dur_den_and_grad_scale(ops, H):
    o, ref = _tail(ops, H, 3, 7, 23, dur_den=5.5, grad_scale=0.25)
    _assert_tail(o, ref, f"H{H} dur_den gs")


@pytest.mark.parametrize("H", [128, 136])
def test_tail_losses_deferred_reduction(ops, H):
    now, ref = _tail(ops, H, 3, 7, 23)
    _assert_tail(now, ref, f"H{H} at once")
    late, _ = _tail(ops, H, 3, 7, 23, defer=True)
    assert late["ticks"].tolist() == [6, 12], "the deferred launch still ticks"
    assert bool(torch.isnan(late["loss"]).all()) and late["counts"].tolist() == [-1] * 4, "a deferred launch reduces nothing"
    ops.losses_finalize(ops.loss_finalize_job(late["ws"], 3, 7, 8, True, None, late["loss"], late["counts"]))
    torch.cuda.synchronize()
    _assert_tail(late, ref, f"H{H} deferred")
    assert torch.equal(late["loss"].view(torch.int32), now["loss"].view(torch.int32)), (late["loss"], now["loss"])
    assert torch.equal(late["counts"], now["counts"])
    for k in ("d_seg", "d_out", "dx", "dx2"):
        assert torch.equal(late[k], now[k]), k


# ----------------------------------------------------------------------------------------------------------
# 4. the loss reduction: on its own and as a rider of the AdamW launches
# ----------------------------------------------------------------------------------------------------------
FIN_SHAPES = {7: (1, 3, 3), 256: (4, 55, 8), 257: (1, 200, 56), 1000: (8, 100, 24)}      # units -> (B, S, Q)
ACC0 = ([1.5, 2.25, 0.125, 3.875], [10, 20, 30, 40])


def _partials(B, S, Q, has_seg, seed):
    """[units, 4] float32 as a loss launch leaves them: {loss, correct, valid, unused}; the duration units carry the mask count"""
    N, BQ = B * S, B * Q
    g = torch.Generator().manual_seed(seed)
    part = torch.zeros(N + BQ + B, 4)
    valid = (torch.rand(N + BQ, generator=g) < 0.8).float()
    part[:N + BQ, 2] = valid
    part[:N + BQ, 1] = valid * (torch.rand(N + BQ, generator=g) < 0.4).float()
    part[:N + BQ, 0] = valid * torch.rand(N + BQ, generator=g) * 5.0
    if not has_seg:
        part[:N] = 0.0
    part[N + BQ:, 0] = torch.rand(B, generator=g)
    part[N + BQ:, 2] = float(max(1, BQ // 2 + 1))
    part[:, 3] = float("nan")                          # never read
    return part


def _fin_job(ops, part_d, B, S, Q, has_seg, dur_den, with_acc):
    o = dict(loss=torch.full((4,), float("nan"), device="cuda"), counts=torch.full((4,), -1, dtype=torch.int64, device="cuda"),
             dur_den=None if dur_den is None else torch.tensor([dur_den], device="cuda"), acc_loss=None, acc_counts=None)
    if with_acc:
        o["acc_loss"] = torch.tensor(ACC0[0], dtype=torch.float64, device="cuda")
        o["acc_counts"] = torch.tensor(ACC0[1], dtype=torch.int64, device="cuda")
    o["job"] = ops.loss_finalize_job(part_d, B, S, Q, has_seg, o["dur_den"], o["loss"], o["counts"], o["acc_loss"], o["acc_counts"])
    return o


def _assert_fin(o, part, B, S, Q, has_seg, dur_den, with_acc, tag):
    want, wcounts = R.finalize64(part.numpy(), B, S, Q, has_seg, dur_den)
    got = o["loss"].cpu().double().numpy()
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (tag, got, want)
    assert o["counts"].tolist() == wcounts, tag
    if with_acc:
        assert o["acc_counts"].tolist() == [a + c for a, c in zip(ACC0[1], wcounts)], tag
        assert o["acc_loss"].cpu().numpy().tolist() == [a + float(x) for a, x in zip(ACC0[0], o["loss"].cpu().tolist())], tag


def _fin_same_bits(a, b, tag):
    assert torch.equal(a["loss"].view(torch.int32), b["loss"].view(torch.int32)), (tag, a["loss"], b["loss"])
    assert torch.equal(a["counts"], b["counts"]), tag
    if a["acc_loss"] is not None:
        assert torch.equal(a["acc_loss"].view(torch.int64), b["acc_loss"].view(torch.int64)), tag
        assert torch.equal(a["acc_counts"], b["acc_counts"]), tag


def _arena(n, seed):
    """p, g, m, v float32 [n] on the device and as numpy: non-zero moments, gradients of the size training sees (drawn on the
    device -- the references are computed from the values read back, so nothing depends on which values they are)"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(n, generator=gen, device="cuda")
    g = torch.randn(n, generator=gen, device="cuda") * 1e-2
    m = torch.randn(n, generator=gen, device="cuda") * 1e-3
    v = torch.rand(n, generator=gen, device="cuda") * 1e-4
    return [p, g, m, v], [t.cpu().numpy() for t in (p, g, m, v)]


@pytest.mark.parametrize("units", sorted(FIN_SHAPES))
def test_loss_reduction_alone_and_riding(ops, units):
    B, S, Q = FIN_SHAPES[units]
    assert B * (S + Q + 1) == units
    lr, st = torch.tensor([1e-3], device="cuda"), i64(7)
    arena, _ = _arena(1024, 3)
    off = i64(3)
    for has_seg in (True, False):
        part = _partials(B, S, Q, has_seg, units + int(has_seg))
        part_d = part.cuda()
        for dur_den in (None, 2.75):
            for with_acc in (False, True):
                tag = f"units{units} seg{int(has_seg)} den{dur_den} acc{int(with_acc)}"
                alone = _fin_job(ops, part_d, B, S, Q, has_seg, dur_den, with_acc)
                ops.losses_finalize(alone["job"])
                flat = _fin_job(ops, part_d, B, S, Q, has_seg, dur_den, with_acc)
                p, g, m, v = (a.clone() for a in arena)
                ops.adamw_flat(p, g, m, v, lr, st, weight_decay=5e-3, loss_fin=flat["job"])
                drop = _fin_job(ops, part_d, B, S, Q, has_seg, dur_den, with_acc)
                p, g, m, v = (a.clone() for a in arena)
                mask = torch.zeros(1000, dtype=torch.uint8, device="cuda")
                ops.adamw_flat_dropout(p, g, m, v, lr, st, mask, 0.1, SEED, off, weight_decay=5e-3, loss_fin=drop["job"])
                torch.cuda.synchronize()
                _assert_fin(alone, part, B, S, Q, has_seg, dur_den, with_acc, tag)
                _fin_same_bits(alone, flat, f"{tag}: riding in adamw_flat")
                _fin_same_bits(alone, drop, f"{tag}: riding in adamw_flat_dropout")


# ----------------------------------------------------------------------------------------------------------
# 5. AdamW
# ----------------------------------------------------------------------------------------------------------
# the hyper-parameters cross the C ABI as float32 (lr lives in a float32 device scalar): the reference takes those values
LR, WD, B1, B2, EPS = (float(np.float32(x)) for x in (1e-3, 5e-3, 0.9, 0.999, 1e-8))
GS = 0.5
M1 = 1048576          # 4096 workgroups x 256 lanes
FLAT_N4 = [1, 255, 256, 257, 1040, M1, M1 + 5, 2 * M1 + 1000, 3276800, 3276800 + 777]


def _assert_adam(got, host, step, tag):
    """got: the launch's p, m, v (numpy); host: the p, g, m, v it started from.  Margins of test_adamw_flat_matches_oracle.  The
    reference is evaluated in pieces of 2^18 elements on a few threads (numpy's loops are single-threaded)."""
    from concurrent.futures import ThreadPoolExecutor
    got = [a.reshape(-1) for a in got]
    host = [a.reshape(-1) for a in host]
    n, piece = host[0].size, 1 << 18

    def check(lo):
        sl = slice(lo, min(lo + piece, n))
        ref = R.adamw64(*(a[sl] for a in host), step, LR, WD, B1, B2, EPS, grad_scale=GS)
        out = []
        for name, a, r, atol in (("p", got[0][sl], ref[0], 1e-6), ("m", got[1][sl], ref[1], 1e-8), ("v", got[2][sl], ref[2], 1e-10)):
            err = np.abs(a.astype(np.float64) - r)
            bad = err > atol + 1e-5 * np.abs(r)
            out.append((name, int(bad.sum()), float(err.max())))
        return out
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(check, range(0, n, piece)))
    for i, name in enumerate("pmv"):
        nbad, worst = sum(r[i][1] for r in res), max(r[i][2] for r in res)
        assert nbad == 0, f"{tag}: {name}: {nbad}/{n} outside tol, max abs err {worst:.3e}"


@pytest.mark.parametrize("n4", FLAT_N4)
def test_adamw_flat_every_plan_matches_float64(ops, n4):
    n = 4 * n4
    (p0, g0, m0, v0), host = _arena(n, n4 % 1000)
    lr = torch.tensor([1e-3], device="cuda")
    for step in (1, 7, 100000):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        ops.adamw_flat(p, g0, m, v, lr, i64(step), weight_decay=5e-3, grad_scale=GS)
        torch.cuda.synchronize()
        _assert_adam([t.cpu().numpy() for t in (p, m, v)], host, step, f"n4 {n4} step {step}")
    assert np.array_equal(g0.cpu().numpy().view(np.int32), host[1].view(np.int32)), f"n4 {n4}: the gradient was written"


def test_adamw_flat_three_steps_match_float64(ops):
    n = 4 * (2 * M1 + 1000)
    (p, g, m, v), host = _arena(n, 17)
    lr, st = torch.tensor([1e-3], device="cuda"), i64(0)
    for step in (1, 2, 3):                                  # each step against float64 from the state the launch started from
        st.add_(1)
        gs = g * float(step)
        ops.adamw_flat(p, gs, m, v, lr, st, weight_decay=5e-3, grad_scale=GS)
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in (p, m, v)]
        _assert_adam(got, [host[0], gs.cpu().numpy(), host[2], host[3]], step, f"step {step}")
        host = [got[0], None, got[1], got[2]]


_PLAIN = {}


def _plain(ops, n4):
    """inputs and the plain r3d_adamw_flat result for them (compared with float64 in the test above), once per size"""
    if n4 not in _PLAIN:
        dev_in, _ = _arena(4 * n4, n4 % 1000)
        p, m, v = dev_in[0].clone(), dev_in[2].clone(), dev_in[3].clone()
        ops.adamw_flat(p, dev_in[1], m, v, torch.tensor([1e-3], device="cuda"), i64(7), weight_decay=5e-3, grad_scale=GS)
        torch.cuda.synchronize()
        _PLAIN[n4] = (dev_in, (p, m, v))
    return _PLAIN[n4]


DROP_BLOCK = 4 * 256 * 512          # mask bytes one pass of the rider's 512 mask workgroups covers


@pytest.mark.parametrize("with_fin", [False, True])
@pytest.mark.parametrize("n_mask", [1, 1023, DROP_BLOCK + 3, 2 * DROP_BLOCK + 5])
@pytest.mark.parametrize("n4", [257, M1 + 5])
def test_adamw_riders_keep_every_role_apart(ops, n4, n_mask, with_fin):
    (p0, g0, m0, v0), plain = _plain(ops, n4)
    lr, st, off = torch.tensor([1e-3], device="cuda"), i64(7), i64((1 << 32) + 3)
    B, S, Q = FIN_SHAPES[257]
    part = _partials(B, S, Q, True, 5)
    part_d = part.cuda()                                   # (a job holds addresses only: the partials must outlive it)
    buf = torch.full((n_mask + 1,), 7, dtype=torch.uint8, device="cuda")
    buf[n_mask] = 0xAB
    own = torch.full((n_mask,), 7, dtype=torch.uint8, device="cuda")
    ops.dropout_mask(own, 0.1, SEED, off)
    fin = _fin_job(ops, part_d, B, S, Q, True, None, True) if with_fin else None
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.adamw_flat_dropout(p, g0, m, v, lr, st, buf[:n_mask], 0.1, SEED, off, weight_decay=5e-3, grad_scale=GS,
                           loss_fin=fin["job"] if with_fin else None)
    torch.cuda.synchronize()
    tag = f"n4 {n4} n_mask {n_mask} fin{int(with_fin)}"
    for name, a, b in zip("pmv", (p, m, v), plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{tag}: {name} differs from the plain launch"
    assert torch.equal(buf[:n_mask], own), f"{tag}: the mask differs from r3d_dropout_mask's"
    assert np.array_equal(own.cpu().numpy(), R.philox_mask(n_mask, 0.1, SEED, (1 << 32) + 3)), f"{tag}: mask vs Philox"
    assert int(buf[n_mask]) == 0xAB, f"{tag}: the byte behind the mask was written"
    if with_fin:
        _assert_fin(fin, part, B, S, Q, True, None, True, tag)
        p2, m2, v2 = p0.clone(), m0.clone(), v0.clone()                 # ... and the AdamW + reduction launch without masks
        fin2 = _fin_job(ops, part_d, B, S, Q, True, None, True)
        ops.adamw_flat(p2, g0, m2, v2, lr, st, weight_decay=5e-3, grad_scale=GS, loss_fin=fin2["job"])
        torch.cuda.synchronize()
        for name, a, b in zip("pmv", (p2, m2, v2), plain):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{tag}: {name} of adamw_flat(loss_fin) differs"
        _fin_same_bits(fin, fin2, tag)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("rows,cols", [(1, 4), (5, 12), (128, 392), (132, 32800)])
def test_adamw_2d_shard(ops, rows, cols, wide):
    """a column block of a wider matrix gets the update r3d_adamw_flat gives the same values, bit for bit, and nothing else moves"""
    ld, c0 = (cols + 64, 32) if wide else (cols, 0)
    full, host = _arena(rows * ld, rows + cols)
    full, host = [t.view(rows, ld) for t in full], [a.reshape(rows, ld) for a in host]
    before = [t.clone() for t in full]
    lr, st = torch.tensor([1e-3], device="cuda"), i64(7)
    blk = [t[:, c0:c0 + cols] for t in full]
    flat = [t[:, c0:c0 + cols].contiguous().view(-1) for t in before]
    ops.adamw_2d(*blk, lr, st, weight_decay=5e-3, grad_scale=GS)
    ops.adamw_flat(*flat, lr, st, weight_decay=5e-3, grad_scale=GS)
    torch.cuda.synchronize()
    tag = f"{rows}x{cols} ld {ld}"
    _assert_adam([blk[i].cpu().numpy() for i in (0, 2, 3)], [np.ascontiguousarray(a[:, c0:c0 + cols]) for a in host], 7, tag)
    inside = torch.zeros(rows, ld, dtype=torch.bool, device="cuda")
    inside[:, c0:c0 + cols] = True
    for name, a, b in zip("pgmv", full, before):
        keep = inside if name != "g" else torch.zeros_like(inside)
        assert torch.equal(a.view(torch.int32)[~keep], b.view(torch.int32)[~keep]), f"{tag}: {name} changed outside the block"
    for name, i in (("p", 0), ("m", 2), ("v", 3)):
        a, b = blk[i].contiguous().view(-1).view(torch.int32), flat[i].view(torch.int32)
        ndiff = int((a != b).sum())
        assert ndiff == 0, f"{tag}: {name}: {ndiff}/{a.numel()} elements differ in bits from r3d_adamw_flat"


# ----------------------------------------------------------------------------------------------------------
# 6. dropout masks: r3d_dropout_mask is Philox4x32-10 with counter (i, offset) and key (seed), whatever grid wrote it
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4 * 256 * 2048 + 7])
def test_dropout_mask_is_philox(ops, n):
    buf = torch.empty(n + 1, dtype=torch.uint8, device="cuda")
    for offset in (0, 1, (1 << 32) + 3, None):
        words = R.philox_words(n, SEED, offset or 0)
        off_t = None if offset is None else i64(offset)
        for p in (0.0, 0.1, 0.5, 0.999):
            buf.fill_(7)
            buf[n] = 0xAB
            ops.dropout_mask(buf[:n], p, SEED, off_t)
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            want = R.mask_of_words(words, n, p)
            assert np.array_equal(got[:n], want), f"n {n} p {p} offset {offset}: {int((got[:n] != want).sum())} bytes differ"
            assert got[n] == 0xAB, f"n {n} p {p} offset {offset}: the byte behind the mask was written"
