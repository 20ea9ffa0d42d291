"""Every kernel instance and branch of csrc/rowops.hip (tests/rowops_cases.py) through r3d_amd.ops against the float64
restatements of tests/rowops_oracle.py: LayerNorm forward and backward at every width instance and row-count regime under
a covering set of the backward's options, the split-K forward input, the multi-job launches (also bitwise against the
same jobs launched one by one), the batched finalize with its "rows < 0" convention, RowsumGroup on both of its paths,
colsum, rowmod_sum and add_rowbcast.  Every output starts as NaN inside a NaN-filled buffer with two guard rows (vectors:
a guard element on each side): what a kernel must write is compared, everything else must still be NaN.  Each test prints
`[rowops] case tensor: err, scale, bound` before it asserts.  Bounds: tests/rowops_cases.py.  Needs an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")

from tests import rowops_cases as RC  # noqa: E402
from tests import rowops_oracle as RO  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


@pytest.fixture(scope="module")
def ws(ops):
    return ops.GemmWorkspace(DEV)


def sync():
    if DEV.startswith("cuda"):
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------
def place(t, lay=None, guard=2):
    """t [rows, H] as the slice [:rows, c0:c0 + H] of a [rows + guard, ld] device buffer, NaN elsewhere (255 for a byte
    mask).  lay = (ld, c0), None: dense.  Returns (slice, buffer, c0)."""
    rows, H = t.shape
    ld, c0 = (H, 0) if lay is None else lay
    buf = torch.full((rows + guard, ld), 255 if t.dtype == torch.uint8 else NAN, dtype=t.dtype)
    buf[:rows, c0:c0 + H] = t
    buf = buf.to(DEV)
    return buf[:rows, c0:c0 + H], buf, c0


def blank(rows, H, lay=None):
    return place(torch.full((rows, H), NAN), lay)


def vec(n, init=None):
    """a length-n output vector with a NaN guard element on each side: (view, buffer)"""
    buf = torch.full((n + 2,), NAN)
    if init is not None:
        buf[1:1 + n] = init
    buf = buf.to(DEV)
    return buf[1:1 + n], buf


def untouched(view, buf, c0):
    rows, H = view.shape
    b = buf.cpu()
    outside = torch.ones(b.shape, dtype=torch.bool)
    outside[:rows, c0:c0 + H] = False
    return bool(torch.isnan(b[outside]).all())


def vec_untouched(buf):
    b = buf.cpu()
    return bool(torch.isnan(b[0]) and torch.isnan(b[-1]))


def held(tag, name, got, want, tol):
    """element-wise |err| <= atol + rtol |ref|"""
    a, want = got.double().cpu(), want.double()
    assert a.shape == want.shape, (tag, name, tuple(a.shape), tuple(want.shape))
    err = (a - want).abs()
    scale = float(want.abs().max())
    print(f"[rowops] {tag} {name}: err {float(err.max()):.2e}, scale {scale:.2e}, bound {tol[1] + tol[0] * scale:.2e}")
    assert bool(torch.isfinite(a).all()), f"{tag} {name}: not finite"
    assert RC.elem_ok(err, want, tol) <= 1.0, f"{tag} {name}: max err {float(err.max()):.3e}"


def held_sum(tag, name, got, f32, f64):
    """max|err| <= max(8 e32, 2e-6 max|ref|)"""
    a = got.double().cpu()
    assert a.shape == f64.shape, (tag, name, tuple(a.shape), tuple(f64.shape))
    bound, e32 = RC.sum_bound(f32, f64)
    err = float((a - f64).abs().max())
    print(f"[rowops] {tag} {name}: err {err:.2e}, scale {float(f64.abs().max()):.2e}, bound {bound:.2e} (e32 {e32:.2e})")
    assert bool(torch.isfinite(a).all()), f"{tag} {name}: not finite"
    assert err <= bound, f"{tag} {name}: err {err:.3e} > bound {bound:.3e}"


def same_bits(one, two, tag):
    """bit for bit, the NaN of what is left unwritten included"""
    for n in one:
        if one[n] is not None:
            assert torch.equal(one[n].contiguous().view(torch.int32), two[n].contiguous().view(torch.int32)), f"{tag}: {n} differs"


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm forward + backward
# ---------------------------------------------------------------------------------------------------------------------
class LnBufs:
    """the device buffers of one LayerNorm site (an rowops_cases ln problem): operands placed, outputs NaN"""

    def __init__(self, p):
        rows, H, o, t = p["rows"], p["H"], p["o"], p["t"]
        lay = lambda n: RC.layout_of(o, n, H)         # noqa: E731
        self.p, self.guards, self.vguards = p, [], []
        self.gamma, self.beta = t["gamma"].to(DEV), t["beta"].to(DEV)
        for n in ("x", "dy", "dy2", "add1", "add2", "mask"):
            setattr(self, n, None if t[n] is None else place(t[n], lay(n))[0])
        for n, r in (("y", rows), ("dx", rows), ("dx2", rows if o["dx2"] else 0), ("pair", rows // 2 if o["pair_in"] else 0)):
            v = None
            if r:
                v, buf, c0 = blank(r, H, None if n == "pair" else lay(n))        # (pair_out is dense by contract)
                self.guards.append((n, v, buf, c0))
            setattr(self, n, v)
        for n, k in (("mean", rows), ("rstd", rows), ("dgamma", 0 if o["dgamma_none"] else H), ("dbeta", 0 if o["dgamma_none"] else H)):
            v = None
            if k:
                v, buf = vec(k)
                self.vguards.append((n, buf))
            setattr(self, n, v)
        self.partial = None

    def fwd_args(self):
        return dict(x=self.x, gamma=self.gamma, beta=self.beta, y=self.y, mean=self.mean, rstd=self.rstd, relu=self.p["o"]["relu"],
                    pair_out=self.pair)

    def bwd_args(self, ops):
        o = self.p["o"]
        if o["defer"] and self.partial is None:
            need = ops.layernorm_bwd_ws_floats(self.p["rows"], self.p["H"])
            self.need = need
            self.partial = torch.full((need + 2,), NAN, device=DEV)
        return dict(dy=self.dy, x=self.x, mean=self.mean, rstd=self.rstd, gamma=self.gamma, beta=self.beta, dx=self.dx, dgamma=self.dgamma,
                    dbeta=self.dbeta, pair_in=o["pair_in"], relu=o["relu"], dy2=self.dy2, add1=self.add1, add2=self.add2, dx2=self.dx2,
                    drop_mask=self.mask, drop_scale=RC.DROP_SCALE if o["dx2"] else 1.0, partial=self.partial)

    def outputs(self):
        return {n: getattr(self, n) for n in ("y", "mean", "rstd", "pair", "dx", "dx2", "dgamma", "dbeta", "partial")}

    def check(self, tag):
        p = self.p
        ref, ref32 = p["ref"], p["ref32"]
        for n in ref:
            if n in RC.LN_SUM_TENSORS and p["o"]["dgamma_none"]:
                continue
            got = getattr(self, n)
            assert got is not None, (tag, n)
            if n in RC.LN_SUM_TENSORS:
                held_sum(tag, n, got, ref32[n], ref[n])
            else:
                held(tag, n, got, ref[n], RC.ln_tol(n))
        for n, v, buf, c0 in self.guards:
            assert untouched(v, buf, c0), f"{tag}: wrote outside {n}"
        for n, buf in self.vguards:
            assert vec_untouched(buf), f"{tag}: wrote outside {n}"
        if self.partial is not None:
            part = self.partial.cpu()
            assert bool(torch.isnan(part[self.need:]).all()), f"{tag}: wrote past the partial pairs"
            if p["o"]["dgamma_none"] or self.need == 0:
                assert bool(torch.isnan(part).all()), f"{tag}: partial pairs written with no dgamma asked for"
            else:
                assert bool(torch.isfinite(part[:self.need]).all()), f"{tag}: partial pairs"


def launch_fwd(ops, b):
    a = b.fwd_args()
    head = [a.pop(n) for n in ("x", "gamma", "beta", "y", "mean", "rstd")]
    ops.layernorm_fwd(*head, **a)


def launch_bwd(ops, ws, b):
    a = b.bwd_args(ops)
    head = [a.pop(n) for n in ("dy", "x", "mean", "rstd", "gamma", "beta", "dx", "dgamma", "dbeta")]
    ops.layernorm_bwd(*head, ws=ws, **a)


def run_ln(ops, ws, p):
    b = LnBufs(p)
    launch_fwd(ops, b)
    launch_bwd(ops, ws, b)
    if b.partial is not None and b.dgamma is not None:
        ops.LnFinalizeGroup([(b.partial, p["rows"], p["H"], b.dgamma, b.dbeta)]).launch()
    sync()
    return b


LN_TWICE = set(RC.LN_IDS[::7])


@pytest.mark.parametrize("cid", RC.LN_IDS)
def test_layernorm_fwd_bwd_at_every_instance_and_option(ops, ws, cid):
    p = RC.ln_problem(cid)
    tag = f"ln {cid} [{' '.join(sorted(RC.flags_of(p['o']))) or 'plain'}]"
    b = run_ln(ops, ws, p)
    b.check(tag)
    if cid in LN_TWICE:
        same_bits(b.outputs(), run_ln(ops, ws, p).outputs(), tag + " second run")


@pytest.mark.parametrize("H", RC.SPLITK_H)
@pytest.mark.parametrize("nsplit", RC.SPLITK_NSPLIT)
def test_layernorm_fwd_splitk_input(ops, nsplit, H):
    rows = RC.SPLITK_ROWS
    for i, (bias, pre, pair) in enumerate(RC.SPLITK_VARIANTS):
        relu = bool(i & 1) != pair
        p = RC.splitk_problem(nsplit, H, bias, relu, pair)
        tag = f"splitk ns{nsplit} H{H} bias{int(bias)} pre{int(pre)} pair{int(pair)} relu{int(relu)}"

        def run():
            y, yb, yc = blank(rows, H, (H + 8, 4) if i % 2 else None)
            mean, meanb = vec(rows)
            rstd, rstdb = vec(rows)
            pre_o, preb, _ = blank(rows, H) if pre else (None, None, 0)
            pair_o, pairb, _ = blank(rows // 2, H) if pair else (None, None, 0)
            ops.layernorm_fwd(p["x"].to(DEV), p["gamma"].to(DEV), p["beta"].to(DEV), y, mean, rstd, relu=relu, pair_out=pair_o, nsplit=nsplit,
                              bias=None if p["bias"] is None else p["bias"].to(DEV), pre_out=pre_o, rows=rows, H=H)
            sync()
            assert untouched(y, yb, yc) and vec_untouched(meanb) and vec_untouched(rstdb), tag
            assert (pre_o is None or untouched(pre_o, preb, 0)) and (pair_o is None or untouched(pair_o, pairb, 0)), tag
            return dict(y=y, mean=mean, rstd=rstd, pre=pre_o, pair=pair_o)
        got = run()
        for n in ("pre", "y", "mean", "rstd", "pair"):
            if got[n] is not None:
                held(tag, n, got[n], p["ref"][n], RC.ln_tol(n))
        if i == 7:
            same_bits(got, run(), tag + " second run")


@pytest.mark.parametrize("njobs,H", RC.multi_cases())
def test_layernorm_multi_launches_equal_their_jobs_one_by_one(ops, ws, njobs, H):
    probs = [RC.multi_job(j, H) for j in range(njobs)]
    multi, single = [LnBufs(p) for p in probs], [LnBufs(p) for p in probs]
    ops.layernorm_fwd_multi([b.fwd_args() for b in multi])
    ops.layernorm_bwd_multi([b.bwd_args(ops) for b in multi])
    for b in single:
        launch_fwd(ops, b)
        launch_bwd(ops, ws, b)
    sync()
    for j, (m, s) in enumerate(zip(multi, single)):          # before the finalize: partial pairs included, NaN where unwritten
        same_bits(m.outputs(), s.outputs(), f"multi {njobs} jobs H{H} job{j} against its own launch")
    ops.LnFinalizeGroup([(b.partial, b.p["rows"], H, b.dgamma, b.dbeta) for b in multi]).launch()
    sync()
    for j, b in enumerate(multi):
        b.check(f"multi {njobs} jobs H{H} job{j} rows{b.p['rows']}")


# ---------------------------------------------------------------------------------------------------------------------
# batched finalize
# ---------------------------------------------------------------------------------------------------------------------
def test_batched_finalize_of_partial_pairs(ops):
    """rows = -n: exactly n partial pairs, widths 8, 1032 and 72 mixed under one max_H"""
    def run():
        jobs, bufs = [], []
        for n, H in RC.fin_jobs():
            p = RC.fin_problem(n, H)
            dg, dgb = vec(H)
            db, dbb = vec(H)
            jobs.append((p["ws"].to(DEV), -n, H, dg, db))
            bufs.append((dgb, dbb))
        ops.LnFinalizeGroup(jobs).launch()
        sync()
        return jobs, bufs
    jobs, bufs = run()
    again, _ = run()
    for (wsb, rows, H, dg, db), (dgb, dbb), two in zip(jobs, bufs, again):
        p = RC.fin_problem(-rows, H)
        tag = f"finalize {-rows} pairs H{H}"
        held_sum(tag, "dgamma", dg, p["ref32"]["dgamma"], p["ref"]["dgamma"])
        held_sum(tag, "dbeta", db, p["ref32"]["dbeta"], p["ref"]["dbeta"])
        assert vec_untouched(dgb) and vec_untouched(dbb), tag
        assert torch.equal(dg, two[3]) and torch.equal(db, two[4]), tag


def test_batched_finalize_after_deferred_backwards(ops, ws):
    """rows > 0: a one-block job is left exactly as layernorm_bwd wrote it; several blocks are reduced"""
    bufs = []
    for rows, H in RC.FIN_LN:
        b = LnBufs(RC.fin_ln_problem(rows, H))
        launch_fwd(ops, b)
        launch_bwd(ops, ws, b)
        bufs.append(b)
    sync()
    before = [(b.dgamma.clone(), b.dbeta.clone()) for b in bufs]
    ops.LnFinalizeGroup([(b.partial, b.p["rows"], b.p["H"], b.dgamma, b.dbeta) for b in bufs]).launch()
    sync()
    for b, (g0, b0) in zip(bufs, before):
        rows, H = b.p["rows"], b.p["H"]
        if ops.layernorm_bwd_ws_floats(rows, H) == 0:
            assert torch.equal(b.dgamma, g0) and torch.equal(b.dbeta, b0) and bool(torch.isfinite(g0).all()), (rows, H)
        else:
            assert bool(torch.isnan(g0).all()) and bool(torch.isnan(b0).all()), (rows, H)       # (deferred: nothing yet)
        b.check(f"finalize rows{rows} H{H}")


# ---------------------------------------------------------------------------------------------------------------------
# RowsumGroup
# ---------------------------------------------------------------------------------------------------------------------
def _rowsum_group(ops, g):
    jobs, keep = [], []
    for k in range(len(RC.RS_GROUPS[g])):
        p = RC.rs_problem(g, k)
        lay = RC.rs_layout(p["cols"], p["how"])
        s1 = place(p["x1"], lay["src1"])[0]
        s2 = None if p["x2"] is None else place(p["x2"], lay["src2"])[0]
        dst, dstb, c0 = blank(p["mod"], p["cols"], lay["dst"])
        for t, n in ((s1, "src1"), (s2, "src2"), (dst, "dst")):         # the layout is what the table says it is
            if t is not None:
                assert (t.data_ptr() % 16 == 0) == (lay[n][1] % 4 == 0) and t.stride(0) == lay[n][0], (n, lay[n])
        jobs.append((s1, s2, p["mod"], dst))
        keep.append((p, dst, dstb, c0))
    ops.RowsumGroup(jobs).launch()
    sync()
    return jobs, keep


@pytest.mark.parametrize("g", range(len(RC.RS_GROUPS)))
def test_rowsum_group_on_both_paths(ops, ws, g):
    jobs, keep = _rowsum_group(ops, g)
    for k, ((s1, s2, mod, dst), (p, _, dstb, c0)) in enumerate(zip(jobs, keep)):
        tag = f"rowsum_group {g}.{k} rows{p['rows']} cols{p['cols']} mod{mod} src2{int(s2 is not None)} {p['how']}"
        held_sum(tag, "dst", dst, p["ref32"], p["ref"])
        assert untouched(dst, dstb, c0), f"{tag}: wrote outside dst"
        if p["rows"] < mod:
            assert float(dst[p["rows"]:].abs().max()) == 0.0, f"{tag}: an empty residue class is not an exact 0"
        # the single launches on the same data
        one = torch.full((mod, p["cols"]), NAN, device=DEV)
        if mod == 1 and s2 is None:
            ops.colsum(s1, one[0], ws=ws)
        else:
            ops.rowmod_sum(s1, mod, one)
            if s2 is not None:
                ops.rowmod_sum(s2, mod, one, accumulate=True)
        sync()
        bound, _ = RC.sum_bound(p["ref32"], p["ref"])
        diff = float((dst.double() - one.double()).abs().max())
        print(f"[rowops] {tag} vs the single launch: err {diff:.2e}, scale {float(p['ref'].abs().max()):.2e}, bound {bound:.2e}")
        assert diff <= bound, tag
    if g == len(RC.RS_GROUPS) - 1:
        again, _ = _rowsum_group(ops, g)
        for a, b in zip(jobs, again):
            assert torch.equal(a[3], b[3]), f"rowsum_group {g}: second launch"


# ---------------------------------------------------------------------------------------------------------------------
# colsum, rowmod_sum, add_rowbcast
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", RC.SUM_ROWS)
def test_colsum(ops, ws, rows):
    for i, cols in enumerate(RC.COLSUM_COLS):
        p = RC.colsum_problem(rows, cols)
        x = place(p["x"], (cols + 3, 1) if i % 2 == 0 else None)[0]
        for acc in (False, True):
            tag = f"colsum rows{rows} cols{cols} acc{int(acc)} ld{x.stride(0) if rows > 1 else cols}"
            out, outb = vec(cols, p["out0"] if acc else None)
            ops.colsum(x, out, accumulate=acc, ws=ws)
            sync()
            held_sum(tag, "out", out, p["ref32_acc" if acc else "ref32"], p["ref_acc" if acc else "ref"])
            assert vec_untouched(outb), tag
            if rows == 4100 and cols == 513:
                out2, _ = vec(cols, p["out0"] if acc else None)
                ops.colsum(x, out2, accumulate=acc, ws=ws)
                sync()
                assert torch.equal(out, out2), f"{tag}: second launch"


@pytest.mark.parametrize("rows", RC.SUM_ROWS)
def test_rowmod_sum(ops, rows):
    for mod in RC.ROWMOD_MODS:
        for i, cols in enumerate(RC.ROWMOD_COLS):
            p = RC.rowmod_problem(rows, cols, mod)
            x = place(p["x"], (cols + 7, 3) if i == 0 else None)[0]
            for acc in (False, True):
                tag = f"rowmod_sum rows{rows} cols{cols} mod{mod} acc{int(acc)}"
                out, outb, c0 = place(p["out0"] if acc else torch.full((mod, cols), NAN), (cols + 5, 2))
                ops.rowmod_sum(x, mod, out, accumulate=acc)
                sync()
                held_sum(tag, "out", out, p["ref32_acc" if acc else "ref32"], p["ref_acc" if acc else "ref"])
                assert untouched(out, outb, c0), tag
                if mod > rows:                       # empty residue classes: an exact 0, or what was there
                    assert torch.equal(out[rows:].cpu(), p["out0"][rows:] if acc else torch.zeros(mod - rows, cols)), tag
                if rows == 4100 and mod == 5 and cols == 257:
                    out2 = place(p["out0"] if acc else torch.full((mod, cols), NAN), (cols + 5, 2))[0]
                    ops.rowmod_sum(x, mod, out2, accumulate=acc)
                    sync()
                    assert torch.equal(out, out2), f"{tag}: second launch"


@pytest.mark.parametrize("rows,cols,mod,has_x,in_place,strided", RC.BCAST_CASES)
def test_add_rowbcast(ops, rows, cols, mod, has_x, in_place, strided):
    """one float32 add: compared with a tolerance of zero"""
    x, add = RC.rnd(rows, cols, seed=rows + mod), RC.rnd(mod, cols, seed=rows + mod + 1)
    want = RO.add_rowbcast(x if has_x else None, add, mod, rows, torch.float32)
    tag = f"add_rowbcast {rows}x{cols} mod{mod} x{int(has_x)} inplace{int(in_place)} strided{int(strided)}"

    def run():
        xd, xb, xc = place(x, (cols + 8, 4) if strided else None)
        ad = place(add, (cols + 4, 3) if strided else None)[0]
        out, outb, oc = (xd, xb, xc) if in_place else blank(rows, cols, (cols + 12, 5) if strided else None)
        ops.add_rowbcast(xd if has_x else None, ad, mod, out)
        sync()
        assert untouched(out, outb, oc), tag
        return out
    got = run()
    err = float((got.cpu().double() - want.double()).abs().max())
    print(f"[rowops] {tag} out: err {err:.2e}, scale {float(want.abs().max()):.2e}, bound 0.00e+00")
    assert torch.equal(got.cpu(), want), tag
    assert torch.equal(run(), got), f"{tag}: second launch"
