"""Seeded case table of the temporal auxiliary losses (r3d_amd/loss/temporal.py), shared by the fixture generator
(tests/golden/make_golden_temporal.py) and both test files.  Nothing is read from disk.

Run structures of one clip of T frames (``structure(pattern, T)`` -> the reference's list of (start, end)):

    a  one run over the clip
    b  every frame its own run
    c  run boundaries at 63/64 and 64/65 and a last run (65, T - 1) that spans the remaining tiles (three at T = 200)
    d  a length-1 run at a start > 0 (its only positive is the self pair)
    e  runs (0, 1), (2, 6), rest: the in-run "diagonal" removes (t = 4, c = 2) and not the self pair
    r  random run lengths of 1 .. 9 frames

The contrastive table has (b) from T = 64 up and not at T = 2: there the only positives are self pairs with p + 1e-5 = 1 - 2.5e-6,
so the whole loss (2.5e-6) is the residue of log(1 - 2.5e-6), which float32 resolves to 2^-24 = 6e-8: the reference's own form
run in float32 is 0.9 % off the float64 value there, 91 times the 1e-4 the GPU tests ask for.

A case lists one pattern per clip, so B = len(patterns): (f) is B = 3 with different structures, (g) ends with a one-run clip
(n_last comes from an earlier clip), (h) is one run per clip (M = 0)."""
import torch

PAD_LABEL = 18          # a label like any other


def structure(pattern, T, seed=0):
    if pattern == "a" or T == 1:
        return [(0, T - 1)]
    if pattern == "b":
        return [(t, t) for t in range(T)]
    if pattern == "c":
        assert T > 66
        return [(0, 63), (64, 64), (65, T - 1)]
    if pattern == "d":
        if T <= 3:
            return [(0, T - 2), (T - 1, T - 1)]
        return [(0, 2), (3, 3), (4, T - 1)]
    if pattern == "e":
        assert T >= 7
        return [(0, 1), (2, 6)] + ([(7, T - 1)] if T > 7 else [])
    assert pattern == "r"
    g = torch.Generator().manual_seed(1000 + seed)
    out, t = [], 0
    while t < T:
        n = min(int(torch.randint(1, 10, (1,), generator=g)), T - t)
        out.append((t, t + n - 1))
        t += n
    return out


def labels_of(intervals, T):
    """[B, T] int64 labels whose runs are exactly the intervals: neighbours differ, PAD_LABEL among the values"""
    vals = (3, PAD_LABEL, 0)
    lab = torch.empty(len(intervals), T, dtype=torch.int64)
    for b, clip in enumerate(intervals):
        for r, (s, e) in enumerate(clip):
            lab[b, s:e + 1] = vals[(r + b) % 3]
    return lab


def _c(name, kind, T, W, patterns, **kw):
    return dict(name=name, kind=kind, B=len(patterns), T=T, W=W, patterns=patterns, temperature=kw.pop("temperature", 0.07),
                zero=kw.pop("zero", False), **kw)


CONTRAST = [
    _c("n_t1_d1_a", "contrast", 1, 1, "a"),
    _c("n_t2_d5_a", "contrast", 2, 5, "a"),
    _c("n_t3_d16_d", "contrast", 3, 16, "d"),
    _c("n_t63_d20_e", "contrast", 63, 20, "e"),
    _c("n_t64_d48_b", "contrast", 64, 48, "b"),
    _c("n_t65_d128_d", "contrast", 65, 128, "d"),
    _c("n_t130_d136_c", "contrast", 130, 136, "c"),
    _c("n_t200_d256_c", "contrast", 200, 256, "c"),
    _c("n_t200_d48_a", "contrast", 200, 48, "a"),
    _c("n_t200_d48_f", "contrast", 200, 48, "cbe"),
    _c("n_t130_d1_f", "contrast", 130, 1, "bcd"),
    _c("n_t65_d16_g", "contrast", 65, 16, "eda"),
    _c("n_t64_d5_h", "contrast", 64, 5, "aaa"),
    _c("n_t130_d20_r", "contrast", 130, 20, "rrr"),
    _c("n_t65_d48_tau05", "contrast", 65, 48, "e", temperature=0.5),
    _c("n_t65_d48_tau001", "contrast", 65, 48, "e", temperature=0.01),
]

CLUSTER = [
    _c("c_t1_c1_a", "cluster", 1, 1, "a"),
    _c("c_t2_c5_b", "cluster", 2, 5, "b"),
    _c("c_t3_c48_d", "cluster", 3, 48, "d"),
    _c("c_t63_c122_e", "cluster", 63, 122, "e"),
    _c("c_t64_c256_b", "cluster", 64, 256, "b"),
    _c("c_t65_c5_d", "cluster", 65, 5, "d"),
    _c("c_t130_c48_c", "cluster", 130, 48, "c"),
    _c("c_t200_c48_b", "cluster", 200, 48, "b"),          # 200 runs: 7 x 7 pair tiles
    _c("c_t200_c1_a", "cluster", 200, 1, "a"),
    _c("c_t200_c122_f", "cluster", 200, 122, "cbe"),
    _c("c_t65_c48_g", "cluster", 65, 48, "eda"),          # n_last = 3 comes from clip 1
    _c("c_t64_c5_h", "cluster", 64, 5, "aaa"),            # M = 0: inter = 0
    _c("c_t130_c256_r", "cluster", 130, 256, "rrr"),
    _c("c_t8_c5_zero", "cluster", 8, 5, "d", zero=True),  # all-zero input: every pair at distance 0
]

# focal: pad = C - 1 unless C == 1; rows: random gold, every 5th row pad, `argmax_pad` forces one unmasked row's argmax onto
# the pad class, `oob` puts a label outside [0, C) on one unmasked row
FOCAL = [
    dict(name="f_n1_c1", kind="focal", N=1, C=1, pad=1, exclude=None, alpha=1.0, gamma=2.0, penalty=0.0, argmax_pad=False, oob=None),
    dict(name="f_n63_c6", kind="focal", N=63, C=6, pad=5, exclude=0, alpha=1.0, gamma=2.0, penalty=2.0, argmax_pad=True, oob=None),
    dict(name="f_n64_c48", kind="focal", N=64, C=48, pad=47, exclude=None, alpha=1.0, gamma=1.0, penalty=0.0, argmax_pad=True, oob=None),
    dict(name="f_n65_c122", kind="focal", N=65, C=122, pad=121, exclude=3, alpha=0.25, gamma=2.0, penalty=2.0, argmax_pad=True, oob=125),
    dict(name="f_n1000_c1000", kind="focal", N=1000, C=1000, pad=999, exclude=None, alpha=1.0, gamma=2.0, penalty=0.0, argmax_pad=False, oob=-2),
    dict(name="f_n1000_c6", kind="focal", N=1000, C=6, pad=5, exclude=2, alpha=1.0, gamma=1.0, penalty=2.0, argmax_pad=True, oob=None),
]

CASES = CONTRAST + CLUSTER + FOCAL
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"])) % 100003


def make(case):
    """contrast / cluster: (x [B, T, W] float32, intervals).  focal: (pred [N, C] float32, gold [N] int64)."""
    g = torch.Generator().manual_seed(_seed(case))
    if case["kind"] == "focal":
        N, C, pad = case["N"], case["C"], case["pad"]
        pred = 2.0 * torch.randn(N, C, generator=g)
        gold = torch.randint(0, C, (N,), generator=g)
        if pad < C:
            gold[4::5] = pad
        live = [i for i in range(N) if int(gold[i]) != pad and int(gold[i]) != case["exclude"]]
        if case["argmax_pad"] and live:
            pred[live[len(live) // 2], pad] += 20.0
        if case["oob"] is not None and live:
            gold[live[len(live) // 3]] = case["oob"]
        return pred, gold
    B, T, W = case["B"], case["T"], case["W"]
    x = torch.zeros(B, T, W) if case["zero"] else torch.randn(B, T, W, generator=g)
    return x, [structure(p, T, seed=b) for b, p in enumerate(case["patterns"])]
