"""The cases of the supervised contrastive loss, shared by tests/golden/make_golden_supcon.py (the imported reference on
CPU), tests/test_supcon_cpu.py (the float64 restatement against those fixtures) and tests/test_supcon_gpu.py (the kernel
against the restatement).  Every input is generated here from a seed; nothing is read from a file.

A case: name, bsz, n_views V, width D, contrast mode, temperature T, base temperature Tb, the label rule, the ignore rule,
whether the rows arrive L2-normalised (`unit`), the module's `normalize` flag and the scale of unnormalised rows."""
import torch

IGNORE = 999            # the label value the ignore cases use as ignore_index


def _case(name, bsz, D, *, V=1, mode="all", T=0.07, Tb=0.07, labels="k5", ignore=None, unit=True, normalize=False, scale=1.0,
          seed=None):
    return dict(name=name, bsz=bsz, V=V, D=D, mode=mode, T=T, Tb=Tb, labels=labels, ignore=ignore, unit=unit,
                normalize=normalize, scale=scale, seed=seed)


# tile edges (1, 2, 3, 63, 64, 65, 130, 200 rows: one tile, its last row, the first row of the next, a partial third and
# fourth) crossed sparsely with widths on both sides of every LDS padding (16, 32, 128, 256) and of the MFMA k-step
# (up to 3 rows: one class, or five random classes would leave no positive pair)
EDGES = [_case(f"n{n}_d{d}", n, d, labels="one" if n <= 3 else "k5") for n, d in
         [(1, 16), (2, 1), (2, 256), (3, 5), (63, 20), (64, 128), (64, 1), (65, 136), (130, 256), (130, 5), (200, 16), (200, 136)]]

LABELS = [_case("one_class", 130, 16, labels="one"), _case("all_distinct", 130, 16, labels="distinct"),
          _case("k122_singletons", 130, 16, labels="k122"), _case("k17", 130, 16, labels="k17")]

TEMPS = [_case("t05_tb007", 130, 16, T=0.5, Tb=0.07), _case("t007_tb02", 65, 20, T=0.07, Tb=0.2)]

VIEWS = [_case("v2_all", 70, 20, V=2), _case("v2_one", 70, 20, V=2, mode="one"), _case("simclr", 70, 20, V=2, labels=None),
         _case("v2_one_t05", 33, 136, V=2, mode="one", T=0.5, Tb=0.07, labels="k17")]

IGNORED = [_case("ign_scattered", 150, 20, ignore="scattered"), _case("ign_tile1_row3", 150, 20, ignore="tile1"),
           _case("ign_all", 150, 20, ignore="all")]

# F.normalize inside the kernel, on rows of norm ~ sqrt(D) and ~ 3 sqrt(D)
NORMALIZE = [_case("normalize_raw", 130, 128, unit=False, normalize=True, scale=1.0),
             _case("normalize_raw_d20_ign", 150, 20, unit=False, normalize=True, scale=3.0, ignore="scattered")]

# the input on which the reference returns nan: its stabilising maximum is the diagonal |z_i|^2 / T
UNNORMALISED = [_case("raw_03_randn", 130, 128, unit=False, scale=0.3, seed=3)]

CASES = EDGES + LABELS + TEMPS + VIEWS + IGNORED + NORMALIZE + UNNORMALISED
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def make(case):
    """(features [bsz, V, D] float32, labels [bsz] int64 or None) of a case."""
    bsz, V, D = case["bsz"], case["V"], case["D"]
    seed = case["seed"] if case["seed"] is not None else 1000 + 7 * bsz + D + 31 * V
    g = torch.Generator().manual_seed(seed)
    x = case["scale"] * torch.randn(bsz * V, D, generator=g)
    if case["unit"]:
        x = torch.nn.functional.normalize(x, dim=1)
    x = x.view(bsz, V, D).float().contiguous()
    rule = case["labels"]
    if rule is None:
        return x, None
    if rule == "one":
        y = torch.full((bsz,), 4, dtype=torch.int64)
    elif rule == "distinct":
        y = torch.randperm(bsz, generator=g)
    else:
        y = torch.randint(0, int(rule[1:]), (bsz,), generator=g)
    ign = case["ignore"]
    if ign == "scattered":
        y[torch.rand(bsz, generator=g) < 0.43] = IGNORE
    elif ign == "tile1":
        y[64:128] = IGNORE
        y[3] = IGNORE
    elif ign == "all":
        y[:] = IGNORE
    return x, y


def module_kwargs(case):
    return dict(temperature=case["T"], contrast_mode=case["mode"], base_temperature=case["Tb"])


def oracle_kwargs(case):
    """keyword arguments of tests.supcon_oracle.supcon for the case's contrast rows"""
    return dict(A=case["bsz"] * (case["V"] if case["mode"] == "all" else 1), temperature=case["T"], base_temperature=case["Tb"],
                ignore_index=IGNORE if case["ignore"] else None, normalize=case["normalize"])


def oracle_labels(case, y):
    """labels of the contrast rows: y repeated per view, or the sample index in the SimCLR case"""
    bsz, V = case["bsz"], case["V"]
    return (torch.arange(bsz) if y is None else y).repeat(V)
