"""The cases of the supervised contrastive loss's wide route (257 <= D <= 2048, csrc/supcon.hip), shared by
tests/test_supcon_wide_cpu.py (their admission: float32 arithmetic alone must sit well inside the bounds) and
tests/test_supcon_wide_gpu.py (the kernels against the float64 restatement, tests/supcon_oracle.py).  Built with
tests/supcon_cases.py's `_case` and `make`; every input is generated from a seed.

Shapes are the smallest at which the wide route can go wrong: the row-tile edges of the narrow cases (1, 2, 3, 63, 64, 65,
130, 200 rows) crossed with the chunk edges of the width (257 = one column into the second chunk of 256, 260 / 261 / 264
just past it, 512 = two full chunks, 516 / 520 into the third, 768 = three, 1024, 2048 = eight); 261 gives an odd row stride
and the scalar staging path."""
import torch

from tests import supcon_cases as SC
from tests.supcon_cases import _case

IGNORE = SC.IGNORE

EDGES = [_case(f"w_n{n}_d{d}", n, d, labels="one" if n <= 3 else "k5") for n, d in
         [(1, 260), (2, 257), (3, 1024), (63, 264), (64, 512), (65, 516), (130, 261), (130, 768), (130, 1024), (200, 520),
          (70, 2048), (200, 2048)]]

# F.normalize inside the kernel (the norm spans chunks), on rows of norm ~ sqrt(D) and ~ 3 sqrt(D)
NORMALIZE = [_case("w_normalize_raw_d512", 130, 512, unit=False, normalize=True, scale=1.0),
             _case("w_normalize_raw_d1032_ign", 150, 1032, unit=False, normalize=True, scale=3.0, ignore="scattered")]

VIEWS = [_case("w_v2_one_t05_d520", 33, 520, V=2, mode="one", T=0.5, Tb=0.07, labels="k17"),
         _case("w_simclr_d264", 70, 264, V=2, labels=None)]

# the inputs on which the reference returns nan: its stabilising maximum is the diagonal |z_i|^2 / T
UNNORMALISED = [_case("w_raw_03_randn_d1024", 130, 1024, unit=False, scale=0.3, seed=3),
                _case("w_raw_01_randn_d2048", 130, 2048, unit=False, scale=0.1, seed=5)]

OTHER = [_case("w_t05_d300", 130, 300, T=0.5, Tb=0.07), _case("w_ign_all_d264", 150, 264, ignore="all"),
         _case("w_all_distinct_d264", 130, 264, labels="distinct")]

# unit rows around their class mean: scores span most of +-1 / T, where random wide rows stay within about +-0.5
CLUSTERED = [dict(_case("w_clustered_d512", 130, 512, seed=17), clustered=0.3)]

CASES = EDGES + NORMALIZE + VIEWS + UNNORMALISED + OTHER + CLUSTERED
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

ADD_CASES = ["w_n130_d768", "w_v2_one_t05_d520", "w_normalize_raw_d512"]      # plain, 'one' mode, normalize
MODULE_CASES = ["w_n65_d516", "w_v2_one_t05_d520", "w_normalize_raw_d1032_ign", "w_raw_03_randn_d1024"]

oracle_kwargs, oracle_labels, module_kwargs = SC.oracle_kwargs, SC.oracle_labels, SC.module_kwargs


def make(case):
    """(features [bsz, V, D] float32, labels [bsz] int64 or None) of a case: tests.supcon_cases.make, and for the clustered
    case rows normalize(class_mean[y] + clustered * noise) on its labels."""
    x, y = SC.make({k: v for k, v in case.items() if k != "clustered"})
    if case.get("clustered"):
        g = torch.Generator().manual_seed(case["seed"] + 1)
        means = torch.nn.functional.normalize(torch.randn(int(y.max()) + 1, case["D"], generator=g), dim=1)
        noise = torch.nn.functional.normalize(torch.randn(x.shape[0], case["D"], generator=g), dim=1)
        x = torch.nn.functional.normalize(means[y] + case["clustered"] * noise, dim=1).view(x.shape).float().contiguous()
    return x, y


def supcon_f32(x, y, *, A=None, temperature=0.07, base_temperature=0.07, ignore_index=None, normalize=False):
    """tests.supcon_oracle.supcon's formula in float32 throughout: (loss, d loss / d x, lse [A]).  What rounding alone
    costs at a case's shape, before any kernel runs."""
    x = x.detach().float().requires_grad_(True)
    N = x.shape[0]
    A = N if A is None else A
    z = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) if normalize else x
    kept = torch.ones(N, dtype=torch.bool) if ignore_index is None else (y != ignore_index)
    s = (z[:A] @ z.t()) / temperature
    in_c = kept[None, :].expand(A, N) & ~torch.eye(N, dtype=torch.bool)[:A]
    pos = in_c & (y[:A, None] == y[None, :])
    P = pos.sum(1)
    lse = torch.logsumexp(s.masked_fill(~in_c, float("-inf")), dim=1)
    live = kept[:A] & (P > 0)
    pos_sum = (s * pos).sum(1)
    per_row = torch.zeros(A)
    if bool(live.any()):
        idx = live.nonzero().flatten()
        per_row = per_row.index_put((idx,), -(temperature / base_temperature) * (pos_sum[idx] / P[idx] - lse[idx]))
    loss = per_row.sum() / max(1, int(kept[:A].sum()))
    if loss.requires_grad:
        loss.backward()
    g = x.grad if x.grad is not None else torch.zeros_like(x)
    return loss.detach(), g, lse.detach()
