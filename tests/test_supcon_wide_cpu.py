"""Host-side checks of the supervised contrastive loss's wide route (257 <= D <= 2048): the admission tables of the library
and the module (none of them touches a GPU), the workspace function, the --wide_supcon flag and the RNN model's shape rule,
and the admission of every case of tests/supcon_wide_cases.py: float32 arithmetic alone, in the oracle's own formula, must
sit within one eighth of each bound the GPU test applies, so that a kernel has the other seven eighths."""
import pytest
import torch

from tests import supcon_oracle as SO, supcon_wide_cases as WC


@pytest.fixture(scope="module")
def ops():
    from r3d_amd import build
    build.build(verbose=False)                                   # (every check below is the library's own host-only one)
    from r3d_amd import ops as o
    return o


def test_wide_admission_table(ops):
    assert [ops.supcon_supported(d, wide=True) for d in (0, 1, 256, 257, 2048, 2049)] == [False, True, True, True, True, False]
    assert ops.supcon_supported(257) is False and ops.supcon_supported(257, wide=False) is False
    assert ops.supcon_supported(256) is True


def test_workspace_is_monotone_and_holds_the_statistics(ops):
    for normalize in (False, True):
        for N in (1, 64, 4096, 9136):
            sizes = [ops.supcon_ws_floats(N, D, normalize, wide=True) for D in (1, 256, 257, 512, 513, 1024, 2048)]
            assert sizes == sorted(sizes) and sizes[0] >= 4 * N + 4, (N, normalize, sizes)
            assert sizes[0] == sizes[1] == ops.supcon_ws_floats(N)           # D <= 256: the narrow launches, their workspace
        for D in (16, 257, 2048):
            sizes = [ops.supcon_ws_floats(N, D, normalize, wide=True) for N in (1, 2, 63, 64, 65, 4096, 9136)]
            assert sizes == sorted(sizes), (D, normalize, sizes)
    for N, D in ((130, 257), (9136, 2048)):                      # normalize stages the backward's dz
        plain, norm = ops.supcon_ws_floats(N, D, False, wide=True), ops.supcon_ws_floats(N, D, True, wide=True)
        assert plain == 4 * N + 4 and norm == plain + N * D
    assert ops.supcon_ws_floats(8, 2049, True, wide=True) == 0 and ops.supcon_ws_floats(0, 512, True, wide=True) == 0
    with pytest.raises(ValueError, match="width"):
        ops.supcon_ws_floats(8, wide=True)


def test_module_refusals_with_wide_are_host_only(ops):
    from r3d_amd.loss import SupConLoss
    from r3d_amd.loss import spc
    assert (spc.MAX_WIDTH, spc.MAX_WIDTH_WIDE) == (256, 2048)
    assert SupConLoss().wide is False and SupConLoss(wide=True).wide is True
    y = torch.arange(6)
    with pytest.raises(ValueError, match="2048"):
        SupConLoss(wide=True)(torch.randn(6, 1, 2049), y)
    with pytest.raises(ValueError, match="2048"):
        SupConLoss(wide=True)(torch.randn(6, 1, 3, 700), y)     # flattened: 2100 wide
    with pytest.raises(TypeError, match="no torch fallback"):
        SupConLoss(wide=True)(torch.randn(6, 1, 512), y)        # a CPU tensor
    with pytest.raises(ValueError, match=r"256.*wide=True"):    # without the keyword: today's message, and where to look
        SupConLoss()(torch.randn(6, 1, 512), y)
    with pytest.raises(TypeError):
        SupConLoss(0.07, "all", 0.07, None, False, True)        # keyword-only


def test_wide_supcon_flag_parses_and_is_off_by_default():
    from r3d_amd import opts
    assert opts.parser.parse_args([]).wide_supcon is False
    a = opts.parser.parse_args(["--wide_supcon", "--supcon_weight", "0.5"])
    assert a.wide_supcon is True and a.supcon_weight == 0.5


def test_rnn_shape_rule_with_wide_supcon():
    from r3d_amd.engine_rnn import check_rnn_shape
    check_rnn_shape(512, 8, wide=True, supcon_weight=0.1, wide_supcon=True)
    check_rnn_shape(1024, 8, wide=True, supcon_weight=0.1, wide_supcon=True)
    check_rnn_shape(128, 8, supcon_weight=0.1, wide_supcon=True)
    with pytest.raises(ValueError, match="wide_rnn"):           # hidden > 256 still needs the recurrence's own flag
        check_rnn_shape(512, 8, supcon_weight=0.1, wide_supcon=True)
    with pytest.raises(ValueError, match=r"supcon_weight.*256 columns.*--wide_supcon"):
        check_rnn_shape(512, 8, wide=True, supcon_weight=0.1)
    with pytest.raises(ValueError, match="hidden 1032"):        # the model's own limit stays
        check_rnn_shape(1032, 8, wide=True, supcon_weight=0.1, wide_supcon=True)


def test_engines_carry_the_flag_off_by_default():
    from r3d_amd.engine_cnn import CnnEngine
    from r3d_amd.engine_rnn import RnnEngine
    assert RnnEngine.wide_supcon is False and CnnEngine.wide_supcon is False


def rel(a, b):
    """tests.test_engine_gpu.close_rel's measure: max abs error over the reference's max abs"""
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-5)


@pytest.mark.parametrize("name", [c["name"] for c in WC.CASES])
def test_case_is_admitted_by_float32_arithmetic_alone(name):
    """The GPU test's bounds are 1e-4 (loss, lse) and 1e-3 (gradient) of the reference's scale.  The oracle's formula in
    float32 must be within one eighth of each at the case's shape."""
    case = WC.BY_NAME[name]
    x, y = WC.make(case)
    z = SO.contrast_rows(x)
    yo = WC.oracle_labels(case, y)
    kw = WC.oracle_kwargs(case)
    l64, g64, lse64, _ = SO.supcon_with_grad(z, yo, **kw)
    l32, g32, lse32 = WC.supcon_f32(z, yo, **kw)
    assert bool(torch.isfinite(l64)) and bool(torch.isfinite(g64).all())
    rows = torch.isfinite(lse64)
    figures = dict(loss=rel(l32.reshape(1), l64.reshape(1)), grad=rel(g32, g64),
                   lse=rel(lse32[rows], lse64[rows]) if bool(rows.any()) else 0.0)
    print(name, {k: f"{v:.2e}" for k, v in figures.items()})
    assert figures["loss"] <= 1e-4 / 8 and figures["lse"] <= 1e-4 / 8 and figures["grad"] <= 1e-3 / 8, figures


def test_case_list_covers_the_shapes_the_route_branches_on():
    shapes = {(c["bsz"] * c["V"], c["D"]) for c in WC.CASES}
    for nd in [(1, 260), (2, 257), (3, 1024), (63, 264), (64, 512), (65, 516), (130, 261), (130, 768), (130, 1024), (200, 520),
               (70, 2048), (200, 2048)]:
        assert nd in shapes
    assert all(256 < c["D"] <= 2048 for c in WC.CASES)
    x, y = WC.make(WC.BY_NAME["w_clustered_d512"])
    s = x[:, 0] @ x[:, 0].t()
    same = y[:, None] == y[None, :]
    assert float(s[same].min()) > 0.8 and float(s[~same].abs().max()) < 0.5      # scores span most of +-1 / T
