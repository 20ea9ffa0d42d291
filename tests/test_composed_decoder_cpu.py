"""The dropout-pool layout of r3d_amd/decoder_composed.py on the CPU: for the site sizes of the three query engines (and of
the token-fusion engine, which calls the same function) at two decoder layers, every view starts at a multiple of 16 bytes,
no two views overlap, and order and offsets are those of the loop every engine's _Shape carried before the layout had one
home -- written out here as the expected value.  The order is behaviour: a site's Philox mask depends on its offset."""
import pytest
import torch

from r3d_amd import decoder_composed as DC

L, H, HEADS, Q = 2, 40, 5, 8


def _sizes(own, B, rows, Tq, Tk):
    """{site: numel} as the engines' _Shape constructors spelled it: their own sites, then the layers in order."""
    sizes = dict(own)
    for l in range(L):
        sizes.update({f"sa_p{l}": B * HEADS * Tq * Tq, f"ca_p{l}": B * HEADS * Tq * Tk, f"d1_{l}": rows * H,
                      f"d2_{l}": rows * H, f"d3_{l}": rows * H, f"ff_{l}": rows * 4 * H})
    return sizes


def _expected(sizes):
    """the nine-line loop: (total bytes, [(site, offset, numel)])"""
    tot = sum((v + 15) // 16 * 16 for v in sizes.values())
    out, o = [], 0
    for k, v in sizes.items():
        out.append((k, o, v))
        o += (v + 15) // 16 * 16
    return tot, out


def _case(name):
    """(own sites, B, query rows, Tq, Tk): odd B and S, so that the site sizes are no multiples of 16"""
    B, S = 3, 5
    N, BQ = B * S, B * Q
    return {"unsup": (dict(pe_rgb=N * H, pe_dep=N * H), B, N, S, S), "l3": (dict(pe_rgb=N * H), B, BQ, Q, S),
            "m3": (dict(x0=3 * N * H), B, BQ, Q, S), "fusion": (dict(x0=2 * N * H), B, BQ, Q, S)}[name]


@pytest.mark.parametrize("name", ["unsup", "l3", "m3", "fusion"])
def test_pool_layout_is_the_engines_loop(name):
    own, B, rows, Tq, Tk = _case(name)
    sizes = {**own, **DC.decoder_drop_sizes(L, B, HEADS, H, rows, Tq, Tk)}
    want_sizes = _sizes(own, B, rows, Tq, Tk)
    assert list(sizes.items()) == list(want_sizes.items())                     # names, order and sizes
    assert any(v % 16 for v in sizes.values()), "the case exercises the rounding"
    pool, views = DC.drop_pool(sizes, torch.device("cpu"))
    tot, want = _expected(want_sizes)
    assert pool.dtype == torch.uint8 and pool.numel() == tot and bool((pool == 1).all())
    got = [(k, v.storage_offset(), v.numel()) for k, v in views.items()]
    assert got == want
    end = 0
    for k, o, n in got:
        assert o % 16 == 0 and o >= end, (k, o, end)                           # aligned, and past the previous view's end
        assert views[k].data_ptr() == pool.data_ptr() + o
        end = o + n
    assert end <= tot
