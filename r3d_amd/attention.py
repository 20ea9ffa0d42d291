"""Which fp32 attention core serves an attention site ("sa", "ca" of a layer's buffer dict c), what the site keeps for its
backward, and the site's two launches; a caller hands over its operands and never branches on the route:
  "core"    csrc/attention.hip: keeps the probabilities c["p_<site>"] [B, heads, Lq, Lk]; bounded by its LDS;
  "splitk"  csrc/attention_splitk.hip: keeps c["lse_<site>"] [B, heads, Lq], chunk partials in c["ws_<site>"]; Lq <= 16;
  "tiled"   csrc/attention_tiled.hip: keeps c["lse_<site>"]; any Lq, Lk.
Kernels are called as attributes of the ops module: the tests patch them there and count the calls."""
from . import ops

ROUTES = ("core", "splitk", "tiled")


def pick(Lq, Lk, dh, train, allowed):
    """The first of ROUTES that the caller allows and whose own check (train: the backward's too) admits the shape, or None."""
    return next((r for r in ROUTES if r in allowed and getattr(ops, f"mha_{r}_supported")(Lq, Lk, dh, train)), None)


def long_clips_hint(Lq, Lk, dh, train, flagged):
    """For the message that refuses a shape without --long_clips: the core that the flag (the routes `flagged`) runs it on."""
    r = pick(Lq, Lk, dh, train, flagged)
    return f" (the {'split-key' if r == 'splitk' else 'tiled'} core runs this shape: --long_clips)" if r else ""


def longest(admits, hi):
    """The largest n in [0, hi] with admits(n), for a bound that only tightens as n grows (0: none)."""
    lo = 0
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if admits(mid) else (lo, mid - 1)
    return lo


def saved(route, site, f, B, heads, Lq, Lk, dh, train):
    """{key: f(*shape)} of what the site keeps; the split-key workspace serves the forward and, when training, the backward."""
    if route == "core":
        return {f"p_{site}": f(B, heads, Lq, Lk)}
    d = {f"lse_{site}": f(B, heads, Lq)}
    if route == "splitk":
        d[f"ws_{site}"] = f(max(ops.mha_splitk_ws_floats(B, heads, Lq, Lk, dh, False),
                                ops.mha_splitk_ws_floats(B, heads, Lq, Lk, dh, True) if train else 0))
    return d


def delta_buffer(route, f, B, heads, Lq, train):
    """A workspace's one delta, which the recomputing routes' backward fills: only off "core" and only when training."""
    return f(B, heads, Lq) if route != "core" and train else None


def thirds(t):
    """The q / k / v column thirds of a [rows, 3H] buffer."""
    H = t.shape[1] // 3
    return t[:, :H], t[:, H:2 * H], t[:, 2 * H:]


def forward(route, site, c, q, k, v, dims, drop_mask, drop_scale, **key_mask):
    """c[site + "_o"] = attention(q, k, v); dims = (B, heads, Lq, Lk, dh); key_mask: key_labels and pad_idx, or kpm."""
    kw = dict(drop_mask=drop_mask, drop_scale=drop_scale, **key_mask)
    o = c[site + "_o"]
    if route == "core":
        ops.mha_core_fwd(q, k, v, c["p_" + site], o, *dims, **kw)
    elif route == "splitk":
        ops.mha_splitk_fwd(q, k, v, o, c["lse_" + site], c["ws_" + site], *dims, **kw)
    else:
        ops.mha_tiled_fwd(q, k, v, o, c["lse_" + site], *dims, **kw)


def backward(route, site, c, q, k, v, d_o, dq, dk, dv, delta, dims, drop_mask, drop_scale, **key_mask):
    """Its adjoint.  The kept probabilities carry the key mask; the recomputing routes are given the forward's again."""
    if route == "core":
        return ops.mha_core_bwd(q, k, v, c["p_" + site], d_o, dq, dk, dv, *dims, drop_mask=drop_mask, drop_scale=drop_scale)
    kw = dict(drop_mask=drop_mask, drop_scale=drop_scale, **key_mask)
    o, lse = c[site + "_o"], c["lse_" + site]
    if route == "splitk":
        ops.mha_splitk_bwd(q, k, v, o, lse, d_o, delta, dq, dk, dv, c["ws_" + site], *dims, **kw)
    else:
        ops.mha_tiled_bwd(q, k, v, o, lse, d_o, delta, dq, dk, dv, *dims, **kw)
