"""The cases and the digests of tests/golden/attention_bits_parent.json: the two lse attention cores run forward then backward
through the r3d_amd.ops wrappers on operands seeded on the CPU, and the SHA-256 of the bytes of o, lse, delta, dq, dk and dv.
tests/golden/make_golden_attention_bits.py wrote the file at the commit before csrc/attention_lse.h;
tests/test_attention_bits_gpu.py holds the kernels to it, bit for bit.

Cases: every row of tests/splitk_cases.ROWS on the split-key core (operands as tests/test_attention_splitk_gpu.py lays them
out), the SQUARE rows of tests/test_tiled_attention_gpu.py and its rectangular case on the tiled core (as that test lays
them out)."""
import hashlib

import torch

from tests import splitk_cases as SC

NAMES = ("o", "lse", "delta", "dq", "dk", "dv")


def cases(chunk_of=None):
    """[(id, core, Lq, Lk, dh, heads, drop, mask)]; chunk_of is ops.mha_splitk_chunk (None: a split-key row's Lk stays as
    tests/splitk_cases.py writes it: for the ids alone).  mask None: the tiled test's labels."""
    from tests.test_tiled_attention_gpu import SQUARE
    out = []
    for row in SC.ROWS:
        lk, Lq, dh, heads, drop, mask = row
        Lk = SC.resolve(lk, dh, chunk_of) if chunk_of else lk
        out.append(("splitk-" + SC.row_id(row), "splitk", Lq, Lk, dh, heads, drop, mask))
    for S, dh, heads, drop in SQUARE:
        out.append((f"tiled-S{S}-dh{dh}x{heads}-{'drop' if drop else 'nodrop'}", "tiled", S, S, dh, heads, drop, None))
    out.append(("tiled-rect-Lq70-Lk133-dh16x8-drop", "rect", 70, 133, 16, 8, True, None))
    return out


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(ops, case):
    """{name: sha256} of one forward + backward of the case."""
    from tests.test_attention_splitk_gpu import grad_buffers, problem, run_splitk
    from tests.test_query_kernels_gpu import rnd, strided
    from tests.test_tiled_attention_gpu import B, keep_mask, labels, run_tiled
    _, core, Lq, Lk, dh, heads, drop, mask = case
    H = heads * dh
    if core == "splitk":
        q, kv, d_o, lab, keep, dsc, _ = problem(Lk, Lq, dh, heads, drop, mask, ops.mha_splitk_chunk(Lk, dh))
        kvd = kv.cuda()
        dq, _, dkv, _ = grad_buffers(Lq, Lk, H)
        dk, dv = dkv[:, :H], dkv[:, H:]
        o, lse, delta = run_splitk(ops, q.cuda(), kvd[:, :H], kvd[:, H:], d_o.cuda(), heads, dh, Lq, Lk, dq, dk, dv,
                                   key_labels=lab.cuda(), keep=keep.cuda() if drop else None, dsc=dsc)
    elif core == "tiled":
        S = Lq
        qkv, d_o, lab = rnd(B * S, 3 * H, seed=S * 7 + dh).cuda(), rnd(B * S, H, seed=3).cuda(), labels(S).cuda()
        keep, dsc = keep_mask(heads, S, S, drop)
        sl = lambda t: (t[:, :H], t[:, H:2 * H], t[:, 2 * H:])      # noqa: E731
        dq, dk, dv = sl(torch.full((B * S, 3 * H), float("nan"), device="cuda"))
        o, lse, delta = run_tiled(ops, *sl(qkv), d_o, heads, dh, S, S, dq, dk, dv, key_labels=lab,
                                  keep=keep.cuda() if drop else None, dsc=dsc)
    else:
        q, kv, d_o = rnd(B * Lq, H, seed=11), rnd(B * Lk, 2 * H, seed=12), rnd(B * Lq, H, seed=13)
        keep, dsc = keep_mask(heads, Lq, Lk, True)
        qd, _ = strided(q, H + 12, 4)
        kvd = kv.cuda()
        dod, _ = strided(d_o, H + 4, 4)
        zq, zk = torch.zeros(B * Lq, H), torch.zeros(B * Lk, H)
        (dq, _), (dk, _), (dv, _) = strided(zq, H + 9, 5), strided(zk, 2 * H + 7, 3), strided(zk, H + 16, 16)
        o, lse, delta = run_tiled(ops, qd, kvd[:, :H], kvd[:, H:], dod, heads, dh, Lq, Lk, dq, dk, dv,
                                  key_labels=labels(Lk).cuda(), keep=keep.cuda(), dsc=dsc)
    torch.cuda.synchronize()
    return {n: sha(t) for n, t in zip(NAMES, (o, lse, delta, dq, dk, dv))}
