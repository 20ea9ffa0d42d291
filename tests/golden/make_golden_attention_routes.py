#!/usr/bin/env python3
"""Records, on the CPU (the predicates are host-only), which attention core serves which shape:

    python tests/golden/make_golden_attention_routes.py [OUT.json]

It ran at the commit before r3d_amd/attention.py, where engine.cross_attention_route and engine_unsup.query_attention_route
each stated the rule; tests/test_attention_routes_cpu.py holds the module's rule and the kept wrappers to the recording.  The
file is not regenerated.

  cross        [Q, S, dh, train, long, route]: cross_attention_route over Q x dh x S x train x long, S among 1, 64, 65, the
               S x S core's last clip for (Q, dh, train), the one after it, and 2000
  query        [S, H, heads, train, long, route]: query_attention_route over the same dh (8 heads) and S, the core's last
               clip being that of the S x S shape
  max_clip     [H, heads, Q, train, long, S]: engine.max_clip_len at max_pos_len 2000 for the (H, heads) of tests/width_cases.py
  max_query    [H, heads, train, long, S]: engine_unsup.max_query_clip_len for those of tests/query_cases.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

QS, DHS, HEADS, MAX_POS = (1, 8, 16, 17, 24), (1, 5, 16, 25, 64, 128, 129), 8, 2000


def last_true(ok, hi=1 << 16):
    lo = 0
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid - 1)
    return lo


if __name__ == "__main__":
    from r3d_amd import build, engine as E, engine_unsup as U, ops
    from tests import query_cases as QC, width_cases as WC
    build.build(verbose=False)
    flags = [(t, f) for t in (False, True) for f in (False, True)]
    rec = dict(cross=[], query=[], max_clip=[], max_query=[])
    for dh in DHS:
        for train, long in flags:
            for Q in QS:
                last = last_true(lambda S: ops.mha_core_supported(Q, S, dh, train))
                for S in sorted({1, 64, 65, last, last + 1, 2000} - {0}):
                    rec["cross"].append([Q, S, dh, train, long, E.cross_attention_route(Q, S, dh, train, long)])
            last = last_true(lambda S: ops.mha_core_supported(S, S, dh, train))
            for S in sorted({1, 64, 65, last, last + 1, 2000} - {0}):
                rec["query"].append([S, HEADS * dh, HEADS, train, long, U.query_attention_route(S, HEADS * dh, HEADS, train, long)])
    for H, heads in sorted({(c.H, c.heads) for c in WC.CASES}):
        for train, long in flags:
            rec["max_clip"].append([H, heads, WC.Q, train, long, E.max_clip_len(H, heads, WC.Q, MAX_POS, train, long)])
    for H, heads in sorted({(c.H, c.heads) for c in QC.CASES}):
        for train, long in flags:
            rec["max_query"].append([H, heads, train, long, U.max_query_clip_len(H, heads, MAX_POS, train, long)])
    assert [9, 1024, 8, True, True, "tiled"] in rec["query"], "the 9-frame clip at hidden 1024 goes to the tiled core"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "attention_routes_parent.json")
    with open(out, "w") as fh:
        fh.write("{\n" + ",\n".join(f'"{k}": [\n' + ",\n".join(json.dumps(r) for r in v) + "\n]" for k, v in rec.items()) + "\n}\n")   # a row a line
    print({k: len(v) for k, v in rec.items()})
