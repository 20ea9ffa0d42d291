#!/usr/bin/env python3
"""Records, on an MI355X, the output bits of the tiled and split-key attention cores over tests/attention_bits_cases.py:

    python tests/golden/make_golden_attention_bits.py [OUT.json]

It ran at the commit before csrc/attention_lse.h (the two cores' shared argument block); tests/test_attention_bits_gpu.py holds
the kernels to the recording.  Every case runs twice, and nothing is written unless the two runs give the same digests: the
kernels' headers promise reproducible bits.  The file is not regenerated."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    from r3d_amd import ops
    from tests import attention_bits_cases as BC
    rec = {}
    for case in BC.cases(ops.mha_splitk_chunk):
        first, second = BC.digests(ops, case), BC.digests(ops, case)
        if first != second:
            sys.exit(f"{case[0]}: two runs differ in {[n for n in BC.NAMES if first[n] != second[n]]}; nothing written")
        rec[case[0]] = first
        print(f"{case[0]}: o {first['o'][:12]} dq {first['dq'][:12]}", flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "attention_bits_parent.json")
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=0)
        fh.write("\n")
