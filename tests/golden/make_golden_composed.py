#!/usr/bin/env python3
"""Records the library entry points one training step calls, in order, for every case of
tests/test_composed_decoder_gpu.py on the GPU:

    python tests/golden/make_golden_composed.py [OUT.json]

Names only.  The recording was taken while engine_unsup, engine_l3 and engine_m3 each carried their own decoder loop; the
test holds r3d_amd/decoder_composed.py, which they share now, to it."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    from tests import test_composed_decoder_gpu as T
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    rec = {}
    for name in T.CASES:
        mp = pytest.MonkeyPatch()
        rec[name] = T.record(name, mp)
        print(f"{name}: {len(rec[name])} launches")
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=0)
        fh.write("\n")
