#!/usr/bin/env python3
"""Records what one optimiser step launches, in order, for every case and path of tests/test_engine_launches_gpu.py on the
GPU:

    python tests/golden/make_golden_engine_launches.py [OUT.json]

The recording was taken while FusionEngine, AfftEngine, CnnEngine, RnnEngine and TcnEngine each carried their own step
plumbing (device scalars, head views, tick + flat AdamW); the test holds r3d_amd/engine_base.py, which they share now, to it.
It is not regenerated."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    from tests import test_engine_launches_gpu as T
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    rec = {}
    for name in T.CASES:
        rec[name] = {}
        for path in T.PATHS:
            mp = pytest.MonkeyPatch()
            rec[name][path] = T.record(name, path, mp)
            print(f"{name}/{path}: {len(rec[name][path])} items", flush=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=0)
        fh.write("\n")
