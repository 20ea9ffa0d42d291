#!/usr/bin/env python3
"""Records, on the CPU, the arena offsets and the state_dict keys of every model of tests/engine_base_cases.py:

    python tests/golden/make_golden_engine_base.py [OUT.json]

It ran at the commit before r3d_amd/engine_base.py and builds each arena the way that commit's engine did (ParamArena's
extra_live argument, engine_unsup._Arena overwriting is_live after the sort); tests/test_engine_base_cpu.py holds the live=
path every engine takes now to the recording.  It does not run on a later commit and the file is not regenerated."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    from r3d_amd import engine as E, engine_afft, engine_cnn, engine_l3, engine_m3, engine_rnn, engine_unsup
    from tests import engine_base_cases as C
    cpu = torch.device("cpu")
    fusion = lambda extra: lambda named: E.ParamArena(named, cpu, extra)                                      # noqa: E731
    ruled = lambda live: lambda named: E.ParamArena(named, cpu, live=live)                                    # noqa: E731
    build = {"tokenfusion": fusion(()), "bn": fusion(E.BN_LIVE_PREFIXES), "vary": fusion(E.VARY_LIVE_PREFIXES),
             "plain": fusion(E.PLAIN_LIVE_PREFIXES), "afft": ruled(engine_afft.is_live),
             "m3": lambda named: E.ParamArena(named, cpu, extra_live=engine_m3.M3_LIVE_EXTRA),
             "cnn": ruled(engine_cnn.is_live), "rnn": ruled(lambda n: n.startswith(engine_rnn.RNN_LIVE_PREFIXES)),
             "tcn": ruled(lambda n: True), "unsup_depth": lambda named: engine_unsup._Arena(named, cpu),
             "unsup_label": lambda named: engine_unsup._Arena(named, cpu),
             "l3": ruled(lambda n: n.startswith(engine_l3.LIVE_PREFIXES))}
    rec = {}
    for name, (make, _, _) in C.MODELS.items():
        model = make()
        keys = list(model.state_dict().keys())
        a = build[name](C.named_params(name, model))
        rec[name] = dict(state_keys=keys, n_live=a.n_live, n_total=a.n_total, live_names=a.live_names, offsets=C.offsets(a),
                         attach_live=[n for n, _ in model.named_parameters() if a.is_live(n)])
        print(f"{name}: {len(keys)} keys, {len(a.offsets)} parameters, {a.n_live} of {a.n_total} live")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "engine_base_parent.json")
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=0)
        fh.write("\n")
