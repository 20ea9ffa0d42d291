#!/usr/bin/env python3
"""Generates tests/golden/rnn_wide_*.npz: the RNN baseline at hidden sizes past 256 (opts --wide_rnn, csrc/lstm_steps.hip),
by IMPORTING THE REFERENCE's model/rnn.py on CPU -- build container only.  Same recipe as make_golden_rnn.py, whose helpers
this file imports: a train-mode step through the reference's model and the loss composition of train_unimodal.py:188-225,
outputs, losses, counters, gradient statistics of every live parameter (no full LSTM tensors: each file stays at rnn_cfg.npz's
size or below) and post-AdamW statistics.  Every value is cross-checked against tests/rnn_oracle.py (float64); the script
aborts on a mismatch."""
import os

import numpy as np

import make_golden_rnn as R


def case(tag, **kw):
    """make_golden_rnn.case (which runs the cross-check), then the file without its full gradient tensors: statistics only."""
    R.case(tag, full_lstm_grads=False, **kw)
    path = os.path.join(R.HERE, f"{tag}.npz")
    with np.load(path, allow_pickle=False) as z:
        fx = {k: z[k] for k in z.files if not k.startswith("grad::")}
    np.savez_compressed(path, **fx)
    print(f"[golden-rnn-wide] {tag}: {len(fx)} arrays -> {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    case("rnn_wide_264", H=264, B=8, S=5, n_class=17, seed=11, with_exclusion=False)
    case("rnn_wide_512", H=512, B=8, S=16, n_class=122, seed=13, with_exclusion=True)      # (class 120 among the labels)
