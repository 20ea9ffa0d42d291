"""The shapes the TCN suite pins (tests/test_tcn_cpu.py, tests/test_tcn_gpu.py, tests/golden/make_golden_tcn.py).

Tolerances are the project's.  Forward values: rtol 1e-3, atol 1e-3 * max(1, |ref|_max).  Kernel gradients: rtol 2e-3, atol
2e-5 * max(1, |ref|_max); whole-step gradients and post-AdamW values: rtol 2e-3, atol 2e-3 * max(1e-3, |ref|_max), norms
within 2e-3 * max(1e-3, |ref|) (all three as tests/test_rnn_gpu.py has them).  They were set for reductions of at most
2048 terms and the first convolution sums 6144; a case that misses them gets 4 x the measured deviation of float32
PyTorch from the float64 oracle on that case, recorded in WIDENED as (case, measured deviation, bound).  None needs one.
ReLU kinks are not a reduction-order effect and are handled apart: a unit whose oracle input lies within fp32 rounding of
zero may land on the other side in fp32 (tcn_odd has one at level 2, conv2, channel 171: oracle pre-activation -3.8e-7
against a maximum of 4.21; a flip moves that channel's bias gradient by 2.9e-5 against an atol of 1.07e-5).  Such units
are identified from the oracle by the rule of tests/helpers.ffn_kink_units (0 < |u| <= 2e-6 max|u|,
tcn_oracle.kink_channels) and left out of the full-tensor comparison of their own channel's bias / weight_g gradient;
the norms over all channels are still compared.

The weight-norm form (s, bias, ReLU epilogue, bwd_prep, the rank-one epilogue of the weight gradient) is pinned over every
case of CONV_CASES as well, next to the raw products."""

# (C_in, C_out, dilation): every convolution the model has
CONV_KINDS = [(2048, 256, 1), (256, 256, 1), (256, 512, 2), (512, 512, 2), (512, 512, 4), (512, 256, 8), (256, 256, 8)]
CONV_B = (1, 8, 13)
CONV_S = (1, 2, 3, 15, 16, 17, 37, 64, 200)     # shorter than one shift, shorter than two, off every tile grid
CONV_CASES = [(ci, co, d, B, S) for (ci, co, d) in CONV_KINDS for B in CONV_B for S in CONV_S]

# whole-model steps: (tag, B, S, num_classes, n_class of the synthetic batch, pad_idx, seed).  In the first case pad_idx is
# a real class index (16 < 17), so the arg-max penalty of cal_loss can fire; in the others it lies outside the logits as in
# the other fixtures (pad_idx = n_class + 1).
STEP_CASES = [("tcn_tiny", 2, 5, 17, 15, 16, 3), ("tcn_cfg", 8, 16, 122, 122, 123, 9), ("tcn_odd", 13, 37, 17, 17, 18, 5),
              ("tcn_long", 4, 200, 49, 49, 50, 7)]
TRAIN_LOOP = dict(tag="tcn_train_loop", B=8, S=6, num_classes=17, n_class=15, pad_idx=16, n_steps=2, epochs=2, seed=1, val_S=9)
LR, WD = 1e-3, 5e-3

# shapes check_tcn_shape refuses: (B, S, num_classes, anticipated_frames, word of the message)
REFUSED = [(0, 16, 17, 8, "at least one"), (8, 0, 17, 8, "at least one"), (8, 16, 0, 8, "positive"), (8, 16, 17, 0, "positive"),
           (1024, 1024, 17, 8, "2^31"), (1, 2 ** 20, 17, 8, "2^31"), (8, 16, 8193, 8, "regression head"),
           (8, 16, 17, 4096, "regression head"), (8200, 1, 17, 8, "loss launch"), (1, 4, 65537, 1, "loss launch")]
ADMITTED = [(1, 1, 1, 1), (1, 1, 17, 8), (8, 16, 122, 8), (16, 1024, 17, 8), (1023, 1024, 17, 8), (8, 16, 8192, 8)]
WIDENED = []
