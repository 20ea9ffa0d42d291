"""Pinned shapes of the RNN baseline's recurrence kernels (csrc/lstm.hip) for tests/test_rnn_gpu.py: every clip count of
{1, 8, 13, 32}, every clip length of {1, 2, 16, 37, 64, 512}, hidden at both ends of the admitted range (8, 256), at the
opts.py default 128, at 64 (the h = 32 / 64 instance boundaries) and off the power-of-two grid (136, 200)."""

# (B, S, H)
KERNEL_CASES = [
    (1, 1, 128),
    (1, 2, 8),
    (8, 16, 128),
    (8, 16, 8),
    (8, 16, 256),
    (13, 37, 136),
    (13, 2, 256),
    (32, 64, 256),
    (32, 1, 64),
    (8, 37, 200),
    (1, 512, 128),
    (2, 520, 256),
]

# hidden sizes the engine admits / refuses (engine_rnn.check_rnn_shape)
ADMITTED_H = (8, 16, 64, 128, 136, 200, 256)
REFUSED_H = (0, 4, 12, 130, 264, 512)
