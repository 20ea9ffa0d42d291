"""The batch shapes of the hidden-128 chain kernels (csrc/fuser_chain.hip, csrc/decoder_chain.hip) and the path the engine
must route each one to.  tests/test_chain_admission_cpu.py checks every row against the host-side admission predicates;
tests/test_chain_shapes_gpu.py runs every row on the GPU and checks the path the engine actually took.

All rows: H = 128, Q = 8, 8 heads, one decoder layer, n_class K, pad_idx K + 1.  Columns of the expected path:
  fuser  -- fuser_chain_fwd / _bwd run (r3d_fuser_chain_supported: 2N % 16 == 0, K <= 128, B*Q % 16 == 0);
  bwd    -- the backward fuser chain's precision: "bf3" (K <= 32) or "fp32", None when the fuser chain is off;
  dec    -- decoder_chain runs (r3d_decoder_chain_supported: 1 <= S <= 64);
  defer  -- in a training step the tail, the losses and the tail backward run inside the decoder chain's launch
            (r3d_decoder_tail_losses_supported: K + 1 <= 24).
pad: "tail" = synth.make_batch's default padding (the last max(S // 8, 1) frames of odd clips), "none" = no padding, or a
tuple of per-clip valid lengths (past them: zero features and depth, as pad_sequence(padding_value=0) leaves them, and
pad_idx labels, as the collate writes a ragged batch)."""
import collections

import numpy as np
import torch

from oracle import synth

H, Q, HEADS = 128, 8, 8

Case = collections.namedtuple("Case", "B S K pad fuser bwd dec defer why")

CASES = [
    Case(8, 16, 17, "tail", True, "bf3", True, True, "the headline shape"),
    Case(8, 16, 23, "tail", True, "bf3", True, True, "largest K whose tail stays in the decoder chain"),
    Case(8, 16, 24, "tail", True, "bf3", True, False, "first K whose tail leaves it"),
    Case(8, 16, 32, "tail", True, "bf3", True, False, "last K with the bf16x3 backward"),
    Case(8, 16, 33, "tail", True, "fp32", True, False, "first K with the fp32 backward under the bf16x3 forward"),
    Case(8, 16, 128, "tail", True, "fp32", True, False, "largest admitted segmentation head (8 tiles)"),
    Case(8, 16, 129, "tail", False, None, True, False, "fuser chain refused, decoder chain on"),
    Case(8, 32, 122, "tail", True, "fp32", True, False, "NTU per-GPU shape (cfg3)"),
    Case(8, 7, 17, "tail", True, "bf3", True, True, "odd S: Lk not a multiple of 16, N = 56"),
    Case(8, 1, 17, "none", True, "bf3", True, True, "one key per clip"),
    Case(8, 63, 17, "tail", True, "bf3", True, True, "S = 63"),
    Case(8, 64, 122, "tail", True, "fp32", True, False, "largest admitted S, with a wide head"),
    Case(8, 65, 17, "tail", True, "bf3", False, False, "decoder chain refused, fuser chain on"),
    Case(10, 12, 17, "tail", True, "bf3", True, True, "B != 8, both chains admitted"),
    Case(9, 16, 17, "tail", False, None, True, True, "fuser chain refused (B*Q = 72), decoder chain on"),
    Case(16, 16, 17, "tail", True, "bf3", True, True, "B = 16"),
    Case(32, 32, 122, "tail", True, "fp32", True, False, "many clips at the NTU head"),
    # ragged padding: clips with 1, 2, S-1 and S valid keys
    Case(8, 16, 17, (1, 2, 15, 16, 16, 8, 3, 16), True, "bf3", True, True, "ragged keys, bf16x3 backward"),
    Case(8, 33, 122, (1, 2, 32, 33, 20, 33, 5, 17), True, "fp32", True, False, "ragged keys, odd S, NTU head"),
    Case(8, 16, 17, "none", True, "bf3", True, True, "no padding at all"),
]

# validation forwards (B = 1: the fuser chain's query role needs B*Q % 16 == 0, the decoder chain admits S <= 64)
VAL_CASES = [(1, 11, 17, True), (1, 64, 17, True), (1, 65, 17, False)]      # (B, S, K, decoder chain)

BATCH_SEED = 77


def case_id(c):
    p = c.pad if isinstance(c.pad, str) else "ragged"
    return f"B{c.B}-S{c.S}-K{c.K}-{p}"


def make_batch(c, seed=BATCH_SEED, depth_hw=(224, 224)):
    """[features, depth, past_label, trans_dur_future, trans_future_target] (torch, CPU) for a case row."""
    pad_idx = c.K + 1
    b = synth.make_batch(c.B, c.S, c.K, pad_idx, seed, pad_tail=(c.pad == "tail"), depth_hw=depth_hw)
    if not isinstance(c.pad, str):
        assert len(c.pad) == c.B and all(1 <= n <= c.S for n in c.pad)
        feats, depth, lab = b[0], b[1], b[2]
        for i, n in enumerate(c.pad):
            feats[i, n:] = 0.0
            depth[i, n:] = 0.0
            lab[i, n:] = pad_idx
    return [torch.from_numpy(np.ascontiguousarray(x)) for x in b]
