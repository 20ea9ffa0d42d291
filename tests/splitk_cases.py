"""The shapes and key masks of tests/test_attention_splitk_gpu.py: the split-key cross-attention core
(csrc/attention_splitk.hip) with B = 3 clips.

Rows: (Lk, Lq, dh, heads, drop, mask).  Lk is a number or a position relative to the chunk C = mha_splitk_chunk(Lk, dh)
("C-1", "C", "C+1", "2C+1": both sides of a chunk boundary, and a third chunk of one key); C does not depend on Lk where
the rows use it (checked by resolve).  Every dropout row has an Lk that is no multiple of 4: the keep-mask's row stride in
bytes.  mask:
  "three"  the tiled test's three-clip pattern (tests/test_tiled_attention_gpu.labels): one valid key; the first 64-key
           tile masked (or every third key); a masked tail;
  "first"  the whole first chunk masked in every clip (clip 1: every third later key as well, clip 2: all but the last key);
  "last"   a single valid key in the last chunk: clip 0 nothing else (every earlier chunk wholly masked), clip 1 the
           earlier chunks valid, clip 2 the earlier chunks valid but for every second key."""
import torch

PAD = 99
B = 3

ROWS = [
    (1, 1, 16, 8, False, "three"),
    (63, 8, 5, 8, True, "three"),
    (64, 16, 16, 8, False, "three"),
    (65, 8, 25, 8, True, "three"),
    ("C-1", 8, 16, 8, True, "three"),
    ("C", 16, 64, 2, False, "three"),
    ("C+1", 8, 128, 1, True, "three"),
    ("C+1", 16, 5, 8, True, "first"),
    ("2C+1", 1, 16, 8, False, "first"),
    ("2C+1", 8, 25, 8, True, "last"),
    ("2C+1", 16, 128, 1, False, "first"),
    (1142, 8, 16, 8, True, "three"),
    (1142, 8, 128, 1, False, "last"),
    (1142, 16, 64, 2, True, "first"),
]


def resolve(lk, dh, chunk_of):
    """The row's Lk as a number; chunk_of(Lk, dh) is ops.mha_splitk_chunk."""
    if not isinstance(lk, str):
        return lk
    C = chunk_of(1, dh)
    n = {"C-1": C - 1, "C": C, "C+1": C + 1, "2C+1": 2 * C + 1}[lk]
    assert chunk_of(n, dh) == C, "the chunk moved with Lk: restate the row"
    return n


def row_id(r):
    return f"Lk{r[0]}-Lq{r[1]}-dh{r[2]}x{r[3]}-{'drop' if r[4] else 'nodrop'}-{r[5]}"


def labels(Lk, mask, C):
    """int64 [B, Lk]: PAD where the key is masked; no clip is masked entirely."""
    if mask == "three":
        from tests.test_tiled_attention_gpu import labels as three
        return three(Lk)
    lab = torch.zeros(B, Lk, dtype=torch.int64)
    last0 = (Lk - 1) // C * C                    # first key of the last chunk
    if mask == "first":
        assert Lk > C
        lab[:, :C] = PAD
        lab[1, C + 2::3] = PAD
        lab[2, C:Lk - 1] = PAD
    elif mask == "last":
        assert last0 > 0
        lab[:, last0:] = PAD
        lab[0, :] = PAD
        lab[0, Lk - 1] = 0
        lab[1, last0] = 0
        lab[2, (last0 + Lk) // 2] = 0
        lab[2, 1:last0:2] = PAD
    else:
        raise ValueError(mask)
    assert bool((lab != PAD).any(dim=1).all())
    return lab
