"""The tiled and split-key attention cores give, bit for bit, what they gave at the commit before their shared argument block
(csrc/attention_lse.h): the SHA-256 of o, lse, delta, dq, dk and dv of every case of tests/attention_bits_cases.py against
tests/golden/attention_bits_parent.json.  Equality is the bar: no sum was reordered.  Needs an MI355X."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_bits_cases as BC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_bits_parent.json")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from r3d_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_every_case_is_recorded(ops, golden):
    assert [c[0] for c in BC.cases(ops.mha_splitk_chunk)] == list(golden)
    assert all(sorted(v) == sorted(BC.NAMES) for v in golden.values())


@pytest.mark.parametrize("i", range(len(BC.cases())), ids=[c[0] for c in BC.cases()])
def test_bits_are_the_parents(ops, golden, i):
    case = BC.cases(ops.mha_splitk_chunk)[i]
    got = BC.digests(ops, case)
    assert got == golden[case[0]], (case[0], [n for n in BC.NAMES if got[n] != golden[case[0]][n]])
