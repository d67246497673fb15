"""GPU: the window kernels (forward, data gradient, weight gradient), every instantiation the gather-GEMM dispatch returns, the
class-grouped data gradient and the bucket farthest point sampling compute, bit for bit, what they computed on the commit
before their ablation switches and trace stamps were taken out; the anchor heads and the point heads (PointHeadSimple,
PointHeadBox, PointIntraPartOffsetHead: targets, losses with their gradients, decoding) what they computed on the commit before
each family was folded onto one core (tests/golden/kernel_digests.json, written there by
tests/golden/make_kernel_digests.py from the cases of tests/kernel_digests.py).  None of them sums with float atomics (the
record was taken twice and agreed), so every output compares by sha256.

Reached by the cases: multi-pass window tiles on the dense block at every width (28 / 75 / 150 tiles at 16 / 32 / 64 channels),
none on the sparse grid; all three bodies of the window weight gradient (every launch runs one workgroup per neighbour run);
both class-tile sizes of the class-grouped data gradient."""
import json
import os

import pytest

import kernel_digests as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_digests():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("group", K.GROUPS)
def test_outputs_are_the_recorded_ones(group, golden_digests):
    want, got = golden_digests[group], K.record(group)
    assert sorted(got) == sorted(want)
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, differ
