"""GPU: the launch sequence of a conv backward -- every pcd_* entry point with the stream it runs on, every Event.record /
wait_event / wait_stream, in order -- and every parameter gradient, bit for bit, equal what the commit before
functional.scheduled_backward issued and computed (tests/golden/backward_schedule_trace.json, written there by
tests/golden/make_backward_schedule_trace.py with the logging code of tests/schedule_trace.py).  None of the weight-gradient
kernels of these layers sums with fp32 atomics (the record was taken twice and agreed), so the gradients compare by sha256.

And the weight-pack launches of a whole backbone over four steps equal what the commit before SparseConvolution's pack cache
issued (tests/golden/backbone_pack_trace.json, tests/golden/make_pack_window_traces.py, tests/pack_window_trace.py).

And the table Conv3x3Packs plans for a small dense model, with the dense weight-pack launches of four steps, equal what the
commit before the dense kinds' one table planned and issued (tests/golden/dense_pack_trace.json,
tests/golden/make_dense_pack_trace.py, tests/dense_pack_trace.py)."""
import json
import os

import pytest

import dense_pack_trace as D
import pack_window_trace as P
import schedule_trace as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_trace():
    return _golden("backward_schedule_trace.json")


def _golden(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


@pytest.mark.parametrize("setting", list(T.SETTINGS))
@pytest.mark.parametrize("case", list(T.CASES))
def test_launch_sequence_and_gradients_are_the_recorded_ones(case, setting, golden_trace, monkeypatch):
    want = golden_trace[case][setting]
    got = T.record(case, setting, monkeypatch)
    for i, (a, b) in enumerate(zip(got["log"], want["log"])):
        assert a == b, (i, a, b, got["log"][max(0, i - 5):i + 3], want["log"][max(0, i - 5):i + 3])
    assert len(got["log"]) == len(want["log"])
    assert got["grads"] == want["grads"]


def test_backbone_packs_once_per_step_and_ahead_of_the_forward_when_told(monkeypatch):
    """VoxelBackBone8x, training, z-fastest bf16 rows: pack_after_update() packs every layer in two batched launches (generic +
    window layers) on the current stream; the step behind it packs nothing; a step without it packs on the side stream, in
    front of the first conv; and so does a step whose weights were edited behind pack_after_update()'s back."""
    want = _golden("backbone_pack_trace.json")
    batched = ["pcd_pack_weights_batched", "pcd_subm_window_pack_weights_batched"]
    assert want["pack_after_update"] == [[n, "main"] for n in batched] and want["step 2"] == []      # the record itself
    assert want["edit, step 3"] == [[n, "side"] for n in batched]
    assert P.backbone_pack_trace(monkeypatch) == want


def test_dense_packs_are_planned_and_made_as_recorded(monkeypatch):
    """BaseBEVBackbone + CenterHeadTowers with the batched head path, training: the plan lists every conv the kernels cover (the
    un-registered first conv of all branches last) with two rows each; run() is ONE launch on the current stream; the step
    behind it packs nothing; a step without it packs per call, forward and data gradient (none for the first conv: no dx);
    and after run() plus an in-place edit of five weights exactly the convs that read them pack per call again (for a branch's
    first-stage weight that is the batched first conv, whose weight aliases it)."""
    want = _golden("dense_pack_trace.json")
    one = ["pcd_conv2d_pack_weight", "main"]
    assert want["run"] == [["pcd_conv2d_pack_weights_batched", "main"]] and want["step 2"] == []      # the record itself
    assert want["step 3, without run"] == [one] * 25 and want["run, edit, step 4"] == want["run"] + [one] * 9
    assert [r[4] for r in want["table"]] == [0, 1, 0, 1, 2, 3, 0, 1, 6, 7, 4, 5] + [0, 1] * 12
    got = D.dense_pack_trace(monkeypatch)
    assert got["table"] == want["table"]
    assert got == want
