"""GPU: the launch sequence of a conv backward -- every pcd_* entry point with the stream it runs on, every Event.record /
wait_event / wait_stream, in order -- and every parameter gradient, bit for bit, equal what the commit before
functional.scheduled_backward issued and computed (tests/golden/backward_schedule_trace.json, written there by
tests/golden/make_backward_schedule_trace.py with the logging code of tests/schedule_trace.py).  None of the weight-gradient
kernels of these layers sums with fp32 atomics (the record was taken twice and agreed), so the gradients compare by sha256."""
import json
import os

import pytest

import schedule_trace as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_trace():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backward_schedule_trace.json")) as f:
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
