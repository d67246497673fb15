#!/usr/bin/env python3
"""Record tests/golden/backward_schedule_trace.json: the launch sequence (every pcd_* entry point with its stream, every
Event.record / wait_event / wait_stream) and the sha256 of every parameter gradient of the two models of
tests/schedule_trace.py under its four switch settings.

Run ONCE, on the GPU, on the commit BEFORE the change whose schedule is to be compared (tests/test_gpu_backward_schedule.py
holds the code under test to this record) -- never on the code under test itself.  Every setting is recorded twice; the two
records must agree (a kernel that sums with atomics would show here), or nothing is written.

Usage: python tests/golden/make_backward_schedule_trace.py [output.json]
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import schedule_trace as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "backward_schedule_trace.json")
    mp = pytest.MonkeyPatch()
    trace = {}
    for case in T.CASES:
        trace[case] = {}
        for setting in T.SETTINGS:
            first, again = T.record(case, setting, mp), T.record(case, setting, mp)
            assert first == again, f"{case} / {setting}: two runs of the same code differ"
            trace[case][setting] = first
            print(f"{case:7s} {setting:13s} {len(first['log'])} log entries, {len(first['grads'])} gradients")
    with open(out, "w") as f:
        json.dump(trace, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
