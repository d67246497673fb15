#!/usr/bin/env python3
"""Record tests/golden/pack_lifecycle_trace.json, window_decisions.json (no device needed) and, with `gpu`,
backbone_pack_trace.json: what the drivers of tests/pack_window_trace.py log.

Run ONCE, on the commit BEFORE the change whose behaviour is to be compared (tests/test_pack_window_decisions.py and
tests/test_gpu_backward_schedule.py hold the code under test to these records) -- never on the code under test itself.  Every
record is taken twice; the two must agree, or nothing is written.

Usage: python tests/golden/make_pack_window_traces.py [cpu] [gpu] [output directory]
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pack_window_trace as P  # noqa: E402

RECORDS = {"cpu": {"pack_lifecycle_trace.json": P.pack_lifecycle, "window_decisions.json": P.window_decisions},
           "gpu": {"backbone_pack_trace.json": P.backbone_pack_trace}}


def main():
    which = [a for a in sys.argv[1:] if a in RECORDS] or ["cpu"]
    out = ([a for a in sys.argv[1:] if a not in RECORDS] or [HERE])[0]
    mp = pytest.MonkeyPatch()
    for kind in which:
        for name, driver in RECORDS[kind].items():
            first, again = driver(mp), driver(mp)
            assert first == again, f"{name}: two runs of the same code differ"
            with open(os.path.join(out, name), "w") as f:
                json.dump(first, f, indent=1)
                f.write("\n")
            print(f"{name}: written")


if __name__ == "__main__":
    main()
