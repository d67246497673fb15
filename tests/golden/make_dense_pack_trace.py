#!/usr/bin/env python3
"""Record tests/golden/dense_pack_trace.json: what the driver of tests/dense_pack_trace.py logs (needs the device).

Run ONCE, on the commit BEFORE the change whose behaviour is to be compared (tests/test_gpu_backward_schedule.py holds the code
under test to this record) -- never on the code under test itself.  The record is taken twice; the two must agree, or nothing
is written.

Usage: python tests/golden/make_dense_pack_trace.py [output directory]
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dense_pack_trace as D  # noqa: E402


def main():
    out = (sys.argv[1:] or [HERE])[0]
    mp = pytest.MonkeyPatch()
    first, again = D.dense_pack_trace(mp), D.dense_pack_trace(mp)
    assert first == again, "two runs of the same code differ"
    with open(os.path.join(out, "dense_pack_trace.json"), "w") as f:
        json.dump(first, f, indent=1)
        f.write("\n")
    print("dense_pack_trace.json: written")


if __name__ == "__main__":
    main()
