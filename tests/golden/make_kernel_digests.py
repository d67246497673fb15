#!/usr/bin/env python3
"""Record tests/golden/kernel_digests.json: the sha256 of every output of the cases of tests/kernel_digests.py.

Run ONCE, on the GPU, on the commit BEFORE a change that must leave these kernels' results bit for bit as they are
(tests/test_gpu_kernel_digests.py holds the code under test to this record) -- never on the code under test itself; copy this
file and tests/kernel_digests.py into a checkout of that commit.  Every group is recorded twice; the two records must agree
(a kernel that sums with atomics would show here), or nothing is written.

Usage: python tests/golden/make_kernel_digests.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import kernel_digests as K  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "kernel_digests.json")
    golden = {}
    for group in K.GROUPS:
        first, again = K.record(group), K.record(group)
        differ = sorted(k for k in first if first[k] != again[k])
        assert not differ, f"{group}: two runs of the same code differ in {differ}"
        golden[group] = first
        print(f"{group:18s} {len(first)} digests")
    multi = {k: v for k, v in golden["subm_window"].items() if k.endswith("multi_pass_tiles")}
    print("multi-pass tiles:", multi)
    assert all(multi[f"dense/{ch}/multi_pass_tiles"] > 0 for ch in (16, 32, 64)), "the dense block must have multi-pass tiles"
    with open(out, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
