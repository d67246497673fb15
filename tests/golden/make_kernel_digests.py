#!/usr/bin/env python3
"""Record tests/golden/kernel_digests.json: the sha256 of every output of the cases of tests/kernel_digests.py.

Run ONCE, on the GPU, on the commit BEFORE a change that must leave these kernels' results bit for bit as they are
(tests/test_gpu_kernel_digests.py holds the code under test to this record) -- never on the code under test itself; copy this
file and tests/kernel_digests.py into a checkout of that commit.  Every group is recorded twice; the two records must agree
(a kernel that sums with atomics would show here), or nothing is written.

With group names, only those groups are recorded and merged into the existing file: the entries of every other group stay
as they are.

Usage: python tests/golden/make_kernel_digests.py [--out output.json] [group ...]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import kernel_digests as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "kernel_digests.json"))
    ap.add_argument("groups", nargs="*", help="record only these groups (default: all)")
    args = ap.parse_args()
    assert set(args.groups) <= set(K.GROUPS), f"groups are {K.GROUPS}"
    golden = {}
    if args.groups:
        with open(args.out) as f:
            golden = json.load(f)
    for group in args.groups or K.GROUPS:
        first, again = K.record(group), K.record(group)
        differ = sorted(k for k in first if first[k] != again[k])
        assert not differ, f"{group}: two runs of the same code differ in {differ}"
        golden[group] = first
        print(f"{group:18s} {len(first)} digests")
    if "subm_window" in (args.groups or K.GROUPS):
        multi = {k: v for k, v in golden["subm_window"].items() if k.endswith("multi_pass_tiles")}
        print("multi-pass tiles:", multi)
        assert all(multi[f"dense/{ch}/multi_pass_tiles"] > 0 for ch in (16, 32, 64)), "the dense block must have multi-pass tiles"
    with open(args.out, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
