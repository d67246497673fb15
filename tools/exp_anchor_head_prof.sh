#!/bin/bash
# Kernel time by name of the plain and the curriculum anchor loss (forward + backward, 468 x 468 x 2 anchors, one class,
# B = 4): ONE rocprofv3 --kernel-trace --stats run of tools/exp_anchor_head_prof.py, then its per-phase summary.
# Run from the repository root; writes $OUT/anchor_head_prof.{log,txt} (OUT defaults to prof_out).
set -o pipefail
export OUT=${OUT:-prof_out}
TRACE=$(mktemp -d)
mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$TRACE" -o r -- python3 tools/exp_anchor_head_prof.py > "$OUT/anchor_head_prof.log" 2>&1 || { tail -20 "$OUT/anchor_head_prof.log"; exit 1; }
DB=$(find "$TRACE" -name "*.db" | head -1)
python3 tools/exp_anchor_head_prof.py --summarise "$DB" "$OUT/anchor_head_prof_phases.json" | tee "$OUT/anchor_head_prof.txt"
