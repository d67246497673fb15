# full GPU suite + the full bench run (`bench.py --full`: the headline and every secondary figure)
# usage: tools/full_run.sh [output dir, default full_run_out]
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
OUT=${1:-full_run_out}
mkdir -p "$OUT"
timeout 2400 python -m pytest tests -x -q -m gpu > "$OUT/full_tests.log" 2>&1
tail -6 "$OUT/full_tests.log"
timeout 900 python bench.py --full > "$OUT/full_bench.json" 2> "$OUT/full_bench.err"
tail -c 600 "$OUT/full_bench.err"
OUT="$OUT" python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['OUT'], 'full_bench.json')).read().strip().splitlines()[-1])
print({k:d[k] for k in ('value','ms_per_step')})
r=d.get('roofline',{})
print('roofline', {k:r.get(k) for k in ('kernel','frac','frac_rocprof','avg_launch_us','traffic')})
print('rulebook', r.get('rulebook'))
for k in ('h2d_inclusive','ragged','full_model','config5_300k','stage2','n_gt_1_form','cpu_baseline'):
    v=d.get(k);
    if isinstance(v,dict): v={a:b for a,b in v.items() if a not in ('what','sample','config','form')}
    print(k, v)
PY
