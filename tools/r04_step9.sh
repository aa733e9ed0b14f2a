# round 4, step 9: GPU suite with the fused multivector products everywhere, leak check, bench lines of the library as it stands
set -x
out=gpurun_out/r04_step9
mkdir -p $out
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout -k 10 1100 python -m pytest tests -m gpu -x -q > $out/tests.log 2>&1
rc=$?
tail -4 $out/tests.log
[ $rc -eq 0 ] || exit $rc
LEAK_ROUNDS=6 timeout -k 10 300 python tools/leak_check.py > $out/leak.log 2>&1; echo "leak exit $?"; tail -5 $out/leak.log
timeout -k 10 300 python bench.py --full > $out/bench_c2.json 2> $out/bench_c2.err; echo "c2 exit $?"
timeout -k 10 400 python bench.py --full --problem 27pt --relax 11 --no-cpu-baseline > $out/bench_c4.json 2> $out/bench_c4.err; echo "c4 exit $?"
timeout -k 10 300 python bench.py --full --problem difconv --mixed --no-cpu-baseline > $out/bench_c5.json 2> $out/bench_c5.err; echo "c5 exit $?"
python - <<'PY'
import json
for f in ("c2", "c4", "c5"):
    for l in open("gpurun_out/r04_step9/bench_%s.json" % f):
        if l.startswith('{"metric"'):
            d = json.loads(l)
            print(f, d["ms_per_step"], d["value"], d["roofline"]["frac"], d.get("ms_per_step_codes_off"))
PY
