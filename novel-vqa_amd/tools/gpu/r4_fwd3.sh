cd $GRAFT_REPO_ROOT
mkdir -p out/r4
timeout -k 10 500 python -m pytest tests/test_gpu_parity_r2.py -x -q -m gpu -k "persistent_forward or headline or timeout or rides_in_the_forward" > out/r4/fwd3_tests.log 2>&1; rc=$?
tail -15 out/r4/fwd3_tests.log
[ $rc -eq 0 ] || exit $rc
for k in 3 1; do
NVQA_FWD_KERNEL=$k timeout -k 10 200 python bench.py --full --no-secondary --no-cpu-baseline > out/r4/fwd3_bench_$k.json 2> out/r4/fwd3_bench_$k.err || { tail -5 out/r4/fwd3_bench_$k.err; exit 1; }
python - <<PY
import json
j = json.loads(open("out/r4/fwd3_bench_$k.json").read().strip().splitlines()[-1])
print("FWD_KERNEL=$k", j["ms_per_step"], j["timed_blocks"], j["roofline"]["frac"], {a: b for a, b in j["kernel_ms_per_step"].items() if "lstm" in a})
PY
done
