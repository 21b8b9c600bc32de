cd $GRAFT_REPO_ROOT
mkdir -p out/r4
for e in "X=1" "NVQA_RIDE_GEMM=0" "NVQA_RIDE_CAP=1.5"; do
env $e timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-secondary --ragged > out/r4/rag.json 2> out/r4/rag.err
python - "$e" <<'PY'
import json,sys
j = json.loads(open("out/r4/rag.json").read().strip().splitlines()[-1])
print(sys.argv[1], j["ms_per_step"], {k: v for k, v in j["kernel_ms_per_step"].items() if k.startswith("lstm") or k in ("gemm_head_bwd","colsum")}, j.get("ridden_head_gflop_per_step"))
PY
env $e NVQA_PB_DBG=32 timeout -k 10 120 python bench.py --steps 4 --warmup 1 --blocks 1 --no-cpu-baseline --no-secondary --no-roofline --ragged 2>&1 >/dev/null | grep "persistent BPTT"
done
