cd $GRAFT_REPO_ROOT
mkdir -p out/r4
for v in 3 2; do
for d in 0 1 2 8 3 9 10 11; do
NVQA_BWD_KERNEL=$v NVQA_PB_DBG=$d timeout -k 10 120 python bench.py --full --steps 10 --warmup 3 --blocks 2 --no-cpu-baseline --no-secondary --arch 2 --bf16 > out/r4/abl.json 2> out/r4/abl.err
python - $v $d <<'PY'
import json,sys
try:
    j = json.loads(open("out/r4/abl.json").read().strip().splitlines()[-1])
    print("bf16 kernel v"+sys.argv[1], "PB_DBG", sys.argv[2], j["ms_per_step"], {k: v for k, v in j["kernel_ms_per_step"].items() if k.startswith("lstm_step_bwd")})
except Exception as e:
    print(sys.argv[1], sys.argv[2], "failed", e, open("out/r4/abl.err").read()[-300:])
PY
done
done
