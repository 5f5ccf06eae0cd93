#!/bin/bash
# r6_call29 -- the driver's round-end sequence on the final tree: GPU tests, smoke(), the default bench line
export PYTHONPATH=$PWD
# OUT (set by the caller, no default): the directory the other steps of this batch write to; the bench lines below write there too
OUT=$(cd "${OUT:?set OUT to the output directory of this batch}" && pwd) || exit 1
mkdir -p gpurun_out/r6
timeout 1500 python3 -m pytest tests -x -q -m gpu > gpurun_out/r6/final_gpu_tests.log 2>&1; tail -2 gpurun_out/r6/final_gpu_tests.log
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
python3 bench.py --full > "$OUT"/r6/final_bench_line.json 2> "$OUT"/r6/final_bench.err; echo "bench rc $?"; wc -c "$OUT"/r6/final_bench_line.json
OUT="$OUT" python3 - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "r6", "final_bench_line.json")).read().strip().splitlines()[-1])
print({k: d[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "scaling", "vs_baseline")})
print("roofline", {k: d["roofline"][k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic")})
print("cpu_baseline", d["cpu_baseline"])
PY
