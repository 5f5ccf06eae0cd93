# tools/round_end_r5_bench_only.sh -- the bench + rocprof part of tools/round_end_r5.sh alone (after profiles/traffic.json was regenerated without a new PMC pass)
# OUT (set by the caller, no default): the directory the other steps of this batch write to; the bench lines below write there too
OUT=$(cd "${OUT:?set OUT to the output directory of this batch}" && pwd) || exit 1
root=$PWD
python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT"/round_end_bench.json.log 2> "$OUT"/round_end_bench.err
cp gpurun_out/bench_suite.json gpurun_out/round_end_bench_suite.json
export TMPDIR=/tmp
rm -rf gpurun_out/round_end_prof
(cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/round_end_prof -- python3 "$root"/bench.py --full --no-suite --no-vendor --steps 20 > "$OUT"/round_end_prof.log 2>&1)
cp gpurun_out/bench_suite.json gpurun_out/round_end_prof_suite.json
tail -c 400 "$OUT"/round_end_bench.json.log
