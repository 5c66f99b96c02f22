# the --full bench line, then the headline step under rocprofv3 --kernel-trace --stats; everything lands in $OUT (default output/prof_bench)
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
out=${OUT:-output/prof_bench}; mkdir -p "$out"
timeout 600 python bench.py --full --steps 10 --warmup 3 > "$out/bench_line.json" 2> "$out/bench_err.log"
tail -1 "$out/bench_line.json"
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof" -- python bench.py --steps 10 --warmup 3 > "$out/prof_bench.log" 2>&1
f=$(ls "$out"/prof/*/*kernel_stats.csv | head -1); cp "$f" "$out/bench_kernel_stats.csv"; head -40 "$f"
