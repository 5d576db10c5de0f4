#!/usr/bin/env bash
# Smoke, GPU parity tests, bench, rocprof kernel trace in one go.  Outputs under $OUT_DIR (default out/).
#   bash tools/gpu_check.sh
cd "${GRAFT_REPO_ROOT:-.}"
R=$(pwd)
O=$(realpath -m "${OUT_DIR:-out}"); mkdir -p "$O"
export TMPDIR=/tmp
echo "== smoke"; timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1; echo "smoke rc=$?"; tail -3 "$O/smoke.log"
if [ "${SKIP_TESTS:-0}" != "1" ]; then
echo "== pytest -m gpu"; timeout 1200 python -m pytest tests -m gpu -q ${PYTEST_ARGS:-} > "$O/pytest_gpu.log" 2>&1; echo "pytest rc=$?"; tail -40 "$O/pytest_gpu.log"
fi
echo "== bench"; timeout 900 python bench.py --full --steps ${STEPS:-20} --warmup 3 ${BENCH_ARGS:-} > "$O/bench.json" 2> "$O/bench.err"; echo "bench rc=$?"; cat "$O/bench.json"; tail -5 "$O/bench.err"
if [ "${SKIP_PROF:-0}" != "1" ]; then
echo "== rocprofv3 kernel trace"
cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -o trace -- python "$R/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline > "$O/prof_bench.json" 2> "$O/prof.err"; echo "rocprof rc=$?"
cd "$R"; find "$O/prof" -name '*stats*' | head
f=$(find "$O/prof" -name '*kernel_stats.csv' | head -1); [ -n "$f" ] && head -25 "$f"
fi
