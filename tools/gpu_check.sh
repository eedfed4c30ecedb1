# GPU suite + smoke + the full default bench line (no separate profiling) on one box.
# Logs go to $OUT (default bench_out/, ignored by git).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 700 python -u -m pytest tests -m gpu -x -v --timeout 180 --timeout-method thread > "$OUT/gpu_tests.log" 2>&1 || { echo TESTFAIL; tail -30 "$OUT/gpu_tests.log"; exit 1; }
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { echo SMOKEFAIL; tail -20 "$OUT/smoke.log"; exit 2; }
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { echo BENCHFAIL; tail -20 "$OUT/bench.err"; exit 3; }
tail -3 "$OUT/gpu_tests.log"; cat "$OUT/bench.json"
echo ALLOK
