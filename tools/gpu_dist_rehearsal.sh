# N = 2 rehearsal of bench.py's multi-rank path on a one-GPU box: two ranks share the GPU
# over gloo (torch all-reduce merge + slab finalize on the comm lane; RCCL needs one GPU per
# rank), then N = 1 over the same global poses: the merged log-odds digests (bench.py --full)
# must be equal.  Lines go to $OUT (default bench_out/dist, ignored by git).
set -o pipefail
cd "$(dirname "$0")/.."
export OUT=${OUT:-bench_out/dist}
mkdir -p "$OUT"
PL=${PL:-16}
DMF_BENCH_BACKEND=gloo timeout -k 10 600 python -m torch.distributed.run --nnodes 1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --poses-per-gpu $PL --steps ${STEPS:-3} --warmup 1 --pmc off --no-secondary --cpu-frames 0 > "$OUT/n2.json" 2> "$OUT/n2.err" || { echo DISTFAIL; tail -30 "$OUT/n2.err"; exit 1; }
timeout -k 10 300 python bench.py --full --poses-per-gpu $((2 * PL)) --steps ${STEPS:-3} --warmup 1 --pmc off --no-secondary --cpu-frames 0 --cpu-reverse-poses 0 > "$OUT/n1.json" 2> "$OUT/n1.err" || { echo N1FAIL; tail -30 "$OUT/n1.err"; exit 2; }
python3 - <<'PY' || exit 3
import json
import os
out = os.environ["OUT"]
a = json.load(open(os.path.join(out, "n2.json"))); b = json.load(open(os.path.join(out, "n1.json")))
print("N=2 gloo", a["logodds_digest"], a["step_breakdown_ms"]["merge_kind"], "| N=1", b["logodds_digest"])
assert a["logodds_digest"] == b["logodds_digest"], "merged log-odds differ from one rank fusing all poses"
print("DIGESTS EQUAL")
PY
echo ALLOK
