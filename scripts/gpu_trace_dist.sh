#!/bin/bash
# p > 1 lookahead evidence: 2x1 and 2x2 RCCL runs (ranks share the GPU), device-span traces
# and the backward-error checks (--full).  Logs and traces go to $OUT (check_out/trace_dist).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-check_out/trace_dist}
mkdir -p "$OUT"
for g in "2 2 1" "4 2 2"; do
  set -- $g
  timeout -k 10 400 python scripts/rccl_multi.py $1 --cmd python bench.py --gpus $1 --p $2 --q $3 --dim 12288 --nb 512 --routines dgetrf,dgeqrf --steps 1 --warmup 1 --full --extras none --trace "$OUT/p$2x$3" > "$OUT/run_$2x$3.log" 2>&1 || { tail -30 "$OUT/run_$2x$3.log"; exit 1; }
  grep -E "timed|backward" "$OUT/run_$2x$3.log" | head -8
  for r in dgetrf dgeqrf; do echo "== $2x$3 $r"; python3 scripts/trace_overlap.py "$OUT/p$2x$3_$r.json"; done
done
rm -f "$OUT"/*.svg
