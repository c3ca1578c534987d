#!/bin/bash
# 8 ranks (2 x 4 grid, the N=8 bench layout) on ONE GPU over RCCL with fake
# host ids: bench.py incl. checks and extras (--full).  Logs go to $OUT (check_out/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-check_out}
mkdir -p "$OUT"
RANK_TIMEOUT=500 timeout -k 10 560 python3 scripts/rccl_multi.py 8 --cmd python3 bench.py --gpus 8 --dim ${BDIM:-4096} --steps 1 --warmup 1 --full > "$OUT/rccl_b8.log" 2>&1
rc=$?; echo "bench 8 rc=$rc"; grep -E '^\{|timed|rror|skipped' "$OUT/rccl_b8.log" | cut -c1-400 | head -40
exit $rc
