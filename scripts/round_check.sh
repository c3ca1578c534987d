#!/bin/bash
# GPU validation pass: gpu tests, smoke, default bench with its checks and extra
# configs (--full), device svd/heev tester rows.  Logs go to $OUT (check_out/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-check_out}
mkdir -p "$OUT"
timeout -k 10 700 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || { tail -20 "$OUT/pytest_gpu.log"; exit 1; }
tail -1 "$OUT/pytest_gpu.log"
timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { tail -20 "$OUT/smoke.log"; exit 1; }
tail -2 "$OUT/smoke.log"
timeout -k 10 560 python bench.py --full > "$OUT/bench_default.log" 2>&1 || { tail -20 "$OUT/bench_default.log"; exit 1; }
grep -e timed -e metric "$OUT/bench_default.log"
timeout -k 10 300 bin/slate_tester svd,heev --type d,z --dim 2048 --nb 128 --target d > "$OUT/eig_dev.log" 2>&1 || { tail -20 "$OUT/eig_dev.log"; exit 1; }
cat "$OUT/eig_dev.log"
