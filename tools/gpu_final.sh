#!/bin/bash
# round-end check: the GPU suite, smoke(), then the benchmark with everything it measures (N = 1)
#   bash tools/gpu_final.sh [OUTDIR]      (logs and the bench line land in OUTDIR, default: a fresh temporary directory)
cd "$(dirname "$0")/.."
OUT=${1:-$(mktemp -d)}
mkdir -p "$OUT"
echo "output in $OUT"
timeout 900 python -m pytest tests -m gpu -x -q > "$OUT/final_pytest.log" 2>&1
echo "pytest rc $?" >> "$OUT/final_pytest.log"
tail -4 "$OUT/final_pytest.log"
timeout 120 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
timeout 600 python bench.py --full > "$OUT/final_bench.json" 2> "$OUT/final_bench.err"
echo "bench rc $?"
python - "$OUT/final_bench.json" <<'PY'
import json
import sys
try:
    d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
    print({k: d[k] for k in ("value", "ms_per_step")}, d["roofline"]["frac"], d["roofline"].get("traffic"))
    print(d["summary"].get("legs_ms_per_1B_rows"))
except Exception as e:
    print("bench line unreadable:", e)
PY
