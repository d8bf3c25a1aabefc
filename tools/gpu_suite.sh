#!/bin/bash
# GPU suite + a short benchmark run with every leg (--full); outputs under $OUT/<TAG>_* (default: results/).
# Usage: [OUT=dir] tools/gpu_suite.sh TAG [pytest -k expr]
TAG=${1:-suite}; K=${2:-}; OUT=${OUT:-results}
mkdir -p "$OUT"
if [ -n "$K" ]; then timeout 1200 python -m pytest tests -m gpu -x -q -k "$K" > $OUT/${TAG}_pytest.log 2>&1
else timeout 1200 python -m pytest tests -m gpu -x -q > $OUT/${TAG}_pytest.log 2>&1; fi
echo "pytest rc=$?" >> $OUT/${TAG}_pytest.log
timeout 300 python bench.py --full --steps 3 --warmup 1 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
tail -15 $OUT/${TAG}_pytest.log
python - <<PY
import json
try:
    d=json.loads(open("$OUT/${TAG}_bench.json").read().strip().splitlines()[-1])
    print("value", d["value"], "ms/step", d["ms_per_step"], "frac", d["roofline"]["frac"], "kernel ms", d["roofline"]["avg_launch_ms"], "free", (d.get("other_states") or {}).get("value"))
except Exception as e:
    print("bench failed", e); print(open("$OUT/${TAG}_bench.err").read()[-2000:])
PY
