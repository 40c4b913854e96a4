#!/bin/bash
# GPU box, repository root: the two N^3-bound workloads (Hessian pass per frame at 512^3; Gauss-Newton relocalisation at 1024^3), one line each
cd "$(dirname "$0")/../.." && export OUT_DIR="${OUT_DIR:-profiles/out}" && mkdir -p "$OUT_DIR"
for w in hessian reloc; do
  timeout -k 10 300 python bench.py --full --workload $w --no-cpu-baseline "$@" > $OUT_DIR/bench_$w.json 2> $OUT_DIR/bench_$w.err
  rc=$?; [ $rc -ge 124 ] && { echo "killed"; exit $rc; }
  python - <<PY
import json
d=json.loads(open("$OUT_DIR/bench_$w.json").read().strip().splitlines()[-1])
print("$w", d["value"], d["unit"], {k: d[k] for k in d if k.startswith("roofline")})
PY
done
