#!/bin/bash
# three runs of the track workload (scene S1 512^3, 200 timed frames x 2 repetitions each), optional extra bench flags
cd "$(dirname "$0")/../.." && export OUT_DIR="${OUT_DIR:-profiles/out}" && mkdir -p "$OUT_DIR"
for i in 1 2 3; do
  timeout -k 10 120 python bench.py --full --workload track --no-s2 --no-cpu-baseline "$@" > $OUT_DIR/bench3_$i.json 2> $OUT_DIR/bench3_$i.err
  rc=$?; [ $rc -ge 124 ] && { echo "killed"; exit $rc; }
  python - <<PY
import json
d=json.loads(open("$OUT_DIR/bench3_$i.json").read().strip().splitlines()[-1])
print("run $i", d["value"], d["repetitions_fps"], d["stages_ms"], d["roofline"]["kernel_ms"], d["roofline"]["frac"])
PY
done
