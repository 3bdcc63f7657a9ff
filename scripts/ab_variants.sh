#!/bin/bash
# scripts/ab_variants.sh TAG [variant.so ...] -- the step's kernel times of bench.py with alternative builds of libagc_hip.so
# (the variant goes IN FRONT of whatever LD_PRELOAD already holds, for the host library, and AGC_HIP_LIB for the ctypes binding --
# both for the one bench command only); first entry "base" = the in-tree library.  Stops at the first run that does not exit 0
# (a variant that faults or hangs ends the comparison: nothing more is started on the GPU).
TAG=$1; shift
OUT=${OUT:-scripts/variants/$TAG}  # (the JSON lines and logs of the runs)
mkdir -p "$OUT"
for v in base "$@"; do
  n=$(basename $v .so)
  if [ "$v" = base ]; then
    timeout -k 10 300 python bench.py --steps ${STEPS:-8} --warmup 2 --full --no-cpu-baseline > "$OUT/ab_$n.json" 2> "$OUT/ab_$n.err"
  else
    LD_PRELOAD="$PWD/$v${LD_PRELOAD:+:$LD_PRELOAD}" AGC_HIP_LIB="$PWD/$v" \
      timeout -k 10 300 python bench.py --steps ${STEPS:-8} --warmup 2 --full --no-cpu-baseline > "$OUT/ab_$n.json" 2> "$OUT/ab_$n.err"
  fi
  rc=$?
  if [ $rc -ne 0 ]; then
    echo "$n: exit status $rc (124 / 137: time limit; 134: abort; 139: segmentation fault) -- stopping" >&2
    tail -n 5 "$OUT/ab_$n.err" >&2
    exit $rc
  fi
  python - <<PY
import json
try:
    d=json.loads(open("$OUT/ab_$n.json").read().strip().splitlines()[-1])
    print("$n", "value", d["value"], "steps_only_ms", d["config"]["steps_only_ms"], "close_ms", d["config"]["close_ms"], json.dumps(d["roofline"]["kernel_ms_per_step_rank0"]))
except Exception as e:
    print("$n", "failed", e)
PY
done
