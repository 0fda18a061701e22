#!/bin/bash
# stress with host delivery (the download workers of the parked host team) and many steps on one handle + MultiMat shards
#   usage: tools/stress_delivery.sh N [OUT_DIR]   (the last run's line and stderr are kept in OUT_DIR, a fresh temporary one by default)
OUT=${2:-$(mktemp -d)}
mkdir -p "$OUT"
for i in $(seq 1 $1); do
  timeout -s ABRT 200 python -X faulthandler bench.py --full --no-cpu-baseline --no-heavy-tailed --no-randsvd --no-split-probe --steps 30 --warmup 2 > "$OUT/stress2_out.txt" 2> "$OUT/stress2_err.txt"
  rc=$?
  if [ $rc -ne 0 ]; then echo "run $i rc=$rc"; tail -12 "$OUT/stress2_err.txt" | cut -c1-150; exit 0; fi
  python -c "import json, sys; d=json.load(open(sys.argv[1])); print('run $i', d['ms_per_step'], d['config']['irlba_ms'])" "$OUT/stress2_out.txt"
done
echo "all $1 runs finished"
