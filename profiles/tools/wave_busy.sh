#!/bin/bash
# Dev tool: per-wave busy / barrier-wait ticks of the fill kernel on the bench workload, from the light clock mode of the diagnostics build
# (make -C mir-prefer_amd/csrc DIAG=1; MIRP_FOLD_CLOCKS=2: two clock reads per wave and interval):
#   profiles/tools/wave_busy.sh [libraries, default libmirprefer_diag.so]
for l in "${@:-libmirprefer_diag.so}"; do
  echo "== $l"
  MIRP_LIB=$PWD/mir-prefer_amd/$l MIRP_FOLD_CLOCKS=2 python profiles/tools/ab_time.py 2>&1 | grep -E "wave +[0-9]+:|fill " | tail -17 | \
    awk '/wave/ { split($0, a, "splits="); split(a[2], b, " barrier="); printf "%s busy %.1f wait %.1f (%.0f %% busy)\n", $5, b[1] / 1e9, b[2] / 1e9, 100 * b[1] / (b[1] + b[2]); next } { print }'
done
