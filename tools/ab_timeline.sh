#!/bin/bash
# Per-kernel timeline (rocprofv3 kernel trace, iterations [100, 1100) of one
# solve) for each library variant: VARIANTS="base x y".  Summaries go to
# $OUT (default bench_out/ in the repository), traces to a temporary directory.
set -u
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT=${OUT:-$ROOT/bench_out}
mkdir -p "$OUT"
TMP=$(mktemp -d) && cd "$TMP" && export TMPDIR="$TMP"
for V in ${VARIANTS:-base}; do
  if [ $V = base ]; then L=$ROOT/easylp_amd/lib/libeasylp_hip.so; else L=$ROOT/easylp_amd/lib/libeasylp_hip_$V.so; fi
  ELP_LIB_PATH=$L timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d "$TMP/tl_$V" -o run -- python3 $ROOT/bench.py --full --steps 0 --warmup 0 --window 1 --c4 0 --sparse 0 --no-cpu --compare-rules 0 > "$OUT/tl_$V.json" 2>&1 || { echo "fail $V"; exit 1; }
  echo "== $V"; python3 $ROOT/tools/timeline.py $(find "$TMP/tl_$V" -name '*kernel_trace.csv') 100 1000 | head -7
  rm -rf "$TMP/tl_$V"
done
