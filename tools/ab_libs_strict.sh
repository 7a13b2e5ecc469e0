#!/bin/bash
# Interleaved A/B of prebuilt variant libraries (tools/prebuild_variants.py → build/variants/): every bench.py invocation runs under its own
# time limit, and the FIRST failure ends the script (tools/bench_libs.py carries on after one): a bench.py that exits non-zero, is killed by
# its time limit or by a signal — also AFTER it has printed its result line —, prints no result line, or prints one without the two figures.
# One line per run into <out file>; the last stdout / stderr of a run stay in <out file>.stdout / .err.
# usage: tools/ab_libs_strict.sh <out file> <reps> <variant> ...
set -u -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
out=$1; reps=$2; shift 2
mkdir -p "$(dirname "$out")"
: > "$out"
for r in $(seq 1 "$reps"); do
  for v in "$@"; do
    lib="$R/build/variants/libsphmi_$v.so"
    [ -f "$lib" ] || { echo "rep $r $v: no such library: $lib" | tee -a "$out"; exit 1; }
    t0=$(date +%s)
    SPHMI_LIB="$lib" timeout -k 10 150 python "$R/bench.py" --steps 60 --warmup 5 > "$out.stdout" 2> "$out.err"
    rc=$?
    if [ $rc -ne 0 ]; then
      echo "rep $r $v: FAILED (bench.py exit $rc)" | tee -a "$out"; tail -20 "$out.err"; exit 1
    fi
    python - "$r" "$v" "$out.stdout" $(( $(date +%s) - t0 )) <<'PY' | tee -a "$out"
import json, sys
lines = [l for l in open(sys.argv[3]) if l.startswith("{")]
if not lines:
    sys.exit(f"rep {sys.argv[1]} {sys.argv[2]}: FAILED (no result line)")
j = json.loads(lines[-1])
print(f"rep {sys.argv[1]} {sys.argv[2]:10s} value {j['value']:.4e} upd/s   kernel {j['roofline']['avg_launch_ms']:.4f} ms   ({sys.argv[4]} s wall)")
PY
    rc=$?
    if [ $rc -ne 0 ]; then
      echo "rep $r $v: FAILED (result line of bench.py not usable, parser exit $rc)" | tee -a "$out"; exit 1
    fi
  done
done
