#!/bin/bash
# One GPU session: smoke, GPU parity tests, bench, kernel-trace profile.
# Every GPU step has its own time limit; a crash/abort/timeout ends the session
# (test *failures* -- pytest exit 1 -- do not, so the bench still runs).
# Logs and results go to $OUT (default bench_out/, relative to the repository).
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${OUT:-bench_out}"
cd "$R" && mkdir -p "$OUT"
export TMPDIR=/tmp
step() { echo "== $1 $(date +%T)" >> "$OUT/steps.log"; }
fatal() { [ "$1" -ne 0 ] && [ "$1" -ne 1 ]; }
step smoke
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { echo smoke failed; tail -20 "$OUT/smoke.log"; exit 1; }
step pytest
timeout -k 10 900 python -m pytest tests -m gpu -q -p no:cacheprovider ${PYTEST_ARGS} > "$OUT/pytest_gpu.log" 2>&1
rc=$?
tail -15 "$OUT/pytest_gpu.log"
if fatal $rc; then echo "pytest-gpu crashed rc=$rc"; exit 1; fi
step bench
timeout -k 10 600 python bench.py ${BENCH_ARGS---full} > "$OUT/bench.json" 2> "$OUT/bench.err" || { echo bench failed; tail -20 "$OUT/bench.err"; exit 1; }
cat "$OUT/bench.json"
step prof
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/prof" -o run -- python3 "$R/bench.py" --steps 10 --warmup 2 > "$R/$OUT/prof.log" 2>&1 || { echo prof failed; tail -20 "$R/$OUT/prof.log"; exit 1; }
if [ -z "${NO_PMC}" ]; then
  step pmc
  cd /tmp && timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$R/$OUT/pmc_fetch" -o run -- python3 "$R/bench.py" --steps 5 --warmup 1 > "$R/$OUT/pmc_fetch.log" 2>&1 || { echo pmc fetch failed; tail -20 "$R/$OUT/pmc_fetch.log"; exit 1; }
  cd /tmp && timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$R/$OUT/pmc_write" -o run -- python3 "$R/bench.py" --steps 5 --warmup 1 > "$R/$OUT/pmc_write.log" 2>&1 || { echo pmc write failed; tail -20 "$R/$OUT/pmc_write.log"; exit 1; }
  cd "$R" && python tools/traffic.py "$OUT/pmc_fetch" "$OUT/pmc_write" cubed_stream_f32_l2_r1 > "$OUT/traffic.json" && cat "$OUT/traffic.json"
fi
echo all-done
