#!/bin/bash
# Round-end profile refresh on a 1-GPU MI355X box: kernel-trace stats of the
# whole bench (every extra), FETCH_SIZE / WRITE_SIZE passes -> per-kernel
# traffic.json, then the bench line itself reading that traffic.  Each step
# has its own time limit; any failure ends the script.
# Logs and results go to $OUT (default bench_out/, relative to the repository).
set -o pipefail
R="${GRAFT_REPO_ROOT:-$(pwd)}"
OUT="${OUT:-bench_out}"
cd "$R" && mkdir -p "$OUT"
export TMPDIR=/tmp
ARGS="--full --steps 5 --warmup 1 --no-cpu-baseline"
cd /tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/prof" -o run -- python3 "$R/bench.py" $ARGS > "$R/$OUT/prof.log" 2>&1 || { echo prof failed; tail -20 "$R/$OUT/prof.log"; exit 1; }
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$R/$OUT/pmc_fetch" -o run -- python3 "$R/bench.py" $ARGS > "$R/$OUT/pmc_fetch.log" 2>&1 || { echo pmc fetch failed; tail -20 "$R/$OUT/pmc_fetch.log"; exit 1; }
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$R/$OUT/pmc_write" -o run -- python3 "$R/bench.py" $ARGS > "$R/$OUT/pmc_write.log" 2>&1 || { echo pmc write failed; tail -20 "$R/$OUT/pmc_write.log"; exit 1; }
cd "$R"
python tools/traffic.py "$OUT/pmc_fetch" "$OUT/pmc_write" $TRAFFIC_KERNELS > "$OUT/traffic.json" || exit 1
cat "$OUT/traffic.json"
cp "$OUT/traffic.json" profiles/traffic.json
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { echo bench failed; tail -20 "$OUT/bench.err"; exit 1; }
tail -c 600 "$OUT/bench.json"
echo all-done
