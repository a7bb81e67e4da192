#!/bin/bash
# GPU session for the distributed executor: 2/3 ranks sharing the box's one
# GPU (gloo-staged collectives), the whole -m gpu suite, and a 2-rank bench
# rehearsal.  Each GPU step has its own limit; a crash ends the session.
# Logs and results go to $OUT (default bench_out/).
set -o pipefail
OUT="${OUT:-bench_out}"
mkdir -p "$OUT"
export TMPDIR=/tmp
fatal() { [ "$1" -ne 0 ] && [ "$1" -ne 1 ]; }
timeout -k 10 900 python -u -m pytest tests/test_gpu_dist.py -x -v -p no:cacheprovider --timeout 600 --timeout-method thread > "$OUT/dist.log" 2>&1
rc=$?; tail -30 "$OUT/dist.log"; if fatal $rc; then echo "dist crashed rc=$rc"; exit 1; fi
timeout -k 10 900 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 600 --timeout-method thread --ignore=tests/test_gpu_dist.py > "$OUT/pytest_gpu.log" 2>&1
rc=$?; tail -15 "$OUT/pytest_gpu.log"; if fatal $rc; then echo "pytest-gpu crashed rc=$rc"; exit 1; fi
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29611 bench.py --full --gpus 2 --backend gloo --t-length 100 --steps 3 --warmup 1 --no-cpu-baseline > "$OUT/bench2.json" 2> "$OUT/bench2.err" || { echo bench2 failed; tail -30 "$OUT/bench2.err"; exit 1; }
cat "$OUT/bench2.json"
echo all-done
