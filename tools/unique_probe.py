"""Probe of the unique_* set functions on MI355X (development tool).

For 2^28 sorted float32 values in chunks of 2^22 and three inputs (all
distinct, 100 distinct values, all equal) it times, warmed up, with device
events, alternating in one process:

* the count launch (``core.ops.unique_count``: tile counts + their scan) and
  the pack launch (``core.ops.unique_pack``: tile counts, scan, pack), each one
  ``cubed_unique_chunks`` call;
* a cubed_copy_boxes copy of the same chunks, one read plus one write of the
  4 B values.  Count reads 4n bytes; pack reads 4n twice (count pass and pack
  pass) and writes at most 4n heads plus the zeroed tail, 4n in all;
* ``xp.unique_counts`` end to end (both phases and the computes of values and
  counts, host clock, device synchronised) against
  ``torch.unique(return_counts=True)`` of the same values.

    python tools/unique_probe.py [--reps 7] [--e2e-reps 3] [--out profiles/unique_probe.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, CHUNK = 2 ** 28, 2 ** 22
INPUTS = ("all distinct", "100 distinct", "all equal")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cubed_amd as cubed
    import cubed_amd.array_api as xp
    from cubed_amd.core import ops
    from cubed_amd.core.plan import arrays_to_plan
    from cubed_amd.lowering import Box, CopyLaunch, UniqueLaunch
    from cubed_amd.runtime.executors.gpu import GpuDagExecutor
    from cubed_amd.storage import DeviceArray

    n = 2 ** args.log2n
    chunk = min(CHUNK, n)
    dev = torch.device("cuda:0")
    results = []
    for kind in INPUTS:
        ex = GpuDagExecutor("cuda:0")
        spec = cubed.Spec(allowed_mem="288GB", executor=ex)
        i = torch.arange(n, dtype=torch.int32, device=dev)
        if kind == "all distinct":   # 1.0 and the n - 1 floats after it, bit pattern by bit pattern
            t_x = (i + 0x3F800000).view(torch.float32)
        elif kind == "100 distinct":
            t_x = (i.to(torch.int64) * 100 // n).to(torch.float32)
        else:
            t_x = torch.full((n,), 0.371, dtype=torch.float32, device=dev)
        del i
        X = DeviceArray((n,), np.float32, (chunk,), name=f"sorted-{kind.replace(' ', '-')}")
        X.allocate(dev)
        X.slabs[None].view(torch.float32)[:n].copy_(t_x)   # whole chunks: the slots are end to end
        X.written = True
        torch.cuda.synchronize()
        x = ops.from_device(X, spec)
        st = torch.cuda.current_stream().cuda_stream

        def launch_of(y):
            arrays_to_plan(y).execute(executor=ex, array_names=[y.name])
            (l,) = [l for step in ex.last_schedule.steps for l in step[1] if isinstance(l, UniqueLaunch)]
            return l

        cnt = ops.unique_count(x)
        pck = ops.unique_pack(x)
        count_launch, pack_launch = launch_of(cnt), launch_of(pck)

        dst = torch.empty(X.device_bytes(), dtype=torch.uint8, device=dev)
        boxes = []
        for key in np.ndindex(*X.numblocks):
            a = X.chunk_addr(key)
            boxes.append(Box(a, dst.data_ptr() + (a - X.base_addr()), [X.chunk_extent(key)[0]], [1], [1]))
        copy = CopyLaunch(boxes, 4, dev)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def ours():
            values, counts = xp.unique_counts(x)
            cubed.compute(values, counts, _return_in_memory_array=False)
            torch.cuda.synchronize()
            return values, counts

        def torchs():
            r = torch.unique(t_x, return_counts=True)
            torch.cuda.synchronize()
            return r

        # warm-up: code objects, torch's allocator
        for fn in (lambda: copy.run(st), lambda: count_launch.run(st), lambda: pack_launch.run(st)):
            fn()
        torch.cuda.synchronize()
        copy_ms, count_ms, pack_ms = [], [], []
        for _ in range(args.reps):
            copy_ms.append(timed(lambda: copy.run(st)))
            count_ms.append(timed(lambda: count_launch.run(st)))
            pack_ms.append(timed(lambda: pack_launch.run(st)))
        heads = int(cnt._read_stored().sum())
        print(f"# {kind}: launches timed, {heads} heads", flush=True)

        values, counts = ours()
        tv, tc = torchs()
        ok = bool(torch.equal(torch.from_numpy(values._read_stored()).to(dev), tv) and
                  torch.equal(torch.from_numpy(counts._read_stored()).to(dev), tc) and len(tv) == heads)
        del values, counts, tv, tc
        ours_ms, torch_ms = [], []
        for _ in range(args.e2e_reps):
            t0 = time.perf_counter()
            r = torchs()
            torch_ms.append((time.perf_counter() - t0) * 1e3)
            del r
            t0 = time.perf_counter()
            r = ours()
            ours_ms.append((time.perf_counter() - t0) * 1e3)
            del r

        cp, cn, pk = (float(np.median(v)) for v in (copy_ms, count_ms, pack_ms))
        om, tm = float(np.median(ours_ms)), float(np.median(torch_ms))
        out = dict(input=kind, n_values=n, chunk=chunk, dtype="float32", reps=args.reps, e2e_reps=args.e2e_reps,
                   heads=heads, work=count_launch.work, ntasks=count_launch.ntasks,
                   copy_ms=[round(v, 4) for v in copy_ms], copy_tb_s=round(2.0 * 4 * n / cp / 1e9, 3),
                   count_launch_ms=[round(v, 4) for v in count_ms], count_launch_median_ms=round(cn, 4),
                   count_launch_tb_s=round(4.0 * n / cn / 1e9, 3), count_launch_over_copy=round(cn / cp, 3),
                   pack_launch_ms=[round(v, 4) for v in pack_ms], pack_launch_median_ms=round(pk, 4),
                   pack_launch_over_copy=round(pk / cp, 3),
                   unique_counts_ms=[round(v, 3) for v in ours_ms], torch_unique_ms=[round(v, 3) for v in torch_ms],
                   unique_counts_over_torch=round(om / tm, 3),
                   check=dict(values_and_counts_equal_torch=ok))
        print(json.dumps(out), flush=True)
        results.append(out)
        del x, cnt, pck, count_launch, pack_launch, copy, dst, ex, X, t_x
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
