"""Probe of cumulative_sum on MI355X (development tool): per-launch times of
the recorded schedule, the scan pass against a cubed_copy_boxes copy of the
same array (the project's one-read-one-write kernel, timed in the same
process), and the whole op against its algorithmic bytes per element:
3 * itemsize (totals read + scan read + scan write), or 2 * itemsize when the
axis has one block and the plan is the scan alone.

    python tools/scan_probe.py [--reps 10] [--cases a,b,c,d] [--out profiles/scan_probe.json]
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    # name: (shape, chunks, axis, dtype, what it exercises)
    "a": ((1000, 720, 1440), (10, 720, 1440), 0, "float32", "cols kernel, carry over 100 blocks"),
    "b": ((1000, 720, 1440), (10, 720, 1440), 2, "float32", "rows kernel, n = 1440, one block along the axis"),
    "c": ((2000, 5000), (100, 5000), 0, "float64", "cols kernel, f64"),
    "d": ((2 ** 28,), (2 ** 22,), 0, "float32", "1-d: one wave per chunk (known weak case)"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cubed_amd as cubed
    import cubed_amd.array_api as xp
    import cubed_amd.random as crandom
    from cubed_amd.core.plan import arrays_to_plan
    from cubed_amd.lowering import Box, CopyLaunch
    from cubed_amd.runtime.executors.gpu import GpuDagExecutor, LaunchTimer
    from cubed_amd.storage import DeviceArray

    results = []
    for case in args.cases.split(","):
        shape, chunks, axis, dt, what = CASES[case]
        ex = GpuDagExecutor("cuda:0")
        spec = cubed.Spec(allowed_mem="288GB", executor=ex)
        random.seed(7000)
        x = crandom.random(shape, chunks=chunks, spec=spec)
        if dt == "float32":
            x = xp.astype(x, xp.float32)
        arrays_to_plan(x).execute(executor=ex, array_names=[x.name])
        torch.cuda.synchronize()
        itemsize = np.dtype(dt).itemsize
        nelem = int(np.prod(shape))

        # the copy of the same chunks, one contiguous box each
        X = x.zarray
        dst = torch.empty(X.device_bytes(), dtype=torch.uint8, device="cuda:0")
        boxes = []
        for key in np.ndindex(*X.numblocks):
            n = int(np.prod(X.chunk_extent(key)))
            a = X.chunk_addr(key)
            boxes.append(Box(a, dst.data_ptr() + (a - X.base_addr()), [n], [1], [1]))
        copy = CopyLaunch(boxes, itemsize, torch.device("cuda:0"))
        st = torch.cuda.current_stream().cuda_stream

        def time_copy():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                copy.run(st)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.reps

        copy.run(st)
        torch.cuda.synchronize()
        copy_ms_before = time_copy()

        y = xp.cumulative_sum(x, axis=axis)
        plan = arrays_to_plan(y)
        keep = {id(X)}

        def step():
            for _, d in plan._finalize_dag().nodes(data=True):
                t = d.get("target")
                if isinstance(t, DeviceArray) and id(t) not in keep:
                    t.written = False
            plan.execute(executor=ex, resume=True, array_names=[y.name])

        for _ in range(2):  # warm-up: lowering, code objects, the recorded schedule
            step()
        torch.cuda.synchronize()
        replays0 = ex.replays
        ex.timing = LaunchTimer()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            step()
        torch.cuda.synchronize()
        plan_ms = (time.perf_counter() - t0) / args.reps * 1e3
        summ = ex.timing.summary()
        ex.timing = None
        copy_ms_after = time_copy()
        copy_ms = min(copy_ms_before, copy_ms_after)

        launches = [(f"{k[0]}#{k[1]}:{k[2]}", round(v[1], 4)) for k, v in summ.items()]
        scans = [ms for name, ms in launches if name.endswith("ScanLaunch")]
        scan_ms = scans[-1]  # the full-size pass (the one before it, if any, scans the totals)
        gpu_ms = sum(ms for _, ms in launches)
        rw = 2.0 * itemsize * nelem
        op_items = 3 if X.numblocks[axis] > 1 else 2
        out = dict(case=case, what=what, shape=list(shape), chunks=list(chunks), axis=axis, dtype=dt,
                   reps=args.reps, replayed=ex.replays - replays0,
                   launches_ms=dict(launches),
                   scan_ms=round(scan_ms, 4), scan_tb_s=round(rw / scan_ms / 1e9, 3),
                   copy_ms=round(copy_ms, 4), copy_tb_s=round(rw / copy_ms / 1e9, 3),
                   copy_ms_before_after=[round(copy_ms_before, 4), round(copy_ms_after, 4)],
                   scan_over_copy=round(scan_ms / copy_ms, 3),
                   op_gpu_ms=round(gpu_ms, 4), op_host_ms=round(plan_ms, 4),
                   op_itemsizes_per_element=op_items,
                   op_tb_s=round(op_items * itemsize * nelem / gpu_ms / 1e9, 3))
        # sampled check of the last plane / row tail against f64 numpy
        # (8 positions along every other dim of the last row of blocks)
        sub = tuple(slice(None) if d == axis else slice(0, 8) for d in range(len(shape)))
        got = y.zarray.read_chunk(tuple(n - 1 for n in y.zarray.numblocks))[sub]
        src_keys = [tuple(n - 1 if d != axis else b for d, n in enumerate(X.numblocks))
                    for b in range(X.numblocks[axis])]
        col = np.concatenate([X.read_chunk(k)[sub].astype(np.float64) for k in src_keys], axis=axis)
        ref = np.cumsum(col, axis=axis)
        A = np.cumsum(np.abs(col), axis=axis)
        tail = [slice(None)] * len(shape)
        tail[axis] = slice(ref.shape[axis] - got.shape[axis], None)
        err = np.abs(got.astype(np.float64) - ref[tuple(tail)])
        bound = 4 * shape[axis] * 2.0 ** -53 * A[tuple(tail)]
        if dt == "float32":
            bound = bound + 2.0 ** -24 * np.abs(ref[tuple(tail)]) * (1 + 1e-6)
        out["check"] = dict(max_err=float(err.max()), within_bound=bool(np.all(err <= bound)))
        print(json.dumps(out), flush=True)
        results.append(out)
        del x, y, plan, copy, dst, ex, X
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
