"""Probe of searchsorted on MI355X (development tool): per-launch times of the
recorded schedule of ``xp.searchsorted`` next to two yardsticks timed in the
same process, alternating with it, warmed up, with device events:

* a cubed_copy_boxes copy of the chunks of ``x2`` -- one read plus one write of
  its values;
* ``torch.searchsorted`` on tensors of the same shapes (int64 result).

Byte floor of one pass (one block of ``x1``): 4 B read and 8 B written per
element of ``x2`` (float32 values, int64 counts); every pass after the first
also reads the 8 B of the counts so far.  The sorted chunk itself is small next
to that and is left out.

    python tools/search_probe.py [--reps 5] [--cases a,b,c] [--out profiles/search_probe.json]
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    # name: (n_values, values chunk, n_sorted, sorted chunk, what it exercises)
    "a": (2 ** 28, 2 ** 22, 1000, 1000, "LDS path: 1000 edges staged whole by every workgroup"),
    "b": (2 ** 28, 2 ** 22, 2 ** 22, 2 ** 22, "split path: 4096 splitters, then a bucket of 1024 in global memory"),
    "c": (2 ** 28, 2 ** 22, 2 ** 24, 2 ** 22, "split path, four blocks of x1: four chained ops"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cubed_amd as cubed
    import cubed_amd.array_api as xp
    import cubed_amd.random as crandom
    from cubed_amd import _native as nat
    from cubed_amd.core.plan import arrays_to_plan
    from cubed_amd.lowering import Box, CopyLaunch
    from cubed_amd.runtime.executors.gpu import GpuDagExecutor, LaunchTimer
    from cubed_amd.storage import DeviceArray

    tile = nat.search_tile()
    results = []
    for case in args.cases.split(","):
        nv, vchunk, ns, schunk, what = CASES[case]
        ex = GpuDagExecutor("cuda:0")
        spec = cubed.Spec(allowed_mem="288GB", executor=ex)
        random.seed(7100)
        x2 = xp.astype(crandom.random((nv,), chunks=(vchunk,), spec=spec), xp.float32)
        sorted_host = np.sort(np.random.default_rng(7101).random(ns, dtype=np.float32))
        x1 = cubed.from_array(sorted_host, chunks=(schunk,), spec=spec)
        for a in (x1, x2):
            arrays_to_plan(a).execute(executor=ex, array_names=[a.name])
        torch.cuda.synchronize()
        X2 = x2.zarray

        # the copy of x2's chunks, one contiguous box each
        dst = torch.empty(X2.device_bytes(), dtype=torch.uint8, device="cuda:0")
        boxes = []
        for key in np.ndindex(*X2.numblocks):
            n = int(np.prod(X2.chunk_extent(key)))
            a = X2.chunk_addr(key)
            boxes.append(Box(a, dst.data_ptr() + (a - X2.base_addr()), [n], [1], [1]))
        copy = CopyLaunch(boxes, 4, torch.device("cuda:0"))
        st = torch.cuda.current_stream().cuda_stream
        # torch.searchsorted's inputs: the same values in one tensor each
        t_vals = torch.empty((nv,), dtype=torch.float32, device="cuda:0")
        t_vals.copy_(X2.slabs[None].view(torch.float32)[:nv])
        t_sorted = torch.from_numpy(sorted_host).to("cuda:0")

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        y = xp.searchsorted(x1, x2, side="right")
        plan = arrays_to_plan(y)
        keep = {id(X2), id(x1.zarray)}

        def step():
            for _, d in plan._finalize_dag().nodes(data=True):
                t = d.get("target")
                if isinstance(t, DeviceArray) and id(t) not in keep:
                    t.written = False
            plan.execute(executor=ex, resume=True, array_names=[y.name])

        def torch_search():
            r = torch.searchsorted(t_sorted, t_vals, right=True)
            del r

        # warm-up: lowering, code objects, the recorded schedule, torch's allocator
        for _ in range(2):
            step()
        copy.run(st)
        torch_search()
        torch.cuda.synchronize()
        print(f"# case {case}: warmed up", flush=True)
        replays0 = ex.replays
        ex.timing = LaunchTimer()
        copy_ms, torch_ms, step_ms, host_ms = [], [], [], []
        for _ in range(args.reps):
            copy_ms.append(timed(lambda: copy.run(st)))
            torch_ms.append(timed(torch_search))
            t0 = time.perf_counter()
            step_ms.append(timed(step))
            host_ms.append((time.perf_counter() - t0) * 1e3)
        summ = ex.timing.summary()
        ex.timing = None

        launches = [(f"{k[0]}#{k[1]}:{k[2]}", round(v[1], 4)) for k, v in summ.items()]
        searches = [ms for name, ms in launches if name.endswith("SearchLaunch")]
        gpu_ms = sum(ms for _, ms in launches)
        nb = -(-ns // schunk)
        assert len(searches) == nb
        pass_bytes = [nv * (4.0 + 8.0 + (8.0 if b else 0.0)) for b in range(nb)]
        cp, ts = float(np.median(copy_ms)), float(np.median(torch_ms))
        out = dict(case=case, what=what, n_values=nv, values_chunk=vchunk, n_sorted=ns, sorted_chunk=schunk,
                   dtype="float32", side="right", reps=args.reps, replayed=ex.replays - replays0, tile=tile,
                   values_per_workgroup=nat.SEARCH_VALUES, passes=nb,
                   launch_ms=dict(launches),
                   search_launch_ms=[round(v, 4) for v in searches],
                   search_launch_tb_s_over_floor_bytes=[round(b / ms / 1e9, 3) for b, ms in zip(pass_bytes, searches)],
                   first_pass_over_copy=round(searches[0] / cp, 3),
                   op_gpu_ms=round(gpu_ms, 4), op_event_ms=[round(v, 4) for v in step_ms],
                   op_host_ms=[round(v, 4) for v in host_ms],
                   op_tb_s_over_floor_bytes=round(sum(pass_bytes) / gpu_ms / 1e9, 3),
                   copy_ms=[round(v, 4) for v in copy_ms], copy_tb_s=round(2.0 * 4 * nv / cp / 1e9, 3),
                   torch_searchsorted_ms=[round(v, 4) for v in torch_ms],
                   torch_tb_s_over_floor_bytes=round(nv * 12.0 / ts / 1e9, 3),
                   op_over_copy=round(gpu_ms / cp, 3), op_over_torch_searchsorted=round(gpu_ms / ts, 3))
        # check of the first and the last chunk against numpy
        Y = y.zarray
        ok = True
        for key in ((0,), (X2.numblocks[0] - 1,)):
            ok = ok and bool(np.array_equal(Y.read_chunk(key),
                                            np.searchsorted(sorted_host, X2.read_chunk(key), side="right")))
        out["check"] = dict(first_and_last_chunk_equal_to_numpy=ok)
        print(json.dumps(out), flush=True)
        results.append(out)
        del x1, x2, y, plan, copy, dst, ex, X2, Y, t_vals, t_sorted
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
