"""Probe of sort on MI355X (development tool): per-launch times of the
recorded schedule of ``xp.sort`` next to two yardsticks timed in the same
process, alternating with it, warmed up, with device events:

* a cubed_copy_boxes copy of the same chunks -- one read plus one write of the
  array, the floor of any one pass;
* ``torch.sort`` of a tensor of the same shape along the same axis.

Algorithmic bytes: the tile sort and every merge pass inside a chunk read and
write each element once (2 * itemsize); in a round of the block network a
paired task reads two chunks and writes one (3 * itemsize per element written),
an unpaired one copies (2 * itemsize); a permute is 2 * itemsize.

    python tools/sort_probe.py [--reps 3] [--cases a,b,c] [--out profiles/sort_probe.json]
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    # name: (shape, chunks, axis, what it exercises)
    "a": ((1000, 720, 1440), (10, 720, 1440), 2, "tile sort only: rows of 1440, one block along the axis"),
    "b": ((1000, 720, 1440), (10, 720, 1440), 0, "two permutes, rows of 10, 28 merge rounds over 100 blocks"),
    "c": ((2 ** 28,), (2 ** 22,), 0, "1-d: 11 merge passes inside every chunk, 21 rounds over 64 blocks"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cubed_amd as cubed
    import cubed_amd.array_api as xp
    import cubed_amd.random as crandom
    from cubed_amd import _native as nat
    from cubed_amd.core.ops import sort_network
    from cubed_amd.core.plan import arrays_to_plan
    from cubed_amd.lowering import Box, CopyLaunch
    from cubed_amd.runtime.executors.gpu import GpuDagExecutor, LaunchTimer
    from cubed_amd.storage import DeviceArray

    tile = nat.sort_tile()
    results = []
    for case in args.cases.split(","):
        shape, chunks, axis, what = CASES[case]
        ex = GpuDagExecutor("cuda:0")
        spec = cubed.Spec(allowed_mem="288GB", executor=ex)
        random.seed(7000)
        x = xp.astype(crandom.random(shape, chunks=chunks, spec=spec), xp.float32)
        arrays_to_plan(x).execute(executor=ex, array_names=[x.name])
        torch.cuda.synchronize()
        itemsize = 4
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
        # torch.sort's input: values of the same distribution in one tensor (the
        # array's own slab, block after block)
        t_in = torch.empty(shape, dtype=torch.float32, device="cuda:0")
        t_in.view(-1).copy_(X.slabs[None].view(torch.float32)[:nelem])

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        y = xp.sort(x, axis=axis)
        plan = arrays_to_plan(y)
        keep = {id(X)}

        def step():
            for _, d in plan._finalize_dag().nodes(data=True):
                t = d.get("target")
                if isinstance(t, DeviceArray) and id(t) not in keep:
                    t.written = False
            plan.execute(executor=ex, resume=True, array_names=[y.name])

        def torch_sort():
            v, i = torch.sort(t_in, dim=axis, stable=True)
            del v, i

        # warm-up: lowering, code objects, the recorded schedule, torch's workspace
        for _ in range(2):
            step()
        copy.run(st)
        torch_sort()
        torch.cuda.synchronize()
        print(f"# case {case}: warmed up", flush=True)
        replays0 = ex.replays
        ex.timing = LaunchTimer()
        copy_ms, torch_ms, step_ms, host_ms = [], [], [], []
        for _ in range(args.reps):
            copy_ms.append(timed(lambda: copy.run(st)))
            torch_ms.append(timed(torch_sort))
            t0 = time.perf_counter()
            step_ms.append(timed(step))
            host_ms.append((time.perf_counter() - t0) * 1e3)
        summ = ex.timing.summary()
        ex.timing = None

        launches = [(f"{k[0]}#{k[1]}:{k[2]}", round(v[1], 4)) for k, v in summ.items()]
        sorts = [ms for name, ms in launches if name.endswith("SortLaunch")]
        others = [ms for name, ms in launches if not name.endswith("SortLaunch")]
        gpu_ms = sum(ms for _, ms in launches)
        # algorithmic bytes of every launch
        n_axis, c_axis = shape[axis], chunks[axis]
        passes = max(0, int(np.ceil(np.log2(np.ceil(c_axis / tile)))))
        chunk_bytes = 2.0 * itemsize * nelem * (1 + passes)
        nb = -(-n_axis // c_axis)
        sizes = [min(c_axis, n_axis - b * c_axis) for b in range(nb)]
        per_slice = nelem // n_axis
        round_bytes = []
        for rnd in sort_network(nb):
            paired = {b for pair in rnd for b in pair}
            elems = sum((sizes[lo] + sizes[hi]) * 1.5 for lo, hi in rnd) + \
                sum(sizes[b] for b in range(nb) if b not in paired)
            round_bytes.append(2.0 * itemsize * per_slice * elems)
        assert len(sorts) == 1 + len(round_bytes)
        op_bytes = chunk_bytes + sum(round_bytes) + 2.0 * itemsize * nelem * len(others)
        cp, ts = min(copy_ms), min(torch_ms)
        out = dict(case=case, what=what, shape=list(shape), chunks=list(chunks), axis=axis, dtype="float32",
                   reps=args.reps, replayed=ex.replays - replays0, tile=tile, passes_in_chunk=passes,
                   merge_rounds=len(round_bytes),
                   launch_ms=dict(launches),
                   chunk_launch_ms=round(sorts[0], 4),
                   chunk_launch_tb_s_over_algorithmic_bytes=round(chunk_bytes / sorts[0] / 1e9, 3),
                   chunk_launch_per_pass_over_copy=round(sorts[0] / (1 + passes) / cp, 3),
                   merge_round_ms_min_max=[round(min(sorts[1:]), 4), round(max(sorts[1:]), 4)] if sorts[1:] else None,
                   merge_round_tb_s_over_algorithmic_bytes=(
                       round(sum(round_bytes) / sum(sorts[1:]) / 1e9, 3) if sorts[1:] else None),
                   merge_round_over_copy=round(float(np.mean(sorts[1:])) / cp, 3) if sorts[1:] else None,
                   other_launches_ms=round(sum(others), 4),
                   op_gpu_ms=round(gpu_ms, 4), op_event_ms=[round(v, 4) for v in step_ms],
                   op_host_ms=[round(v, 4) for v in host_ms],
                   op_tb_s_over_algorithmic_bytes=round(op_bytes / gpu_ms / 1e9, 3),
                   copy_ms=[round(v, 4) for v in copy_ms], copy_tb_s=round(2.0 * itemsize * nelem / cp / 1e9, 3),
                   torch_sort_ms=[round(v, 4) for v in torch_ms],
                   op_over_copy=round(gpu_ms / cp, 3), op_over_torch_sort=round(gpu_ms / ts, 3))
        # sampled check against numpy: 8 positions along every other dim
        sub = tuple(slice(None) if d == axis else slice(0, 8) for d in range(len(shape)))
        Y = y.zarray
        keys = [tuple(b if d == axis else 0 for d in range(len(shape))) for b in range(nb)]
        got = np.concatenate([Y.read_chunk(k)[sub] for k in keys], axis=axis)
        src = np.concatenate([X.read_chunk(k)[sub] for k in keys], axis=axis)
        out["check"] = dict(sampled_equal_to_numpy=bool(np.array_equal(got, np.sort(src, axis=axis, kind="stable"))))
        print(json.dumps(out), flush=True)
        results.append(out)
        del x, y, plan, copy, dst, ex, X, Y, t_in
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
