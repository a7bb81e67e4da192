"""Probe of histogram on MI355X (development tool): per-launch times of the
recorded schedule of ``xp.histogram`` next to two yardsticks timed in the same
process, alternating with it, warmed up, with device events:

* a cubed_copy_boxes copy of the chunks of ``x`` -- one read plus one write of
  its values, the streaming bound of the machine as this library reaches it;
* ``torch.histc`` on a tensor of the same values where the bins are evenly
  spaced, and for explicit edges ``torch.histogram`` if the device has it, else
  ``torch.bucketize`` + ``torch.bincount`` (named in the output).

Byte floor: the 4 B of every float32 value, read once; the counts are small
next to that.  The roofline time is those bytes over 8 TB/s.

    python tools/hist_probe.py [--reps 7] [--cases a,b,c,d,e,f] [--out profiles/hist_probe.json]
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, CHUNK, LO, HI = 2 ** 28, 2 ** 22, 0.0, 1.0
CASES = {
    # name: (bins, explicit edges, input, what it exercises)
    "a": (100, False, "random", "lds-uniform: 100 evenly spaced bins"),
    "b": (4096, False, "random", "lds-uniform at the LDS limit: 4096 bins, 32 KiB of LDS"),
    "c": (1000, True, "random", "lds-search: 1000 explicit edges, binary search in LDS"),
    "d": (100000, False, "random", "wide: binary search in global memory, one global atomic per run"),
    "e": (100, False, "constant", "lds-uniform, every value in one bin: one LDS add per wave and step"),
    "f": (100, False, "alternating",
          "lds-uniform, two bins alternating every 4 values: no two neighbouring lanes agree, so the "
          "merge finds nothing and 32 lanes add to each of two LDS words"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="a,b,c,d,e,f")
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

    results = []
    for case in args.cases.split(","):
        nbins, explicit, kind, what = CASES[case]
        ex = GpuDagExecutor("cuda:0")
        spec = cubed.Spec(allowed_mem="288GB", executor=ex)
        random.seed(7200)
        if kind == "random":
            x = xp.astype(crandom.random((N,), chunks=(CHUNK,), spec=spec), xp.float32)
        elif kind == "constant":
            x = cubed.from_array(np.full(N, 0.371, np.float32), chunks=(CHUNK,), spec=spec)
        else:
            x = cubed.from_array(np.tile(np.array([0.371] * 4 + [0.622] * 4, np.float32), N // 8),
                                 chunks=(CHUNK,), spec=spec)
        arrays_to_plan(x).execute(executor=ex, array_names=[x.name])
        torch.cuda.synchronize()
        X = x.zarray
        edges = np.histogram_bin_edges(np.empty(0, np.float32), nbins, (LO, HI))
        if explicit:  # uneven: squared spacing
            edges = (np.linspace(0, 1, nbins + 1) ** 2).astype(np.float32)
        bins = edges if explicit else nbins

        # the copy of x's chunks, one contiguous box each
        dst = torch.empty(X.device_bytes(), dtype=torch.uint8, device="cuda:0")
        boxes = []
        for key in np.ndindex(*X.numblocks):
            n = int(np.prod(X.chunk_extent(key)))
            a = X.chunk_addr(key)
            boxes.append(Box(a, dst.data_ptr() + (a - X.base_addr()), [n], [1], [1]))
        copy = CopyLaunch(boxes, 4, torch.device("cuda:0"))
        st = torch.cuda.current_stream().cuda_stream
        t_x = torch.empty((N,), dtype=torch.float32, device="cuda:0")
        t_x.copy_(X.slabs[None].view(torch.float32)[:N])
        t_edges = torch.from_numpy(edges).to("cuda:0")

        torch_name = "torch.histc"
        if explicit:
            try:
                torch.histogram(t_x[:1024], bins=t_edges)
                torch_name = "torch.histogram"
            except Exception:  # not implemented for the device
                torch_name = "torch.bucketize+torch.bincount"

        def torch_hist():
            if torch_name == "torch.histc":
                r = torch.histc(t_x, bins=nbins, min=LO, max=HI)
            elif torch_name == "torch.histogram":
                r = torch.histogram(t_x, bins=t_edges)
            else:
                r = torch.bincount(torch.bucketize(t_x, t_edges, right=True), minlength=nbins + 2)
            del r

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        hist, _ = xp.histogram(x, bins, range=(LO, HI))
        plan = arrays_to_plan(hist)
        keep = {id(X)}

        def step():
            for _, d in plan._finalize_dag().nodes(data=True):
                t = d.get("target")
                if isinstance(t, DeviceArray) and id(t) not in keep:
                    t.written = False
            plan.execute(executor=ex, resume=True, array_names=[hist.name])

        # warm-up: lowering, code objects, the recorded schedule, torch's allocator
        for _ in range(2):
            step()
        copy.run(st)
        torch_hist()
        torch.cuda.synchronize()
        print(f"# case {case}: warmed up", flush=True)
        replays0 = ex.replays
        ex.timing = LaunchTimer()
        copy_ms, torch_ms, step_ms, host_ms = [], [], [], []
        for _ in range(args.reps):
            copy_ms.append(timed(lambda: copy.run(st)))
            torch_ms.append(timed(torch_hist))
            t0 = time.perf_counter()
            step_ms.append(timed(step))
            host_ms.append((time.perf_counter() - t0) * 1e3)
        summ = ex.timing.summary()
        per_launch = {}
        for key, a, b in ex.timing.records:
            per_launch.setdefault(f"{key[0]}#{key[1]}:{key[2]}", []).append(a.elapsed_time(b))
        ex.timing = None

        launches = [(f"{k[0]}#{k[1]}:{k[2]}", round(v[1], 4)) for k, v in summ.items()]
        (hist_name,) = [name for name, _ in launches if name.endswith("HistLaunch")]
        hist_ms = float(np.median(per_launch[hist_name]))
        gpu_ms = sum(float(np.median(v)) for v in per_launch.values())
        cp, ts = float(np.median(copy_ms)), float(np.median(torch_ms))
        roof_ms = 4.0 * N / 8e12 * 1e3
        got = hist.compute()
        # the counts of everything in range, and the first chunk alone against numpy
        in_range = int(((t_x >= LO) & (t_x <= HI)).sum().item())
        first = X.read_chunk((0,))
        small, _ = xp.histogram(cubed.from_array(first, chunks=first.shape, spec=spec), bins, range=(LO, HI))
        ok = bool(np.array_equal(small.compute(), np.histogram(first, bins, range=(LO, HI))[0]))
        out = dict(case=case, what=what, n_values=N, chunk=CHUNK, nbins=nbins, explicit_edges=explicit, input=kind,
                   dtype="float32", reps=args.reps, replayed=ex.replays - replays0,
                   bins_lds=nat.hist_bins_lds(), launch_ms=dict(launches),
                   hist_launch_ms=[round(v, 4) for v in per_launch[hist_name]],
                   hist_launch_median_ms=round(hist_ms, 4),
                   hist_launch_tb_s=round(4.0 * N / hist_ms / 1e9, 3),
                   roofline_ms_at_8_tb_s=round(roof_ms, 4), hist_launch_over_roofline=round(hist_ms / roof_ms, 3),
                   op_gpu_ms=round(gpu_ms, 4), op_event_ms=[round(v, 4) for v in step_ms],
                   op_host_ms=[round(v, 4) for v in host_ms],
                   copy_ms=[round(v, 4) for v in copy_ms], copy_tb_s=round(2.0 * 4 * N / cp / 1e9, 3),
                   torch_yardstick=torch_name, torch_ms=[round(v, 4) for v in torch_ms],
                   hist_launch_over_copy=round(hist_ms / cp, 3), hist_launch_over_torch=round(hist_ms / ts, 3),
                   op_over_copy=round(gpu_ms / cp, 3), op_over_torch=round(gpu_ms / ts, 3),
                   check=dict(sum_equals_values_in_range=bool(int(got.sum()) == in_range),
                              first_chunk_equal_to_numpy=ok, most_in_one_bin=int(got.max())))
        print(json.dumps(out), flush=True)
        results.append(out)
        del x, hist, small, plan, copy, dst, ex, X, t_x, t_edges
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
