"""Probe of nonzero / boolean-mask selection on MI355X (development tool).

For 2^28 float32 values in chunks of 2^22 and a 2^28-byte bool mask in the same
chunking, each with none, about half and all of the elements not zero, it
times, warmed up, with device events, alternating in one process:

* the select count launch (``core.ops.select_count``: tile counts + their
  scan) and the select pack launch of positions (``core.ops.select_pack``: tile
  counts, scan, pack), each one ``cubed_select_chunks`` call;
* a cubed_copy_boxes copy of the same chunks, one read plus one write of the
  elements.  Count reads the n elements once; pack reads them twice (count pass
  and pack pass) and writes 8n bytes, positions and the zeroed tail;
* for the float32 input the unique count launch (``core.ops.unique_count``) on
  the same buffer, which loads 4 B per lane;
* ``xp.nonzero`` end to end (both phases and the compute of the positions,
  host clock, device synchronised) against ``torch.nonzero`` of the same data.

    python tools/select_probe.py [--reps 7] [--e2e-reps 3] [--out profiles/select_probe.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK = 2 ** 22
DENSITIES = (0.0, 0.5, 1.0)


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
    from cubed_amd.lowering import Box, CopyLaunch, SelectLaunch, UniqueLaunch
    from cubed_amd.runtime.executors.gpu import GpuDagExecutor
    from cubed_amd.storage import DeviceArray

    n = 2 ** args.log2n
    chunk = min(CHUNK, n)
    dev = torch.device("cuda:0")
    results = []
    for dtype, tdtype in ((np.float32, torch.float32), (np.bool_, torch.bool)):
        esize = np.dtype(dtype).itemsize
        for density in DENSITIES:
            ex = GpuDagExecutor("cuda:0")
            spec = cubed.Spec(allowed_mem="288GB", executor=ex)
            gen = torch.Generator(device=dev)
            gen.manual_seed(7)
            t_x = (torch.rand(n, device=dev, generator=gen) < density).to(tdtype)
            X = DeviceArray((n,), dtype, (chunk,), name=f"select-{np.dtype(dtype).name}-{density}")
            X.allocate(dev)
            X.slabs[None].view(tdtype)[:n].copy_(t_x)   # whole chunks: the slots are end to end
            X.written = True
            torch.cuda.synchronize()
            x = ops.from_device(X, spec)
            st = torch.cuda.current_stream().cuda_stream

            def launch_of(y, cls):
                arrays_to_plan(y).execute(executor=ex, array_names=[y.name])
                (l,) = [l for step in ex.last_schedule.steps for l in step[1] if isinstance(l, cls)]
                return l

            cnt = ops.select_count(x)
            pck = ops.select_pack(x)
            launches = {"count": launch_of(cnt, SelectLaunch), "pack": launch_of(pck, SelectLaunch)}
            if dtype is np.float32:
                ucnt = ops.unique_count(x)
                launches["unique_count"] = launch_of(ucnt, UniqueLaunch)

            dst = torch.empty(X.device_bytes(), dtype=torch.uint8, device=dev)
            boxes = []
            for key in np.ndindex(*X.numblocks):
                a = X.chunk_addr(key)
                boxes.append(Box(a, dst.data_ptr() + (a - X.base_addr()), [X.chunk_extent(key)[0]], [1], [1]))
            launches["copy"] = CopyLaunch(boxes, esize, dev)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            def ours():
                (pos,) = xp.nonzero(x)
                cubed.compute(pos, _return_in_memory_array=False)
                torch.cuda.synchronize()
                return pos

            def torchs():
                r = torch.nonzero(t_x)
                torch.cuda.synchronize()
                return r

            # warm-up: code objects, torch's allocator
            for l in launches.values():
                l.run(st)
            torch.cuda.synchronize()
            ms = {name: [] for name in launches}
            for _ in range(args.reps):
                for name, l in launches.items():
                    ms[name].append(timed(lambda l=l: l.run(st)))
            selected = int(cnt._read_stored().sum())
            print(f"# {np.dtype(dtype).name} density {density}: launches timed, {selected} selected", flush=True)

            pos = ours()
            tp = torchs()
            got = pos._read_stored() if selected else np.zeros(0, dtype=np.int64)
            ok = bool(len(tp) == selected and torch.equal(torch.from_numpy(got).to(dev), tp.reshape(-1)))
            del pos, tp, got
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

            med = {name: float(np.median(v)) for name, v in ms.items()}
            om, tm = float(np.median(ours_ms)), float(np.median(torch_ms))
            out = dict(dtype=np.dtype(dtype).name, density=density, n=n, chunk=chunk, reps=args.reps,
                       e2e_reps=args.e2e_reps, selected=selected, work=launches["count"].work,
                       ntasks=launches["count"].ntasks,
                       copy_ms=[round(v, 4) for v in ms["copy"]], copy_median_ms=round(med["copy"], 4),
                       copy_tb_s=round(2.0 * esize * n / med["copy"] / 1e9, 3),
                       count_launch_ms=[round(v, 4) for v in ms["count"]],
                       count_launch_median_ms=round(med["count"], 4),
                       count_launch_tb_s=round(1.0 * esize * n / med["count"] / 1e9, 3),
                       count_launch_over_copy=round(med["count"] / med["copy"], 3),
                       pack_launch_ms=[round(v, 4) for v in ms["pack"]],
                       pack_launch_median_ms=round(med["pack"], 4),
                       pack_launch_over_copy=round(med["pack"] / med["copy"], 3),
                       nonzero_ms=[round(v, 3) for v in ours_ms], torch_nonzero_ms=[round(v, 3) for v in torch_ms],
                       nonzero_over_torch=round(om / tm, 3),
                       check=dict(positions_equal_torch=ok))
            if "unique_count" in med:
                out.update(unique_count_launch_ms=[round(v, 4) for v in ms["unique_count"]],
                           unique_count_launch_median_ms=round(med["unique_count"], 4),
                           count_launch_over_unique_count=round(med["count"] / med["unique_count"], 3))
            print(json.dumps(out), flush=True)
            results.append(out)
            del x, cnt, pck, launches, dst, ex, X, t_x
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
