"""Probe of take_along_axis on MI355X (development tool): times of the gather
launches the executor would make for five float32 cases of 2^26 elements, next
to two yardsticks timed in the same process, alternating with them, warmed up,
with device events:

* a cubed_copy_boxes copy of the output's bytes -- one read plus one write;
* ``torch.take_along_axis`` on tensors of the same shapes.

Where the host picks the LDS form the same table is also timed with the direct
form forced, which is the measurement the path rule rests on.

Byte floor of one pass (one block of the axis): 8 B of index and 4 B of source
read and 4 B written per output element; every pass after the first also reads
the 4 B of the result so far.

    python tools/gather_probe.py [--reps 7] [--cases a,b,c,d,e] [--out profiles/gather_probe.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    # name: (shape of x and of the indices, axis, blocks of x along the axis, indices, what it exercises)
    "a": ((64, 2 ** 20), 1, 1, "identity", "identity, last axis, one chunk: direct form, coalesced reads"),
    "b": ((16384, 4096), 1, 1, "permutation", "a random permutation of rows of 4096: the LDS form (and direct, forced)"),
    "c": ((64, 2 ** 20), 1, 1, "permutation", "a random permutation of rows of 2^20: direct form over 4 MiB rows"),
    "d": ((4096, 16384), 0, 1, "random", "axis 0 of (4096, 16384): inner = 16384, lanes along the inner dimension"),
    "e": ((4096, 16384), 0, 4, "random", "the same in four blocks of the axis: four chained passes"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="a,b,c,d,e")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from cubed_amd import _native as nat
    from cubed_amd.lowering import Box, CopyLaunch, GatherLaunch

    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    results = []

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stats(ms):
        return dict(median=round(float(np.median(ms)), 4), min=round(min(ms), 4), max=round(max(ms), 4))

    for case in args.cases.split(","):
        shape, axis, nb, kind, what = CASES[case]
        n = shape[axis]
        total = shape[0] * shape[1]
        g = torch.Generator(device=dev)
        g.manual_seed(9100)
        x = torch.rand(shape, device=dev, generator=g, dtype=torch.float32)
        if kind == "identity":
            idx = torch.arange(n, device=dev, dtype=torch.int64).expand(shape).contiguous()
        elif kind == "permutation":
            idx = torch.argsort(torch.rand(shape, device=dev, generator=g), dim=axis)
        else:
            idx = torch.randint(0, n, shape, device=dev, generator=g, dtype=torch.int64)
        # x in nb blocks along the axis, each a compact chunk of its own
        step = n // nb
        blocks = [x.narrow(axis, b * step, step).contiguous() for b in range(nb)]
        bufs = [torch.empty(shape, device=dev, dtype=torch.float32) for _ in range(min(nb, 2))]
        outer = shape[0] if axis == 1 else 1
        inner = 1 if axis == 1 else shape[1]

        def table(b, path=None):
            rows = np.zeros(1, dtype=nat.GATHER_TASK_DTYPE)
            r = rows[0]
            r["src_base"], r["idx_base"] = blocks[b].data_ptr(), idx.data_ptr()
            r["dst_base"] = bufs[b % len(bufs)].data_ptr()
            r["prev_base"] = bufs[(b - 1) % len(bufs)].data_ptr() if b else 0
            r["outer"], r["n_idx"], r["n_src"], r["inner"] = outer, n, step, inner
            r["lo"], r["n_total"] = b * step, n
            return GatherLaunch(rows, 4, dev, path=path)

        chosen = [table(b) for b in range(nb)]
        forms = {"chosen": chosen}
        if all(l.path == nat.GATHER_LDS for l in chosen):
            forms["direct_forced"] = [table(b, nat.GATHER_DIRECT) for b in range(nb)]
        result_buf = bufs[(nb - 1) % len(bufs)]

        copy_dst = torch.empty(shape, device=dev, dtype=torch.float32)
        piece = 2 ** 22  # one box per run of 2^22 elements, as the chunks of the other probes
        copy = CopyLaunch([Box(x.data_ptr() + 4 * o, copy_dst.data_ptr() + 4 * o, [piece], [1], [1])
                           for o in range(0, total, piece)], 4, dev)

        def torch_gather():
            r = torch.take_along_dim(x, idx, dim=axis)
            del r

        def run(launches):
            for l in launches:
                l.run(st)

        for _ in range(2):  # warm-up: code objects, torch's allocator
            for launches in forms.values():
                run(launches)
            copy.run(st)
            torch_gather()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        per_pass = {k: [[] for _ in range(nb)] for k in forms}
        copy_ms, torch_ms = [], []
        for _ in range(args.reps):
            copy_ms.append(timed(lambda: copy.run(st)))
            torch_ms.append(timed(torch_gather))
            for k, launches in forms.items():
                ms[k].append(timed(lambda: run(launches)))
                for b, l in enumerate(launches):
                    per_pass[k][b].append(timed(lambda: l.run(st)))
        # the last form timed left its result in result_buf
        ok = bool(torch.equal(result_buf, torch.take_along_dim(x, idx, dim=axis)))
        pass_bytes = [total * (8.0 + 4.0 + 4.0 + (4.0 if b else 0.0)) for b in range(nb)]
        cp, ts = float(np.median(copy_ms)), float(np.median(torch_ms))
        out = dict(case=case, what=what, shape=list(shape), axis=axis, blocks=nb, indices=kind, dtype="float32",
                   reps=args.reps, tile_bytes=nat.gather_tile_bytes(),
                   path=["direct", "lds"][chosen[0].path], work=[l.work for l in chosen],
                   copy_ms=stats(copy_ms), copy_tb_s=round(2.0 * 4 * total / cp / 1e9, 3),
                   torch_take_along_dim_ms=stats(torch_ms), check=dict(equal_to_torch=ok))
        for k in forms:
            med = float(np.median(ms[k]))
            out[k] = dict(op_ms=stats(ms[k]), pass_ms=[stats(p) for p in per_pass[k]],
                          tb_s_over_floor_bytes=round(sum(pass_bytes) / med / 1e9, 3),
                          over_copy=round(med / cp, 3), over_torch=round(med / ts, 3))
        print(json.dumps(out), flush=True)
        results.append(out)
        del x, idx, blocks, bufs, copy_dst, copy, forms, chosen
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
