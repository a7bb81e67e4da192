"""The unique_* set functions on CPU: the API rules, the plans of the run-head
ops and of the gather, the pieces the gather reads, the task tables they lower
to (nothing is launched) and the binding.

The values themselves are checked on the GPU (tests/test_gpu_unique.py)."""

import os
import subprocess

import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
import cubed_amd.lowering as Lw
from cubed_amd import _native as nat
from cubed_amd import ir
from cubed_amd.core import ops
from cubed_amd.core.plan import arrays_to_plan
from cubed_amd.primitive.blockwise import apply_blockwise
from cubed_amd.storage import DeviceArray
from dryrun import DryExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("unique_values", "unique_counts", "unique_inverse", "unique_all")


class UniqueDryExecutor(DryExecutor):
    """DryExecutor that also records (instead of running) the sort and
    run-head launches."""

    def execute_dag(self, *args, **kwargs):
        saved = {cls: cls.run for cls in (Lw.UniqueLaunch, Lw.SortLaunch, Lw.SearchLaunch)}
        for cls in saved:
            cls.run = lambda launch, stream, _log=self.launched: _log.append(launch)
        try:
            return super().execute_dag(*args, **kwargs)
        finally:
            for cls, fn in saved.items():
                cls.run = fn


@pytest.fixture
def udry(built):
    return UniqueDryExecutor()


def _spec(ex=None, allowed_mem="2GB", reserved_mem="100MB"):
    return cubed.Spec(allowed_mem=allowed_mem, reserved_mem=reserved_mem, executor=ex)


def _arr(shape, chunks, dtype, spec):
    return cubed.from_array(np.zeros(shape, dtype=dtype), chunks=chunks, spec=spec)


def _ops(dag, kind=None):
    """(name, program, primitive op) of the blockwise ops, in topological order."""
    import networkx as nx

    out = []
    for name in nx.topological_sort(dag):
        p = dag.nodes[name].get("pipeline")
        if p is not None and p.function is apply_blockwise and (kind is None or isinstance(p.config.function, kind)):
            out.append((name, p.config.function, dag.nodes[name]["primitive_op"]))
    return out


def _lower(udry, *ys):
    udry.launched.clear()
    arrays_to_plan(*ys).execute(executor=udry, array_names=[y.name for y in ys])
    return [l for l in udry.launched if isinstance(l, Lw.UniqueLaunch)]


# ------------------------------------------------------------------ API rules


def test_all_four_are_exported():
    for name in FUNCS:
        assert callable(getattr(xp, name)) and name in dir(xp)
    for name in ("unique_count", "unique_pack", "unique_gather", "from_device"):
        assert callable(getattr(cubed.core, name)) and name in cubed.core.__all__


@pytest.mark.parametrize("dt", ["bfloat16", "complex64", "complex128"])
@pytest.mark.parametrize("func", FUNCS)
def test_rejected_input_dtypes(func, dt):
    spec = _spec()
    bad = xp.astype(_arr((6,), (2,), np.float32, spec), getattr(xp, dt))
    with pytest.raises(TypeError, match=func):
        getattr(xp, func)(bad)


@pytest.mark.parametrize("dt", [np.float32, np.int8, np.bool_, np.uint64])
def test_empty_input_computes_nothing(udry, dt):
    spec = _spec(udry)
    for shape, chunks in (((0,), (1,)), ((3, 0), (2, 1))):
        x = _arr(shape, chunks, dt, spec)
        res = xp.unique_all(x)
        assert res._fields == ("values", "indices", "inverse_indices", "counts")
        assert xp.unique_counts(x)._fields == ("values", "counts")
        assert xp.unique_inverse(x)._fields == ("values", "inverse_indices")
        assert res.values.shape == (0,) and res.values.dtype == np.dtype(dt)
        assert res.indices.shape == (0,) and res.indices.dtype == np.int64
        assert res.counts.shape == (0,) and res.counts.dtype == np.int64
        assert res.inverse_indices.shape == shape and res.inverse_indices.dtype == np.int64
        assert res.inverse_indices.chunks == x.chunks
        v = xp.unique_values(x)
        assert v.shape == (0,) and v.dtype == np.dtype(dt)
        for a in tuple(res) + (v,):
            assert not _ops(a.plan.dag, (ir.SortProgram, ir.UniqueProgram, ir.SearchProgram))
            got = a.compute()
            assert got.shape == a.shape and got.dtype == a.dtype
    assert udry.launched == []


def test_nd_input_is_flattened_through_whole_rows():
    from cubed_amd.array_api.set_functions import _ravel

    spec = _spec()
    for shape, chunks, flat in (((37, 46), (10, 16), (138,) * 12 + (46,)), ((5, 3, 7), (2, 2, 3), (21,) * 5),
                                ((4, 1), (2, 1), (2, 2)), ((1, 9), (1, 4), (9,)), ((6,), (4,), (4, 2)),
                                ((2, 50), (2, 10), (50, 50))):
        f = _ravel(_arr(shape, chunks, np.float32, spec))
        assert f.shape == (int(np.prod(shape)),) and f.chunks == (flat,), (shape, f.chunks)
        # block b of the flat array is block b of the rows: C order is kept
        assert not _ops(f.plan.dag, (ir.SortProgram, ir.UniqueProgram))


# ------------------------------------------------------------------ plans of count and pack


@pytest.mark.parametrize("nb", [1, 2, 5])
def test_count_and_pack_are_one_op_each(nb):
    spec = _spec()
    c = 1000
    n = (nb - 1) * c + 37
    s = _arr((n,), (c,), np.float32, spec)
    sp = ops.sort(_arr((n,), (c,), np.float64, spec), 0, False, True, True)
    assert sp.dtype == ir.sort_pairs_dtype(np.float64) and sp.numblocks == (nb,)
    c = s.chunksize[0]                                   # 37 for one block
    tile_scratch = Lw.unique_scratch_bytes(c, nat.UNIQUE_TILE)
    cases = [
        (ops.unique_count(s), "count", False, None, np.dtype(np.int64), (nb,), ((1,) * nb,), 4),
        (ops.unique_pack(s), "pack", False, None, np.dtype(np.float32), (n,), s.chunks, 4),
        (ops.unique_pack(s, False, "position"), "pack", False, "position", ir.sort_pairs_dtype(np.float32),
         (n,), s.chunks, 4),
        (ops.unique_count(sp, True), "count", True, None, np.dtype(np.int64), (nb,), ((1,) * nb,), 16),
        (ops.unique_pack(sp, True, "index"), "pack", True, "index", ir.sort_pairs_dtype(np.float64),
         (n,), sp.chunks, 16),
        (ops.unique_pack(sp, True, "position"), "pack", True, "position", ir.sort_pairs_dtype(np.float64),
         (n,), sp.chunks, 16),
    ]
    for y, kind, pairs, payload, dtype, shape, chunks, in_item in cases:
        assert y.shape == shape and y.dtype == dtype and y.chunks == chunks
        for dag in (y.plan.dag, y.plan._finalize_dag(optimize_graph=True)):
            ((name, prog, op),) = _ops(dag, ir.UniqueProgram)
            assert (prog.kind, prog.pairs, prog.payload) == (kind, pairs, payload)
            assert op.fusable is False and op.num_tasks == nb
            cfg = op.pipeline.config
            for b in range(nb):
                keys = cfg.block_function(("out", b))
                assert all(isinstance(k, tuple) for k in keys)      # whole single chunks
                assert len({k[0] for k in keys}) == 1               # of the one sorted array
                assert [k[1] for k in keys] == ([0] if b == 0 else [b, b - 1])
            # two copies of the chunk, of the chunk before it and of the output chunk, and the tile counts
            out_chunk = 8 if kind == "count" else c * dtype.itemsize
            assert op.projected_mem == 100_000_000 + 4 * c * in_item + 2 * out_chunk + tile_scratch
            assert op.projected_mem <= op.allowed_mem
    with pytest.raises(ValueError, match="payload"):
        ops.unique_pack(s, False, "index")
    with pytest.raises(ValueError, match="payload"):
        ops.unique_pack(s, False, "first")
    with pytest.raises(TypeError, match="pairs"):
        ops.unique_count(s, True)
    with pytest.raises(ValueError, match="allowed_mem"):
        ops.unique_pack(_arr((5000,), (2500,), np.float64, _spec(allowed_mem=60_000, reserved_mem=0)))


def test_sort_can_hand_back_the_pairs():
    spec = _spec()
    x = _arr((50,), (20,), np.int32, spec)
    idx = ops.sort(x, 0, False, True)
    assert idx.dtype == np.int64                                     # argsort is as it was
    pairs = ops.sort(x, 0, False, True, True)
    assert pairs.dtype == ir.sort_pairs_dtype(np.int32) and pairs.chunks == x.chunks
    assert len(_ops(pairs.plan.dag, ir.SortProgram)) == len(_ops(idx.plan.dag, ir.SortProgram))
    assert len(_ops(idx.plan.dag)) == len(_ops(pairs.plan.dag)) + 1  # the index field's extraction
    with pytest.raises(ValueError, match="return_pairs"):
        ops.sort(x, 0, False, False, True)
    with pytest.raises(ValueError, match="return_pairs"):
        ops.sort(_arr((6, 4), (3, 4), np.int32, spec), 0, False, True, True)


# ------------------------------------------------------------------ the gather


def _gather_cases():
    c = 8
    full = [c] * 4
    yield c, [3, 0, 2], "k < c, a zero"
    yield c, [0, 0, 5, 0], "zeros at both ends"
    yield c, [1, 0, 0, 7, 0], "k == c"
    yield c, [c], "one block, full"
    yield c, full, "all blocks full: k a multiple of c"
    yield c, [c, 0, c, 1], "k a multiple of c plus 1"
    yield c, [1] * 19, "every block contributes one head"
    yield c, [1, c, 0, 1, c, 2, 0, 0, 3], "pieces straddle output chunks"
    yield 5, [5, 5, 5, 3], "ragged last chunk full"


@pytest.mark.parametrize("c,counts,what", list(_gather_cases()))
def test_gather_pieces_reassemble_the_prefixes(c, counts, what):
    nb = len(counts)
    last = max(counts[-1], 3) if c == 5 else c
    n = (nb - 1) * c + last
    spec = _spec()
    rng = np.random.default_rng(7)
    packed_np = rng.permutation(n).astype(np.int64) + 1
    packed = cubed.from_array(packed_np, chunks=(c,), spec=spec)
    out = ops.unique_gather(packed, np.array(counts))
    k = sum(counts)
    want = np.concatenate([packed_np[b * c:b * c + counts[b]] for b in range(nb)])
    assert out.shape == (k,) and out.dtype == np.int64 and out.chunksize == (min(c, k),)
    # one gather op whatever nb is, and it is within allowed_mem
    gathers = [(nm, p, op) for nm, p, op in _ops(out.plan.dag)
               if any(isinstance(l, ir.Concat) for l in ir.leaves_of_program(p))]
    assert len(gathers) == 1 and len(_ops(out.plan.dag)) == 1
    (_, prog, op) = gathers[0]
    assert op.projected_mem <= op.allowed_mem and op.num_tasks == len(out.chunks[0])
    (leaf,) = [l for l in ir.leaves_of_program(prog) if isinstance(l, ir.Concat)]
    assert len(leaf.sources) == 1
    got = np.zeros(k, dtype=np.int64)
    for j, ext in enumerate(out.chunks[0]):
        block = np.zeros(ext, dtype=np.int64)
        parts = leaf.region((j,))
        total = 0
        for ai, (region,), off in parts:
            assert ai == 0 and region.step in (None, 1) and region.stop > region.start
            # a piece is the front of one source chunk's heads
            b = region.start // c
            assert (region.stop - 1) // c == b and region.stop - b * c <= counts[b]
            block[off:off + region.stop - region.start] = packed_np[region]
            total += region.stop - region.start
        assert total == ext <= out.chunksize[0]      # exactly one output chunk's worth
        got[j * out.chunksize[0]:j * out.chunksize[0] + ext] = block
    assert np.array_equal(got, want), what


def test_gather_argument_errors_and_fields():
    spec = _spec()
    p = _arr((20,), (8,), np.float32, spec)
    with pytest.raises(ValueError, match="counts"):
        ops.unique_gather(p, [1, 2])
    with pytest.raises(ValueError, match="outside"):
        ops.unique_gather(p, [1, 2, 5])       # the last chunk has 4 elements
    with pytest.raises(ValueError, match="outside"):
        ops.unique_gather(p, [9, 0, 0])
    with pytest.raises(ValueError, match="nothing"):
        ops.unique_gather(p, [0, 0, 0])
    pp = ops.unique_pack(p, False, "position")
    v, i = ops.unique_gather(pp, [2, 0, 1], "v"), ops.unique_gather(pp, [2, 0, 1], "i")
    assert v.dtype == np.float32 and i.dtype == np.int64 and v.shape == i.shape == (3,)


def test_gather_lowers_to_one_copy_of_the_pieces(udry):
    spec = _spec(udry)
    c, counts = 8, [1, 8, 0, 1, 8, 2, 0, 0, 3]
    n = len(counts) * c
    src = DeviceArray((n,), ir.sort_pairs_dtype(np.float32), (c,), name="packed-heads")
    src.allocate(udry.device)
    src.written = True
    packed = ops.from_device(src, spec)
    assert packed.name == "packed-heads" and packed.zarray is src
    assert not [d for _, d in packed.plan.dag.nodes(data=True) if d.get("pipeline") is not None]
    with pytest.raises(ValueError, match="computed"):
        ops.from_device(DeviceArray((4,), np.float32, (4,)), spec)
    for field, isz in (("v", 4), ("i", 8)):
        out = ops.unique_gather(packed, counts, field)
        udry.launched.clear()
        arrays_to_plan(out).execute(executor=udry, array_names=[out.name])
        (copy,) = udry.launched
        assert isinstance(copy, Lw.CopyLaunch) and copy.itemsize == isz
        assert sum(b.extent[-1] for b in copy.boxes) == sum(counts)
        assert len(copy.boxes) == 8                                  # six blocks, two of them cut in two
        lo, hi = src.base_addr(field), src.base_addr(field) + src.device_bytes()
        assert all(lo <= b.src < hi for b in copy.boxes)
        # the source buffer is counted among the plan's HBM-resident arrays
        assert udry._resident_bytes >= src.device_bytes()
        assert src.written and src.base_addr(field) == lo            # and was not allocated again


# ------------------------------------------------------------------ lowering of count and pack


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint64])
def test_task_tables(udry, dt):
    spec = _spec(udry)
    c, n = 1000, 4099
    nb = 5
    s = _arr((n,), (c,), dt, spec)
    sp = ops.sort(_arr((n,), (c,), dt, spec), 0, False, True, True)
    T = nat.unique_tile()
    assert T == nat.UNIQUE_TILE
    for src, pairs in ((s, False), (sp, True)):
        ys = [ops.unique_count(src, pairs), ops.unique_pack(src, pairs, "position")]
        if pairs:
            ys.append(ops.unique_pack(src, True, "index"))
        else:
            ys.append(ops.unique_pack(src, False, None))
        launches = _lower(udry, *ys)
        assert len(launches) == 3
        by_kind = {(l.kind, l.payload): l for l in launches}
        S = src.zarray
        fv = "v" if pairs else None
        for y in ys:
            prog = _ops(y.plan.dag, ir.UniqueProgram)[0][1]
            l = by_kind[(prog.kind, prog.payload)]
            assert l.ntasks == nb and l.ktype == ir.dtype_code(dt) and l.work == 1
            D = y.zarray
            for b, row in enumerate(l.rows):
                ext = S.chunk_extent((b,))[0]
                assert row["n"] == ext and row["offset"] == b * c
                assert row["src_base"] == S.chunk_addr((b,), fv)
                assert row["src_idx_base"] == (S.chunk_addr((b,), "i") if pairs else 0)
                if b == 0:
                    assert row["prev_base"] == 0 and row["n_prev"] == 0
                else:
                    assert row["prev_base"] == S.chunk_addr((b - 1,), fv) and row["n_prev"] == c
                if prog.kind == "count":
                    assert row["dst_base"] == D.chunk_addr((b,)) and row["dst_idx_base"] == 0
                elif prog.payload is None:
                    assert row["dst_base"] == D.chunk_addr((b,)) and row["dst_idx_base"] == 0
                else:
                    assert row["dst_base"] == D.chunk_addr((b,), "v")
                    assert row["dst_idx_base"] == D.chunk_addr((b,), "i")
            # every task has its own scratch for ceil(n / T) + 1 int64
            sc = np.sort(l.rows["scratch_base"])
            assert (sc > 0).all() and (sc % 8 == 0).all()
            assert (np.diff(sc) >= (-(-c // T) + 1) * 8).all()
            assert l.scratch_bytes >= nb * (-(-c // T) + 1) * 8
    # the launches were recorded, not executed
    assert all(isinstance(l, (Lw.UniqueLaunch, Lw.SortLaunch)) for l in udry.launched)


def test_work_follows_the_tile(udry):
    spec = _spec(udry)
    T = nat.unique_tile()
    for n, work in ((1, 1), (T - 1, 1), (T, 1), (T + 1, 2), (3 * T + 5, 4)):
        (l,) = _lower(udry, ops.unique_count(_arr((n,), (n,), np.float32, spec)))
        assert l.work == work and l.ntasks == 1
    (l,) = _lower(udry, ops.unique_pack(_arr((2 * T + 10,), (T + 5,), np.int64, spec)))
    assert l.work == 2 and l.ntasks == 2


def test_scratch_is_owned_by_the_plan(udry):
    import gc

    spec = _spec(udry)
    s = _arr((5000,), (1000,), np.float32, spec)
    arrays_to_plan(s).execute(executor=udry, array_names=[s.name])
    gc.collect()
    before = udry.owned_bytes()
    y = ops.unique_pack(s)
    launches = _lower(udry, y)
    assert udry.owned_bytes() >= before + sum(l.rows.nbytes + l.scratch_bytes for l in launches)
    del y, launches
    udry.launched.clear()
    udry.last_schedule = None
    gc.collect()
    assert udry.owned_bytes() == before


def test_unique_task_checks():
    V = Lw.ArrView
    f4, f8, i8 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int64)
    src = (V(1 << 20, [9], [1], f4), V(1 << 21, [9], [1], i8))
    prev = (V(1 << 22, [12], [1], f4), V(1 << 23, [12], [1], i8))
    dst = (V(1 << 24, [9], [1], f4), V(1 << 25, [9], [1], i8))
    one = (V(1 << 26, [1], [1], i8), None)
    row = Lw.unique_task(src, prev, dst, 24, "pack", "index")
    assert tuple(row.tolist()) == (1 << 20, 1 << 21, 1 << 22, 1 << 24, 1 << 25, 0, 9, 12, 24)
    row = Lw.unique_task((src[0], None), None, one, 0, "count", None)
    assert tuple(row.tolist()) == (1 << 20, 0, 0, 1 << 26, 0, 0, 9, 0, 0)
    bad = [
        ((src, prev, dst, 0, "sum", None), "kind"),
        ((src, prev, one, 0, "count", "index"), "kind"),
        (((V(1 << 20, [9], [2], f4), None), None, one, 0, "count", None), "compact"),
        (((V(1 << 20, [3, 3], [3, 1], f4), None), None, one, 0, "count", None), "1-d"),
        ((src, (V(1 << 22, [12], [1], f8), None), dst, 0, "pack", "index"), "previous chunk"),
        ((src, (V(1 << 22, [0], [1], f4), None), dst, 0, "pack", "index"), "empty previous"),
        (((src[0], V(1 << 21, [8], [1], i8)), prev, dst, 0, "pack", "index"), "index field"),
        (((src[0], None), None, dst, 0, "pack", "index"), "pairs chunk"),
        ((src, prev, (V(1 << 26, [1], [1], np.dtype(np.int32)), None), 0, "count", None), "counts into"),
        ((src, prev, (V(1 << 26, [2], [1], i8), None), 0, "count", None), "counts into"),
        ((src, prev, (V(1 << 24, [8], [1], f4), dst[1]), 0, "pack", "index"), "packs"),
        ((src, prev, (V(1 << 24, [9], [1], f8), dst[1]), 0, "pack", "index"), "packs"),
        ((src, prev, (dst[0], None), 0, "pack", "position"), "payload"),
        ((src, prev, dst, 0, "pack", None), "payload"),
        ((src, prev, (dst[0], V(1 << 25, [9], [1], f8)), 0, "pack", "position"), "index field"),
    ]
    for args, msg in bad:
        with pytest.raises(Lw.LoweringError, match=msg):
            Lw.unique_task(*args)


def test_lowering_rejects_other_shapes_of_task(udry):
    from cubed_amd.core.ops import general_blockwise

    spec = _spec(udry)
    s = _arr((40,), (16,), np.float32, spec)
    s64 = _arr((40,), (16,), np.float64, spec)
    s2d = _arr((3, 16), (1, 16), np.float32, spec)

    def build(prog, fn, *arrays, shape=(3,), dtype=np.int64, chunks=((1, 1, 1),)):
        return general_blockwise(prog, fn, *arrays, shape=shape, dtype=dtype, chunks=chunks, fusable=False)

    P = ir.UniqueProgram(kind="count", dtype=np.dtype(np.float32), nargs=2)
    own = lambda k: [(s.name, k[1])] if k[1] == 0 else [(s.name, k[1]), (s.name, k[1] - 1)]  # noqa: E731
    assert len(_lower(udry, build(P, own, s))) == 1
    cases = [
        (build(P, lambda k: [(s.name, k[1])], s), "inputs"),
        (build(P, lambda k: [(s.name, k[1]), (s.name, max(k[1] - 1, 0))], s), "inputs"),
        (build(P, lambda k: [[(s.name, 0)]] if k[1] == 0 else [(s.name, k[1]), (s.name, k[1] - 1)], s),
         "whole single chunks"),
        (build(P, lambda k: [(s.name, 0)] if k[1] == 0 else [(s.name, k[1]), (s.name, 0)], s), "the\\s+one before"),
        (build(P, lambda k: [(s64.name, 0)] if k[1] == 0 else [(s64.name, k[1]), (s64.name, k[1] - 1)], s64),
         "not a 1-d device array of float32"),
        (build(P, lambda k: [(s2d.name, 0, 0)] if k[1] == 0 else [(s2d.name, k[1], 0), (s2d.name, k[1] - 1, 0)], s2d),
         "own chunk"),
        (build(P, own, s, dtype=np.int32), "int32"),
        (build(ir.UniqueProgram(kind="pack", dtype=np.dtype(np.float32), nargs=2), own, s), "int64"),
        (build(ir.UniqueProgram(kind="count", dtype=np.dtype(np.int16), nargs=2), own, s), "not lowered"),
    ]
    for y, msg in cases:
        with pytest.raises(Lw.LoweringError, match=msg):
            _lower(udry, y)


def test_several_ranks_raise(built):
    from dryrun import FakeComm

    ex = UniqueDryExecutor(FakeComm(0, 2))
    spec = _spec(ex)
    y = ops.unique_count(_arr((40,), (8,), np.float64, spec))
    with pytest.raises(Lw.LoweringError, match="one GPU only"):
        arrays_to_plan(y).execute(executor=ex, array_names=[y.name])


# ------------------------------------------------------------------ host-side validation and the binding


def _rows(tasks):
    rows = np.zeros(len(tasks), dtype=nat.UNIQUE_TASK_DTYPE)
    for i, t in enumerate(tasks):
        rows[i]["src_base"], rows[i]["dst_base"] = t.get("src", 1 << 24), t.get("dst", 1 << 26)
        rows[i]["scratch_base"], rows[i]["n"] = t.get("scratch", 1 << 28), t["n"]
        for f in ("src_idx_base", "prev_base", "dst_idx_base", "n_prev", "offset"):
            rows[i][f] = t.get(f, 0)
    return rows


def test_unique_work(built):
    T = nat.unique_tile()
    f4, i8 = ir.dtype_code(np.float32), ir.dtype_code(np.int64)
    C, P = nat.UNIQUE_COUNT, nat.UNIQUE_PACK
    K, POS, IDX = nat.UNIQUE_KEYS, nat.UNIQUE_POSITION, nat.UNIQUE_INDEX
    assert nat.unique_work(_rows([]), f4, C, K) == 0
    assert nat.unique_work(_rows([{"n": 0}]), f4, C, K) == 0
    assert nat.unique_work(_rows([{"n": 1}, {"n": 2 * T + 1}, {"n": T}]), f4, C, K) == 3
    assert nat.unique_work(_rows([{"n": T, "dst_idx_base": 1 << 27}]), i8, P, POS) == 1
    assert nat.unique_work(_rows([{"n": T, "dst_idx_base": 1 << 27, "src_idx_base": 1 << 25}]), i8, P, IDX) == 1
    assert nat.unique_work(_rows([{"n": 5, "prev_base": 1 << 20, "n_prev": 3}]), f4, P, K) == 1
    bad = [
        (_rows([{"n": -1}]), f4, C, K, "negative"),
        (_rows([{"n": 5, "n_prev": -2}]), f4, C, K, "negative"),
        (_rows([{"n": (1 << 40) + 1}]), f4, C, K, "too large"),
        (_rows([{"n": 5, "scratch": 0}]), f4, C, K, "scratch"),
        (_rows([{"n": 5, "scratch": (1 << 28) + 4}]), f4, C, K, "scratch"),
        (_rows([{"n": 5, "dst": 0}]), f4, C, K, "destination"),
        (_rows([{"n": 5, "src": 0}]), f4, C, K, "null chunk"),
        (_rows([{"n": 5, "prev_base": 1 << 20}]), f4, C, K, "previous"),
        (_rows([{"n": 5, "src": (1 << 24) + 2}]), f4, C, K, "aligned"),
        (_rows([{"n": 5, "src": (1 << 24) + 4}]), i8, C, K, "aligned"),
        (_rows([{"n": 5, "dst": (1 << 26) + 4}]), f4, C, K, "aligned"),
        (_rows([{"n": 5}]), f4, P, POS, "payload"),
        (_rows([{"n": 5, "dst_idx_base": 1 << 27}]), f4, P, K, "payload"),
        (_rows([{"n": 5, "dst_idx_base": 1 << 27}]), f4, P, IDX, "pairs"),
        (_rows([{"n": 5, "dst": 1 << 24}]), f4, P, K, "in place"),
        (_rows([{"n": 5}]), f4, C, POS, "kind or payload"),
        (_rows([{"n": 5}]), f4, 2, K, "kind or payload"),
        (_rows([{"n": 5}]), f4, P, 3, "kind or payload"),
        (_rows([{"n": 5}]), ir.dtype_code(np.int16), C, K, "key type"),
    ]
    for rows, ktype, kind, payload, msg in bad:
        with pytest.raises(nat.NativeError, match=msg):
            nat.unique_work(rows, ktype, kind, payload)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "cubed_amd.h"
#define P(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("sizeof_unique %zu\n", sizeof(cubed_unique_task_t));
  printf("abi %d\n", CUBED_ABI_VERSION);
  printf("tile %d\n", CUBED_UNIQUE_TILE);
  printf("kinds %d\n", CUBED_UNIQUE_COUNT * 10 + CUBED_UNIQUE_PACK);
  printf("payloads %d\n", CUBED_UNIQUE_KEYS * 100 + CUBED_UNIQUE_POSITION * 10 + CUBED_UNIQUE_INDEX);
  P(cubed_unique_task_t, src_base); P(cubed_unique_task_t, src_idx_base);
  P(cubed_unique_task_t, prev_base); P(cubed_unique_task_t, dst_base);
  P(cubed_unique_task_t, dst_idx_base); P(cubed_unique_task_t, scratch_base);
  P(cubed_unique_task_t, n); P(cubed_unique_task_t, n_prev); P(cubed_unique_task_t, offset);
  return 0;
}
"""


def test_task_layout_matches_binding(built, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert c.pop("sizeof_unique") == nat.UNIQUE_TASK_DTYPE.itemsize
    assert c.pop("abi") == nat.ABI_VERSION == 19
    assert c.pop("tile") == nat.UNIQUE_TILE == nat.unique_tile()
    assert c.pop("kinds") == nat.UNIQUE_COUNT * 10 + nat.UNIQUE_PACK
    assert c.pop("payloads") == nat.UNIQUE_KEYS * 100 + nat.UNIQUE_POSITION * 10 + nat.UNIQUE_INDEX
    fields = {k.split(".")[1]: v for k, v in c.items()}
    assert set(fields) == set(nat.UNIQUE_TASK_DTYPE.names)
    for f, off in fields.items():
        assert nat.UNIQUE_TASK_DTYPE.fields[f][1] == off, f
        assert nat.UNIQUE_TASK_DTYPE.fields[f][0].itemsize == 8


def test_new_symbols_are_exported(built):
    import ctypes

    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in ("cubed_unique_tile", "cubed_unique_work", "cubed_unique_chunks"):
        assert name in nat.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
