"""take_along_axis on CPU: the API rules, the plan it builds, the task tables
it lowers to (nothing is launched), the host-side path choice and the binding.

The values themselves are checked on the GPU (tests/test_gpu_gather.py)."""

import itertools
import os
import subprocess

import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
import cubed_amd.lowering as Lw
from cubed_amd import _native as nat
from cubed_amd import ir
from cubed_amd.core.plan import arrays_to_plan
from cubed_amd.primitive.blockwise import apply_blockwise
from dryrun import DryExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class GatherDryExecutor(DryExecutor):
    """DryExecutor that also records (instead of running) gather launches."""

    def execute_dag(self, *args, **kwargs):
        saved = Lw.GatherLaunch.run
        Lw.GatherLaunch.run = lambda launch, stream, _log=self.launched: _log.append(launch)
        try:
            return super().execute_dag(*args, **kwargs)
        finally:
            Lw.GatherLaunch.run = saved


@pytest.fixture
def gdry(built):
    return GatherDryExecutor()


def _spec(ex=None, allowed_mem="2GB", reserved_mem="100MB"):
    return cubed.Spec(allowed_mem=allowed_mem, reserved_mem=reserved_mem, executor=ex)


def _arr(shape, chunks, dtype, spec):
    return cubed.from_array(np.zeros(shape, dtype=dtype), chunks=chunks, spec=spec)


def _ops(dag):
    """(name, program, primitive op) of the blockwise ops, in topological order."""
    import networkx as nx

    out = []
    for name in nx.topological_sort(dag):
        p = dag.nodes[name].get("pipeline")
        if p is not None and p.function is apply_blockwise:
            out.append((name, p.config.function, dag.nodes[name]["primitive_op"]))
    return out


def _gather_ops(dag):
    return [(n, p, op) for n, p, op in _ops(dag) if isinstance(p, ir.GatherProgram)]


def _lower(gdry, y):
    gdry.launched.clear()
    arrays_to_plan(y).execute(executor=gdry, array_names=[y.name])
    return [l for l in gdry.launched if isinstance(l, Lw.GatherLaunch)]


# ------------------------------------------------------------------ API rules

X_DTYPES = [np.bool_, np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64,
            np.float32, np.float64, "bfloat16"]
I_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64]


def test_is_exported():
    assert xp.take_along_axis is not None and "take_along_axis" in dir(xp)
    from cubed_amd.core import take_along_axis  # noqa: F401


@pytest.mark.parametrize("dt", X_DTYPES)
def test_result_dtype_shape_and_chunks(dt):
    spec = _spec()
    x = _arr((7, 13, 11), (3, 5, 4), np.float32, spec)
    if dt == "bfloat16":
        x = xp.astype(x, xp.bfloat16)
        dt = ir.bfloat16
    else:
        x = _arr((7, 13, 11), (3, 5, 4), dt, spec)
    for it in I_DTYPES:
        idx = _arr((7, 29, 11), (3, 6, 4), it, spec)
        for axis in (1, -2):
            y = xp.take_along_axis(x, idx, axis=axis)
            assert np.dtype(y.dtype) == np.dtype(dt) and y.shape == (7, 29, 11)
            assert y.chunks == ((3, 3, 1), (6, 6, 6, 6, 5), (4, 4, 3))
            progs = [p for _, p, _ in _gather_ops(y.plan.dag)]
            assert len(progs) == 3 and all(p.axis == 1 and np.dtype(p.dtype) == np.dtype(dt) for p in progs)
    # the default axis is the last one; extent 1 and a longer extent than x's
    y = xp.take_along_axis(x, _arr((7, 13, 1), (3, 5, 1), np.int64, spec))
    assert y.shape == (7, 13, 1) and y.chunks == ((3, 3, 1), (5, 5, 3), (1,))
    assert [p.axis for _, p, _ in _gather_ops(y.plan.dag)] == [2, 2, 2]
    y = xp.take_along_axis(x, _arr((30, 13, 11), (8, 5, 4), np.int64, spec), axis=0)
    assert y.shape == (30, 13, 11) and y.chunks == ((8, 8, 8, 6), (5, 5, 3), (4, 4, 3))


def test_argument_errors():
    spec = _spec()
    x = _arr((6, 8), (3, 4), np.float32, spec)
    idx = _arr((6, 5), (3, 5), np.int64, spec)
    with pytest.raises(ValueError):                      # different ndim
        xp.take_along_axis(x, _arr((5,), (5,), np.int64, spec))
    with pytest.raises(ValueError):
        xp.take_along_axis(_arr((6, 8, 1), (3, 4, 1), np.float32, spec), idx)
    with pytest.raises(ValueError):                      # 0-d
        xp.take_along_axis(xp.asarray(3.0, spec=spec), xp.asarray(0, spec=spec))
    with pytest.raises(NotImplementedError, match="broadcast"):
        xp.take_along_axis(x, _arr((1, 5), (1, 5), np.int64, spec), axis=1)
    with pytest.raises(NotImplementedError, match="broadcast"):
        xp.take_along_axis(x, idx, axis=0)
    for axis in ((0, 1), (1,), [1]):
        with pytest.raises(TypeError):
            xp.take_along_axis(x, idx, axis=axis)
    with pytest.raises(TypeError):
        xp.take_along_axis(x, idx, axis=1.0)
    with pytest.raises(Exception):                       # numpy's AxisError
        xp.take_along_axis(x, idx, axis=2)
    for bad in (np.bool_, np.float32, np.float64):
        with pytest.raises(TypeError):
            xp.take_along_axis(x, _arr((6, 5), (3, 5), bad, spec), axis=1)
    with pytest.raises(IndexError):                      # nonempty indices over an empty axis
        xp.take_along_axis(_arr((6, 0), (3, 1), np.float32, spec), idx, axis=1)


@pytest.mark.parametrize("dt", ["complex64", "complex128"])
def test_complex_is_rejected(dt):
    spec = _spec()
    x = xp.astype(_arr((6, 8), (3, 4), np.float32, spec), getattr(xp, dt))
    with pytest.raises(TypeError):
        xp.take_along_axis(x, _arr((6, 5), (3, 5), np.int64, spec), axis=1)


def test_zero_sizes_build_no_gather_op(gdry):
    spec = _spec(gdry)
    x = _arr((6, 8), (3, 4), np.float32, spec)
    e = xp.take_along_axis(x, _arr((6, 0), (3, 1), np.int64, spec), axis=1)
    assert e.shape == (6, 0) and e.dtype == np.float32 and not _gather_ops(e.plan.dag)
    got = e.compute()
    assert got.shape == (6, 0) and got.dtype == np.float32
    e = xp.take_along_axis(_arr((0, 8), (1, 4), np.int16, spec), _arr((0, 3), (1, 3), np.int64, spec), axis=1)
    assert e.shape == (0, 3) and e.dtype == np.int16 and not _gather_ops(e.plan.dag)
    # an empty axis under empty indices is fine as well
    e = xp.take_along_axis(_arr((6, 0), (3, 1), np.float32, spec), _arr((6, 0), (3, 1), np.int64, spec), axis=1)
    assert e.shape == (6, 0) and not _gather_ops(e.plan.dag)
    assert not [l for l in gdry.launched if isinstance(l, Lw.GatherLaunch)]


# ------------------------------------------------------------------ plan shape


@pytest.mark.parametrize("nb", [1, 2, 4])
@pytest.mark.parametrize("optimize_function", [None, "multiple_inputs"])
def test_nb_chained_ops_of_at_most_three_chunks(nb, optimize_function):
    from cubed_amd.core.optimization import multiple_inputs_optimize_dag

    fn = multiple_inputs_optimize_dag if optimize_function else None
    spec = _spec()
    n = 8 * (nb - 1) + 3  # a ragged last block
    x = _arr((7, n), (3, 8), np.float32, spec)
    idx = _arr((7, 10), (3, 4), np.int64, spec)
    assert x.numblocks == (3, nb)
    y = xp.take_along_axis(x + 1, idx + 1, axis=1) * 2  # elementwise producers and a consumer
    before = _gather_ops(y.plan.dag)
    after = _gather_ops(y.plan._finalize_dag(optimize_graph=True, optimize_function=fn))
    assert len(before) == len(after) == nb
    for ops in (before, after):
        prev = None
        for b, (name, prog, op) in enumerate(ops):
            assert type(prog) is ir.GatherProgram and op.fusable is False
            assert prog.nargs == (2 if b == 0 else 3) and prog.axis == 1
            assert op.num_tasks == 3 * 3 and op.target_array.dtype == np.float32
            assert op.target_array.shape == (7, 10) and op.target_array.chunks == (3, 4)
            cfg = op.pipeline.config
            for j in itertools.product(range(3), range(3)):
                keys = cfg.block_function(("out",) + j)
                assert len(keys) == prog.nargs <= 3
                assert all(isinstance(k, tuple) for k in keys)  # whole single chunks
                assert tuple(keys[0][1:]) == j                  # idx[j]
                assert tuple(keys[1][1:]) == (j[0], b)          # x[j with the axis coordinate b]
                assert cfg.reads_map[keys[0][0]].array.shape == (7, 10)
                assert cfg.reads_map[keys[1][0]].array.shape == (7, n)
                if b > 0:
                    assert keys[2] == (prev,) + j               # result_{b-1}[j]
            # the ordinary check: two copies of every argument chunk and of the output chunk
            want = 100_000_000 + 2 * (12 * 8 + 3 * min(8, n) * 4 + 12 * 4) + (2 * 12 * 4 if b else 0)
            assert op.projected_mem == want
            prev = op.target_array.name


def test_allowed_mem_of_four_chunks_passes():
    """A task holds an index chunk, a source chunk, the earlier result and
    the output: with chunks of equal bytes (float64 and int64 of one extent)
    an allowed_mem of four chunks -- counted twice each, as the projected
    memory check does -- passes, where a task that held all blocks of x could
    not."""
    chunk = 1000 * 1000 * 8
    spec = _spec(allowed_mem=2 * 4 * chunk, reserved_mem=0)
    x = xp.empty((1000, 8000), dtype=xp.float64, chunks=(1000, 1000), spec=spec)
    idx = xp.empty((1000, 8000), dtype=xp.int64, chunks=(1000, 1000), spec=spec)
    y = xp.take_along_axis(x, idx, axis=1)
    ops = _gather_ops(y.plan.dag)
    assert len(ops) == 8
    assert max(op.projected_mem for _, _, op in ops) == 2 * 4 * chunk < 2 * 5 * chunk
    with pytest.raises(ValueError, match="allowed_mem"):
        spec3 = _spec(allowed_mem=2 * 4 * chunk - 1, reserved_mem=0)
        xp.take_along_axis(xp.empty((1000, 8000), dtype=xp.float64, chunks=(1000, 1000), spec=spec3),
                           xp.empty((1000, 8000), dtype=xp.int64, chunks=(1000, 1000), spec=spec3), axis=1)


def test_indices_are_rechunked_to_x_off_the_axis():
    spec = _spec()
    x = _arr((12, 10), (4, 5), np.float32, spec)
    idx = _arr((12, 7), (6, 3), np.int64, spec)
    y = xp.take_along_axis(x, idx, axis=1)
    assert y.chunks == ((4, 4, 4), (3, 3, 1))
    names = [n for n in y.plan.dag.nodes if y.plan.dag.nodes[n].get("op_name") == "rechunk"]
    assert names
    (first, *_rest) = _gather_ops(y.plan.dag)
    cfg = first[2].pipeline.config
    keys = cfg.block_function(("out", 2, 1))
    assert cfg.reads_map[keys[0][0]].array.chunks == (4, 3)
    # the same chunks: no rechunk
    y = xp.take_along_axis(x, _arr((12, 7), (4, 3), np.int64, spec), axis=1)
    assert not [n for n in y.plan.dag.nodes if y.plan.dag.nodes[n].get("op_name") == "rechunk"]


# ------------------------------------------------------------------ lowering


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_task_tables_ragged_chunks(gdry, axis):
    spec = _spec(gdry)
    shape, chunks = (7, 13, 11), (3, 5, 4)
    x = _arr(shape, chunks, np.float32, spec)
    ishape, ichunks = list(shape), list(chunks)
    ishape[axis], ichunks[axis] = 9, 4
    idx = _arr(tuple(ishape), tuple(ichunks), np.int64, spec)
    y = xp.take_along_axis(x, idx, axis=axis)
    launches = _lower(gdry, y)
    ops = _gather_ops(y.plan.dag)
    nb = x.numblocks[axis]
    assert len(launches) == len(ops) == nb == 3
    blocks = list(itertools.product(*(range(n) for n in y.numblocks)))
    results = [op.target_array for _, _, op in ops]
    starts = np.concatenate([[0], np.cumsum(x.chunks[axis])])
    for b, launch in enumerate(launches):
        assert launch.ntasks == len(blocks) and launch.esize == 4 and launch.path == nat.GATHER_DIRECT
        most = max(int(np.prod([y.chunks[d][blk[d]] for d in range(3)])) for blk in blocks)
        assert launch.work == -(-most // nat.GATHER_ELEMS) == 1
        for row, blk in zip(launch.rows, blocks):
            ext = [y.chunks[d][blk[d]] for d in range(3)]
            assert row["outer"] == int(np.prod(ext[:axis])), blk
            assert row["inner"] == int(np.prod(ext[axis + 1:])), blk
            assert row["n_idx"] == ext[axis] and row["n_src"] == x.chunks[axis][b]
            assert row["lo"] == starts[b] and row["n_total"] == shape[axis]
            assert row["dst_base"] == results[b].chunk_addr(blk)
            assert row["prev_base"] == (results[b - 1].chunk_addr(blk) if b else 0)
            assert row["idx_base"] != 0 and row["src_base"] != 0
        assert launch.rows["idx_base"].tolist() == launches[0].rows["idx_base"].tolist()
        assert len(set(launch.rows["idx_base"].tolist())) == len(blocks)
    # op b reads block b of x: the tasks off the axis agree, the blocks differ
    srcs = [set(l.rows["src_base"].tolist()) for l in launches]
    assert all(len(s) == len(blocks) // y.numblocks[axis] for s in srcs)
    assert not (srcs[0] & srcs[1]) and not (srcs[1] & srcs[2])


def test_lds_form_work(gdry):
    spec = _spec(gdry)
    tile = nat.gather_tile_bytes()
    n = tile // 4
    x = _arr((3, n), (3, n), np.float32, spec)
    e = nat.GATHER_LDS_ELEMS
    (launch,) = _lower(gdry, xp.take_along_axis(x, _arr((3, 2 * e + 1), (3, 2 * e + 1), np.int64, spec)))
    assert launch.path == nat.GATHER_LDS and launch.work == 3 * 3
    (launch,) = _lower(gdry, xp.take_along_axis(x, _arr((3, n - 1), (3, n - 1), np.int64, spec)))
    assert launch.path == nat.GATHER_DIRECT and launch.work == -(-3 * (n - 1) // nat.GATHER_ELEMS)
    # forcing the direct form on a table the LDS form takes
    rows = _rows([dict(ext=(3, 2 * n, n, 1))])
    assert Lw.GatherLaunch(rows, 4, "cpu").path == nat.GATHER_LDS
    forced = Lw.GatherLaunch(rows, 4, "cpu", path=nat.GATHER_DIRECT)
    assert forced.path == nat.GATHER_DIRECT and forced.work == -(-3 * 2 * n // nat.GATHER_ELEMS)
    with pytest.raises(Lw.LoweringError):
        Lw.GatherLaunch(_rows([dict(ext=(3, 2 * n, n, 2))]), 4, "cpu", path=nat.GATHER_LDS)


def test_table_is_owned_by_the_plan(gdry):
    import gc

    spec = _spec(gdry)
    x = _arr((6, 50), (3, 16), np.float32, spec)
    idx = _arr((6, 100), (3, 30), np.int64, spec)
    for a in (x, idx):
        arrays_to_plan(a).execute(executor=gdry, array_names=[a.name])
    gc.collect()
    before = gdry.owned_bytes()
    y = xp.take_along_axis(x, idx, axis=1)
    launches = _lower(gdry, y)
    assert sum(l.rows.nbytes for l in launches) > 0
    assert gdry.owned_bytes() >= before + sum(l.rows.nbytes for l in launches)
    del y, launches
    gdry.launched.clear()
    gdry.last_schedule = None
    gc.collect()
    assert gdry.owned_bytes() == before


def test_gather_task_checks():
    V = Lw.ArrView
    f4, i8 = np.dtype(np.float32), np.dtype(np.int64)
    src = V(1 << 20, [3, 6, 5], [30, 5, 1], f4)
    idx, dst, prev = (V(a << 20, [3, 4, 5], [20, 5, 1], t) for a, t in ((2, i8), (3, f4), (4, f4)))
    row = Lw.gather_task(src, idx, dst, 1, 12, 20, prev)
    assert tuple(row.tolist()) == (1 << 20, 2 << 20, 3 << 20, 4 << 20, 3, 4, 6, 5, 12, 20)
    assert Lw.gather_task(src, idx, dst, 1, 12, 20)["prev_base"] == 0
    with pytest.raises(Lw.LoweringError, match="compact"):
        Lw.gather_task(V(1 << 20, [3, 6, 5], [40, 5, 1], f4), idx, dst, 1, 0, 6)
    with pytest.raises(Lw.LoweringError, match="compact"):
        Lw.gather_task(src, V(2 << 20, [3, 4, 5], [1, 3, 12], i8), dst, 1, 0, 6)
    with pytest.raises(Lw.LoweringError, match="compact"):
        Lw.gather_task(src, idx, V(3 << 20, [3, 4, 5], [20, 5, 2], f4), 1, 0, 6)
    with pytest.raises(Lw.LoweringError, match="compact"):
        Lw.gather_task(src, idx, dst, 1, 0, 6, V(4 << 20, [3, 4, 5], [24, 6, 1], f4))
    with pytest.raises(Lw.LoweringError, match="int64"):
        Lw.gather_task(src, V(2 << 20, [3, 4, 5], [20, 5, 1], np.dtype(np.int32)), dst, 1, 0, 6)
    with pytest.raises(Lw.LoweringError, match="index chunk"):   # extents off the axis differ
        Lw.gather_task(V(1 << 20, [2, 6, 5], [30, 5, 1], f4), idx, dst, 1, 0, 6)
    with pytest.raises(Lw.LoweringError, match="result chunk"):
        Lw.gather_task(src, idx, V(3 << 20, [3, 4, 5], [20, 5, 1], np.dtype(np.float64)), 1, 0, 6)
    with pytest.raises(Lw.LoweringError, match="result chunk"):
        Lw.gather_task(src, idx, dst, 1, 0, 6, V(4 << 20, [3, 6, 5], [30, 5, 1], f4))
    with pytest.raises(Lw.LoweringError, match="axis"):
        Lw.gather_task(src, idx, dst, 3, 0, 6)
    with pytest.raises(Lw.LoweringError, match="block"):
        Lw.gather_task(src, idx, dst, 1, 15, 20)
    with pytest.raises(Lw.LoweringError):
        Lw.gather_esize(np.complex64)


def test_several_ranks_raise(built):
    from dryrun import FakeComm

    ex = GatherDryExecutor(FakeComm(0, 2))
    spec = _spec(ex)
    y = xp.take_along_axis(_arr((40, 64), (8, 16), np.float64, spec), _arr((40, 64), (8, 64), np.int64, spec), axis=1)
    with pytest.raises(Lw.LoweringError, match="take_along_axis runs on one GPU only"):
        arrays_to_plan(y).execute(executor=ex, array_names=[y.name])


# ------------------------------------------------------------------ cubed_gather_path


def _rows(tasks):
    rows = np.zeros(len(tasks), dtype=nat.GATHER_TASK_DTYPE)
    for i, t in enumerate(tasks):
        rows[i]["src_base"], rows[i]["idx_base"] = t.get("src", 1 << 20), t.get("idx", 1 << 24)
        rows[i]["dst_base"], rows[i]["prev_base"] = t.get("dst", 1 << 28), t.get("prev", 0)
        rows[i]["outer"], rows[i]["n_idx"], rows[i]["n_src"], rows[i]["inner"] = t["ext"]
        rows[i]["lo"] = t.get("lo", 0)
        rows[i]["n_total"] = t.get("n_total", rows[i]["lo"] + rows[i]["n_src"])
    return rows


def _path(tasks, esize):
    rows = _rows(tasks)
    return nat.lib().cubed_gather_path(rows.ctypes.data, len(rows), esize)


def test_gather_path(built):
    tile = nat.gather_tile_bytes()
    D, L = nat.GATHER_DIRECT, nat.GATHER_LDS
    for es in (1, 2, 4, 8):
        n = tile // es
        assert _path([dict(ext=(3, n, n, 1))], es) == L           # the row is exactly the tile, n_idx == n_src
        assert _path([dict(ext=(3, 5 * n, n, 1))], es) == L
        assert _path([dict(ext=(3, n + 1, n + 1, 1))], es) == D   # one element past the tile
        assert _path([dict(ext=(3, n, n, 2))], es) == D           # inner == 2
        assert _path([dict(ext=(3, 1, n, 1))], es) == D           # n_idx == 1
        assert _path([dict(ext=(3, n - 1, n, 1))], es) == D       # fewer indices than the row has
        assert _path([dict(ext=(3, 1, 1, 1))], es) == L
    assert _path([dict(ext=(3, 9, 8, 1)), dict(ext=(2, 8, 8, 1), prev=1 << 29, lo=8)], 4) == L
    assert _path([dict(ext=(3, 9, 8, 1)), dict(ext=(3, 7, 8, 1))], 4) == D        # mixed
    assert _path([dict(ext=(3, 9, 8, 1)), dict(ext=(0, 1, 8, 7), idx=0, dst=0)], 4) == L   # an empty task has no say
    assert _path([], 4) == D
    assert nat.gather_path(_rows([dict(ext=(3, 9, 8, 1), lo=4, n_total=30)]), 8) == L
    # malformed tables
    assert _path([dict(ext=(3, 9, 8, 1))], 3) < 0
    assert _path([dict(ext=(3, 9, 8, 1))], 16) < 0
    for bad in ((-3, 9, 8, 1), (3, -9, 8, 1), (3, 9, -8, 1), (3, 9, 8, -1)):
        assert _path([dict(ext=bad, n_total=100)], 4) < 0
    assert _path([dict(ext=(3, 9, 8, 1), src=0)], 4) < 0
    assert _path([dict(ext=(3, 9, 8, 1), idx=0)], 4) < 0
    assert _path([dict(ext=(3, 9, 8, 1), dst=0)], 4) < 0
    assert _path([dict(ext=(3, 9, 8, 1), src=(1 << 20) + 4)], 8) < 0
    assert _path([dict(ext=(3, 9, 8, 1), src=(1 << 20) + 4)], 4) == L
    assert _path([dict(ext=(3, 9, 8, 1), idx=(1 << 24) + 4)], 4) < 0
    assert _path([dict(ext=(3, 9, 8, 1), dst=(1 << 28) + 2)], 4) < 0
    assert _path([dict(ext=(3, 9, 8, 1), prev=(1 << 29) + 2)], 4) < 0
    assert _path([dict(ext=(3, 9, 8, 1), dst=1 << 20)], 4) < 0          # in place
    assert _path([dict(ext=(3, 9, 8, 1), lo=-1, n_total=20)], 4) < 0
    assert _path([dict(ext=(3, 9, 8, 1), lo=13, n_total=20)], 4) < 0    # the block ends past the axis
    assert _path([dict(ext=(1 << 30, 1 << 30, 8, 1))], 4) < 0
    assert b"cubed_gather_path" in nat.lib().cubed_last_error()
    with pytest.raises(nat.NativeError, match="cubed_gather_path"):
        nat.gather_path(_rows([dict(ext=(3, 9, 8, 1), dst=0)]), 4)
    lib = nat.lib()
    assert lib.cubed_gather_path(None, 1, 4) < 0
    # the compute entry refuses malformed arguments before any device call
    assert lib.cubed_gather_chunks(None, 1, 4, 0, 1, None) == -1
    assert b"cubed_gather_chunks" in lib.cubed_last_error()
    assert lib.cubed_gather_chunks(1 << 20, 1, 3, 0, 1, None) == -1        # bad element size
    assert lib.cubed_gather_chunks(1 << 20, 1, 4, 2, 1, None) == -1        # unknown path
    assert lib.cubed_gather_chunks(1 << 20, 4, 4, 0, 1 << 30, None) == -1  # grid too large
    assert lib.cubed_gather_chunks(None, 0, 4, 0, 0, None) == 0


# ------------------------------------------------------------------ struct layout and binding

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "cubed_amd.h"
#define P(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("sizeof_gather %zu\n", sizeof(cubed_gather_task_t));
  printf("abi %d\n", CUBED_ABI_VERSION);
  printf("tile %d\n", CUBED_GATHER_TILE_BYTES);
  printf("elems %d\n", CUBED_GATHER_ELEMS);
  printf("lds_elems %d\n", CUBED_GATHER_LDS_ELEMS);
  printf("paths %d\n", CUBED_GATHER_DIRECT * 10 + CUBED_GATHER_LDS);
  P(cubed_gather_task_t, src_base); P(cubed_gather_task_t, idx_base);
  P(cubed_gather_task_t, dst_base); P(cubed_gather_task_t, prev_base);
  P(cubed_gather_task_t, outer); P(cubed_gather_task_t, n_idx);
  P(cubed_gather_task_t, n_src); P(cubed_gather_task_t, inner);
  P(cubed_gather_task_t, lo); P(cubed_gather_task_t, n_total);
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
    assert c.pop("sizeof_gather") == nat.GATHER_TASK_DTYPE.itemsize
    assert c.pop("abi") == nat.ABI_VERSION == 19
    tile = c.pop("tile")
    assert tile == nat.gather_tile_bytes() and 0 < tile <= 160 * 1024 // 2 and tile % 16 == 0
    assert c.pop("elems") == nat.GATHER_ELEMS
    assert c.pop("lds_elems") == nat.GATHER_LDS_ELEMS
    assert c.pop("paths") == nat.GATHER_DIRECT * 10 + nat.GATHER_LDS
    fields = {k.split(".")[1]: v for k, v in c.items()}
    assert set(fields) == set(nat.GATHER_TASK_DTYPE.names)
    for f, off in fields.items():
        assert nat.GATHER_TASK_DTYPE.fields[f][1] == off, f
        assert nat.GATHER_TASK_DTYPE.fields[f][0].itemsize == 8


def test_new_symbols_are_exported_and_load(built):
    header = open(os.path.join(ROOT, "include", "cubed_amd.h")).read()
    for name in ("cubed_gather_tile_bytes", "cubed_gather_path", "cubed_gather_chunks"):
        assert name in nat.EXPORTED_SYMBOLS and name + "(" in header
        assert getattr(nat.lib(), name) is not None
