"""histogram on CPU: the API rules, the plan it builds, the task tables it
lowers to (nothing is launched), the host-side path and share choice and the
binding.

The counts themselves are checked on the GPU (tests/test_gpu_hist.py)."""

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


class HistDryExecutor(DryExecutor):
    """DryExecutor that also records (instead of running) histogram launches."""

    def execute_dag(self, *args, **kwargs):
        saved = Lw.HistLaunch.run
        Lw.HistLaunch.run = lambda launch, stream, _log=self.launched: _log.append(launch)
        try:
            return super().execute_dag(*args, **kwargs)
        finally:
            Lw.HistLaunch.run = saved


@pytest.fixture
def hdry(built):
    return HistDryExecutor()


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


def _hist_ops(dag):
    return [(n, p, op) for n, p, op in _ops(dag) if isinstance(p, ir.HistogramProgram)]


def _lower(hdry, y):
    hdry.launched.clear()
    arrays_to_plan(y).execute(executor=hdry, array_names=[y.name])
    return [l for l in hdry.launched if isinstance(l, Lw.HistLaunch)]


# ------------------------------------------------------------------ API rules


def test_is_exported():
    assert xp.histogram is not None and "histogram" in dir(xp)


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.int32, np.uint8, np.bool_])
def test_result_and_edges_follow_numpy(dt):
    spec = _spec()
    like = np.empty(0, np.uint8 if dt is np.bool_ else dt)
    for shape, chunks in (((), ()), ((11,), (4,)), ((37, 5, 46), (10, 2, 16))):
        x = _arr(shape, chunks, dt, spec)
        for bins, rng in ((1, (0, 1)), (10, (-2.5, 7)), (7, (3, 3)), ([0, 0.5, 0.5, 4], None),
                          (np.array([1, 2, 5, 9]), (100, 200)), (np.array([0.25, 1.5], np.float32), None)):
            hist, edges = xp.histogram(x, bins, range=rng)
            want = np.histogram_bin_edges(like, bins, rng)
            nbins = len(want) - 1
            assert hist.dtype == np.int64 and hist.shape == (nbins,) and hist.numblocks == (1,)
            assert edges.shape == (nbins + 1,) and edges.numblocks == (1,)
            assert edges.dtype == want.dtype
            (src,) = [d["pipeline"].config.source.array for _, d in edges.plan.dag.nodes(data=True)
                      if d.get("pipeline") is not None]
            assert src.dtype == want.dtype and np.array_equal(src, want)
            (op,) = _hist_ops(hist.plan.dag)
            key = np.float32 if dt is np.float32 and want.dtype == np.float32 else np.float64
            assert op[1].dtype == np.dtype(key) and op[1].nbins == nbins and op[1].nargs == 2
            assert op[1].uniform == (np.ndim(bins) == 0)
    # the dtype numpy gives: float32 edges for float32 x, float64 otherwise
    assert np.histogram_bin_edges(like, 4, (0, 1)).dtype == (np.float32 if dt is np.float32 else np.float64)


def test_density_is_float64():
    spec = _spec()
    hist, edges = xp.histogram(_arr((30, 4), (8, 4), np.float32, spec), 6, range=(0, 3), density=True)
    assert hist.dtype == np.float64 and hist.shape == (6,) and hist.numblocks == (1,)
    assert edges.dtype == np.float32 and len(_hist_ops(hist.plan.dag)) == 1


def test_argument_errors():
    spec = _spec()
    x = _arr((20,), (8,), np.float32, spec)
    with pytest.raises(ValueError, match="range"):
        xp.histogram(x, 10)                                   # an int bins needs a range: x is lazy
    with pytest.raises(NotImplementedError, match="weights"):
        xp.histogram(x, 10, range=(0, 1), weights=x)
    with pytest.raises(TypeError, match="compute"):
        xp.histogram(x, _arr((5,), (5,), np.float32, spec))   # an Array as bins
    # numpy's own errors pass through
    for bins, rng in ((0, (0, 1)), (-3, (0, 1)), ([3, 2, 1], None), ([0, 2, 1], None), (4, (2, 1)),
                      (4, (0, np.inf)), (4, (np.nan, 1)), ([[0, 1], [2, 3]], None)):
        with pytest.raises(ValueError):
            xp.histogram(x, bins, range=rng)
        with pytest.raises(ValueError):
            np.histogram(np.zeros(3, np.float32), bins, range=rng)
    # explicit edges ignore range, as numpy does
    hist, edges = xp.histogram(x, [0, 1, 2], range=(5, 1))
    assert hist.shape == (2,)


@pytest.mark.parametrize("dt", ["bfloat16", "complex64", "complex128"])
def test_rejected_input_dtypes(dt):
    spec = _spec()
    bad = xp.astype(_arr((6,), (2,), np.float32, spec), getattr(xp, dt))
    with pytest.raises(TypeError):
        xp.histogram(bad, 4, range=(0, 1))
    with pytest.raises(TypeError):
        xp.histogram(bad, [0, 1, 2])


def test_zero_size_builds_no_histogram_op(hdry):
    spec = _spec(hdry)
    hist, edges = xp.histogram(_arr((3, 0), (1, 1), np.float32, spec), 5, range=(0, 1))
    assert hist.shape == (5,) and hist.dtype == np.int64 and not _hist_ops(hist.plan.dag)
    assert hist.compute().tolist() == [0] * 5
    assert not [l for l in hdry.launched if isinstance(l, Lw.HistLaunch)]
    dens, _ = xp.histogram(_arr((0,), (1,), np.float64, spec), [0, 1, 3], density=True)
    assert dens.dtype == np.float64 and not _hist_ops(dens.plan.dag)


# ------------------------------------------------------------------ plan shape


@pytest.mark.parametrize("optimize_function", [None, "multiple_inputs"])
def test_one_histogram_op_then_the_sum(optimize_function):
    import networkx as nx

    from cubed_amd.core.optimization import multiple_inputs_optimize_dag

    fn = multiple_inputs_optimize_dag if optimize_function else None
    spec = _spec()
    u = _arr((300, 700), (128, 256), np.float32, spec)
    v = _arr((300, 700), (128, 256), np.float32, spec)
    nbins = 12
    hist, edges = xp.histogram(u * v, nbins, range=(0, 1))   # a lazy producer
    hist = hist * 2                                          # and a consumer
    before = hist.plan.dag
    after = hist.plan._finalize_dag(optimize_graph=True, optimize_function=fn)
    for dag in (before, after):
        ((name, prog, op),) = _hist_ops(dag)
        assert type(prog) is ir.HistogramProgram and op.fusable is False
        assert prog.nbins == nbins and prog.uniform is True and prog.dtype == np.float32 and prog.nargs == 2
        assert op.num_tasks == 3 * 3 and op.target_array.dtype == np.int64
        assert op.target_array.shape == (3, 3, nbins) and op.target_array.chunks == (1, 1, nbins)
        cfg = op.pipeline.config
        for j in itertools.product(range(3), range(3)):
            keys = cfg.block_function(("out",) + j + (0,))
            assert len(keys) == 2 and all(isinstance(k, tuple) for k in keys)  # whole single chunks
            assert tuple(keys[0][1:]) == j and tuple(keys[1][1:]) == (0,)
            # the product u * v is materialised, not fused in: the op reads an array of x's shape
            assert cfg.reads_map[keys[0][0]].array.shape == (300, 700)
            assert cfg.reads_map[keys[0][0]].array.dtype == np.float32
            assert cfg.reads_map[keys[1][0]].array.shape == (nbins + 1,)
        # the ordinary check: two copies of every argument chunk and of the output chunk
        assert op.projected_mem == 100_000_000 + 2 * (128 * 256 * 4 + (nbins + 1) * 4 + nbins * 8)
        # the product is an op of its own before the histogram, the sum ops come after it
        order = [n for n, _, _ in _ops(dag)]
        producers = [n for n in nx.ancestors(dag, name) if n in order]
        sums = [n for n in nx.descendants(dag, name) if n in order]
        assert any(isinstance(dag.nodes[n]["pipeline"].config.function, ir.ExprProgram) for n in producers)
        assert any(getattr(dag.nodes[n]["pipeline"].config.function, "reduce", None) is not None for n in sums)
        assert all(order.index(n) > order.index(name) for n in sums)


def test_non_float_input_is_converted_first():
    spec = _spec()
    hist, _ = xp.histogram(_arr((40,), (16,), np.int32, spec), 4, range=(0, 9))
    ((name, prog, op),) = _hist_ops(hist.plan.dag)
    assert prog.dtype == np.float64
    x_name = op.pipeline.config.block_function(("out", 1, 0))[0][0]
    assert op.pipeline.config.reads_map[x_name].array.dtype == np.float64


def test_too_many_bins_for_allowed_mem():
    spec = _spec(allowed_mem="200MB", reserved_mem=0)
    x = xp.empty((1000,), dtype=xp.float64, chunks=(100,), spec=spec)
    xp.histogram(x, 1_000_000, range=(0, 1))
    with pytest.raises(ValueError, match="allowed_mem"):
        xp.histogram(x, 20_000_000, range=(0, 1))
    with pytest.raises(ValueError, match="allowed_mem"):
        xp.histogram(xp.empty((4, 30_000_000), dtype=xp.float64, chunks=(1, 30_000_000), spec=spec), 10, range=(0, 1))


# ------------------------------------------------------------------ lowering


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.int16])
def test_task_tables_edge_chunks(hdry, dt):
    spec = _spec(hdry)
    x = _arr((37, 5, 46), (10, 2, 16), dt, spec)
    nbins = 9
    hist, edges = xp.histogram(x, nbins, range=(0, 1))
    (launch,) = _lower(hdry, hist)
    ((_, prog, op),) = _hist_ops(hist.plan.dag)
    blocks = list(itertools.product(range(4), range(3), range(3)))
    key = np.float32 if dt is np.float32 else np.float64
    assert launch.ntasks == len(blocks) and launch.nbins == nbins and launch.uniform is True
    assert launch.ktype == ir.dtype_code(key) and launch.path == nat.HIST_UNIFORM
    assert launch.work == 1
    assert len(set(launch.rows["edges_base"].tolist())) == 1        # the one chunk of the edges
    assert len(set(launch.rows["x_base"].tolist())) == len(blocks)
    for row, blk in zip(launch.rows, blocks):
        ext = [x.chunks[d][blk[d]] for d in range(3)]
        assert row["n_values"] == ext[0] * ext[1] * ext[2], blk
        assert row["dst_base"] == op.target_array.chunk_addr(blk + (0,))
        assert row["x_base"] != 0 and row["edges_base"] != 0
    # the rows of the partials do not overlap
    dst = np.sort(launch.rows["dst_base"])
    assert (np.diff(dst) >= nbins * 8).all()
    # explicit edges take the search path
    hist, _ = xp.histogram(x, np.linspace(0, 1, nbins + 1), range=(0, 1))
    (launch,) = _lower(hdry, hist)
    assert launch.path == nat.HIST_SEARCH and launch.uniform is False and launch.ktype == ir.dtype_code(np.float64)


def test_paths_at_the_lds_limit(hdry):
    spec = _spec(hdry)
    L = nat.hist_bins_lds()
    x = _arr((1000,), (400,), np.float32, spec)
    for nbins, int_path, edges_path in ((L - 1, nat.HIST_UNIFORM, nat.HIST_SEARCH), (L, nat.HIST_UNIFORM, nat.HIST_SEARCH),
                                        (L + 1, nat.HIST_WIDE, nat.HIST_WIDE)):
        (launch,) = _lower(hdry, xp.histogram(x, nbins, range=(0, 1))[0])
        assert launch.path == int_path and launch.nbins == nbins
        (launch,) = _lower(hdry, xp.histogram(x, np.linspace(0, 1, nbins + 1, dtype=np.float32))[0])
        assert launch.path == edges_path and launch.nbins == nbins


def test_table_is_owned_by_the_plan(hdry):
    import gc

    spec = _spec(hdry)
    x = _arr((100,), (30,), np.float32, spec)
    arrays_to_plan(x).execute(executor=hdry, array_names=[x.name])
    gc.collect()
    before = hdry.owned_bytes()
    hist, _ = xp.histogram(x, 5, range=(0, 1))
    launches = _lower(hdry, hist)
    assert hdry.owned_bytes() >= before + sum(l.rows.nbytes for l in launches)
    del hist, launches, _
    hdry.launched.clear()
    hdry.last_schedule = None
    gc.collect()
    assert hdry.owned_bytes() == before


def test_hist_task_checks():
    V = Lw.ArrView
    f4, f8, i8 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int64)
    x, e, d = V(1 << 21, [3, 5], [5, 1], f4), V(1 << 20, [8], [1], f4), V(1 << 22, [1, 1, 7], [7, 7, 1], i8)
    assert tuple(Lw.hist_task(x, e, d, 7).tolist()) == (1 << 21, 1 << 20, 1 << 22, 15)
    assert Lw.hist_task(V(1 << 21, [], [], f4), e, V(1 << 22, [7], [1], i8), 7)["n_values"] == 1
    with pytest.raises(Lw.LoweringError, match="compact"):
        Lw.hist_task(V(1 << 21, [3, 5], [8, 1], f4), e, d, 7)
    with pytest.raises(Lw.LoweringError, match="compact"):
        Lw.hist_task(x, V(1 << 20, [8], [2], f4), d, 7)
    with pytest.raises(Lw.LoweringError, match="edges"):
        Lw.hist_task(x, V(1 << 20, [7], [1], f4), d, 7)
    with pytest.raises(Lw.LoweringError, match="edges"):
        Lw.hist_task(x, V(1 << 20, [8], [1], f8), d, 7)
    with pytest.raises(Lw.LoweringError, match="counts"):
        Lw.hist_task(x, e, V(1 << 22, [1, 1, 7], [7, 7, 1], np.dtype(np.int32)), 7)
    with pytest.raises(Lw.LoweringError, match="counts"):
        Lw.hist_task(x, e, V(1 << 22, [1, 2, 7], [14, 7, 1], i8), 7)
    with pytest.raises(Lw.LoweringError, match="counts"):
        Lw.hist_task(x, e, V(1 << 22, [1, 1, 6], [6, 6, 1], i8), 7)


def test_lowering_rejects_other_shapes_of_task(hdry):
    """_lower_hist: whole single chunks, the single edges chunk, the dtypes
    and the extent of the target."""
    from cubed_amd.core.ops import general_blockwise

    spec = _spec(hdry)
    x = _arr((40,), (16,), np.float32, spec)
    e = cubed.from_array(np.linspace(0, 1, 5, dtype=np.float32), chunks=(5,), spec=spec)
    e2 = cubed.from_array(np.linspace(0, 1, 10, dtype=np.float32), chunks=(5,), spec=spec)
    e64 = cubed.from_array(np.linspace(0, 1, 5), chunks=(5,), spec=spec)

    def build(prog, fn, *arrays, shape=(3, 4), dtype=np.int64, chunks=((1, 1, 1), (4,))):
        return general_blockwise(prog, fn, *arrays, shape=shape, dtype=dtype, chunks=chunks, fusable=False)

    P = ir.HistogramProgram(nbins=4, uniform=True, dtype=np.dtype(np.float32), nargs=2)
    good = build(P, lambda k: [(x.name, k[1]), (e.name, 0)], x, e)
    assert len(_lower(hdry, good)) == 1
    cases = [
        (build(P, lambda k: [[(x.name, k[1])], (e.name, 0)], x, e), "whole single chunks"),
        (build(P, lambda k: [(x.name, k[1]), (e2.name, 1)], x, e2), "single chunk of its edges"),
        (build(P, lambda k: [(x.name, k[1])], x), "inputs"),
        (build(P, lambda k: [(x.name, k[1]), (e64.name, 0)], x, e64), "not a device array of float32"),
        (build(P, lambda k: [(x.name, k[1]), (e.name, 0)], x, e, dtype=np.int32), "int32"),
        (build(P, lambda k: [(x.name, k[1]), (e.name, 0)], x, e, shape=(3, 8), chunks=((1, 1, 1), (8,))), "counts chunk"),
        (build(ir.HistogramProgram(nbins=4, uniform=True, dtype=np.dtype(np.int32), nargs=2),
               lambda k: [(x.name, k[1]), (e.name, 0)], x, e), "not lowered"),
    ]
    for y, msg in cases:
        with pytest.raises(Lw.LoweringError, match=msg):
            _lower(hdry, y)


def test_several_ranks_raise(built):
    from dryrun import FakeComm

    ex = HistDryExecutor(FakeComm(0, 2))
    spec = _spec(ex)
    hist, _ = xp.histogram(_arr((40, 64), (8, 64), np.float64, spec), 10, range=(0, 1))
    with pytest.raises(Lw.LoweringError, match="histogram runs on one GPU only"):
        arrays_to_plan(hist).execute(executor=ex, array_names=[hist.name])


# ------------------------------------------------------------------ a workgroup's share


def _rows(tasks):
    rows = np.zeros(len(tasks), dtype=nat.HIST_TASK_DTYPE)
    for i, t in enumerate(tasks):
        rows[i]["x_base"], rows[i]["edges_base"] = t.get("x", 1 << 24), t.get("edges", 1 << 20)
        rows[i]["dst_base"], rows[i]["n_values"] = t.get("dst", 1 << 28), t["n"]
    return rows


def _share(n, work):
    """What the kernel gives a workgroup: ceil(n / work) rounded up to 1024 values."""
    return -(-(-(-n // work)) // 1024) * 1024


def test_a_share_stays_below_two_to_the_32():
    for path in (nat.HIST_UNIFORM, nat.HIST_SEARCH, nat.HIST_WIDE):
        for nbins in (1, 4096, 1 << 20):
            rows = _rows([dict(n=2 ** 40), dict(n=5)])
            work = Lw.hist_work(rows, nbins, path)
            assert work >= 1 and work * len(rows) <= 2 ** 31 - 1
            assert _share(2 ** 40, work) < 2 ** 32
            # small tables: one workgroup per task until the share passes its least size
            assert Lw.hist_work(_rows([dict(n=nat.HIST_VALUES)]), 10, path) == 1
            assert Lw.hist_work(_rows([dict(n=nat.HIST_VALUES + 1)]), 10, path) == 2
            assert Lw.hist_work(_rows([dict(n=0)]), 10, path) == 0
    # staging and flushing nbins counters is paid for by eight values per bin
    assert Lw.hist_work(_rows([dict(n=8 * 4096 + 1)]), 4096, nat.HIST_SEARCH) == 2
    assert Lw.hist_work(_rows([dict(n=8 * 4096)]), 4096, nat.HIST_UNIFORM) == 1
    assert Lw.hist_work(_rows([dict(n=8 * 4096)]), 4097, nat.HIST_WIDE) == 2
    # about HIST_GROUPS workgroups over a large table
    rows = _rows([dict(n=1 << 22)] * 64)
    assert Lw.hist_work(rows, 100, nat.HIST_UNIFORM) * 64 == Lw.HIST_GROUPS
    assert Lw.HIST_SHARE_MAX + 1024 < 2 ** 32


def test_share_bound_raises_when_a_launch_cannot_hold_it(monkeypatch):
    rows = _rows([dict(n=2 ** 40)] * 3)
    monkeypatch.setattr(Lw, "HIST_SHARE_MAX", 1 << 20)   # a narrower counter: 2^20 workgroups per task
    assert Lw.hist_work(rows, 10, nat.HIST_UNIFORM) == 2 ** 20
    monkeypatch.setattr(Lw, "HIST_MAX_GROUPS", 3 * 2 ** 20 - 1)
    with pytest.raises(Lw.LoweringError, match="workgroups"):
        Lw.hist_work(rows, 10, nat.HIST_UNIFORM)


# ------------------------------------------------------------------ cubed_hist_path


def _path(tasks, ktype, nbins, uniform):
    rows = _rows(tasks)
    return nat.lib().cubed_hist_path(rows.ctypes.data, len(rows), ktype, nbins, uniform)


def test_hist_path(built):
    L = nat.hist_bins_lds()
    # edges and counters of two workgroups fit a CU's 160 KiB of LDS with f64 edges
    assert L >= 4096 and 2 * ((L + 1) * 8 + 8 + L * 4) <= 160 * 1024
    F32, F64 = ir.dtype_code(np.float32), ir.dtype_code(np.float64)
    for kt in (F32, F64):
        for nbins in (1, L - 1, L):
            assert _path([dict(n=10)], kt, nbins, 1) == nat.HIST_UNIFORM
            assert _path([dict(n=10)], kt, nbins, 0) == nat.HIST_SEARCH
        for nbins in (L + 1, 3 * L + 5, 100000):
            assert _path([dict(n=10)], kt, nbins, 1) == nat.HIST_WIDE
            assert _path([dict(n=10)], kt, nbins, 0) == nat.HIST_WIDE
    assert _path([], F32, 10, 1) == nat.HIST_UNIFORM
    assert _path([dict(n=0, x=0)], F32, 10, 0) == nat.HIST_SEARCH
    assert nat.hist_path(_rows([dict(n=3)]), F64, L + 1, True) == nat.HIST_WIDE
    # malformed tables
    for kt in (np.int32, np.int64, np.uint64, np.int8):
        assert _path([dict(n=10)], ir.dtype_code(kt), 10, 1) < 0
    assert _path([dict(n=10)], 99, 10, 1) < 0
    assert _path([dict(n=10)], F32, 0, 1) < 0
    assert _path([dict(n=10)], F32, -1, 1) < 0
    assert _path([dict(n=10)], F32, (1 << 30) + 1, 1) < 0
    assert _path([dict(n=-10)], F32, 10, 1) < 0
    assert _path([dict(n=(1 << 40) + 1)], F32, 10, 1) < 0
    assert _path([dict(n=10, x=0)], F32, 10, 1) < 0
    assert _path([dict(n=10, edges=0)], F32, 10, 1) < 0
    assert _path([dict(n=10, dst=0)], F32, 10, 1) < 0
    assert _path([dict(n=10, x=(1 << 24) + 4)], F64, 10, 1) < 0
    assert _path([dict(n=10, x=(1 << 24) + 4)], F32, 10, 1) == nat.HIST_UNIFORM
    assert _path([dict(n=10, edges=(1 << 20) + 4)], F64, 10, 1) < 0
    assert _path([dict(n=10, dst=(1 << 28) + 4)], F32, 10, 1) < 0
    assert b"cubed_hist_path" in nat.lib().cubed_last_error()
    with pytest.raises(nat.NativeError, match="cubed_hist_path"):
        nat.hist_path(_rows([dict(n=10, dst=0)]), F32, 10, True)
    lib = nat.lib()
    assert lib.cubed_hist_path(None, 1, F32, 10, 1) < 0
    # the compute entry refuses malformed arguments before any device call
    assert lib.cubed_hist_chunks(None, 1, F32, 10, 0, 1, None) == -1
    assert b"cubed_hist_chunks" in lib.cubed_last_error()
    assert lib.cubed_hist_chunks(1 << 20, 1, 99, 10, 0, 1, None) == -1            # unknown ktype
    assert lib.cubed_hist_chunks(1 << 20, 1, ir.dtype_code(np.int64), 10, 0, 1, None) == -1
    assert lib.cubed_hist_chunks(1 << 20, 1, F32, 0, 0, 1, None) == -1            # no bins
    assert lib.cubed_hist_chunks(1 << 20, 1, F32, 10, 3, 1, None) == -1           # unknown path
    assert lib.cubed_hist_chunks(1 << 20, 1, F32, L + 1, nat.HIST_UNIFORM, 1, None) == -1  # too wide for LDS
    assert lib.cubed_hist_chunks(1 << 20, 1, F32, L + 1, nat.HIST_SEARCH, 1, None) == -1
    assert lib.cubed_hist_chunks(1 << 20, 4, F32, 10, 0, 1 << 30, None) == -1     # grid too large
    assert lib.cubed_hist_chunks(1 << 20, 1, F32, 10, 0, -1, None) == -1
    assert b"cubed_hist_chunks" in lib.cubed_last_error()
    assert lib.cubed_hist_chunks(None, 0, F32, 10, 0, 0, None) == 0


# ------------------------------------------------------------------ struct layout

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "cubed_amd.h"
#define P(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("sizeof_hist %zu\n", sizeof(cubed_hist_task_t));
  printf("abi %d\n", CUBED_ABI_VERSION);
  printf("bins_lds %d\n", CUBED_HIST_BINS_LDS);
  printf("values %d\n", CUBED_HIST_VALUES);
  printf("paths %d\n", CUBED_HIST_UNIFORM * 100 + CUBED_HIST_SEARCH * 10 + CUBED_HIST_WIDE);
  P(cubed_hist_task_t, x_base); P(cubed_hist_task_t, edges_base);
  P(cubed_hist_task_t, dst_base); P(cubed_hist_task_t, n_values);
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
    assert c.pop("sizeof_hist") == nat.HIST_TASK_DTYPE.itemsize
    assert c.pop("abi") == nat.ABI_VERSION == 19
    assert c.pop("bins_lds") == nat.hist_bins_lds()
    assert c.pop("values") == nat.HIST_VALUES
    assert c.pop("paths") == nat.HIST_UNIFORM * 100 + nat.HIST_SEARCH * 10 + nat.HIST_WIDE
    fields = {k.split(".")[1]: v for k, v in c.items()}
    assert set(fields) == set(nat.HIST_TASK_DTYPE.names)
    for f, off in fields.items():
        assert nat.HIST_TASK_DTYPE.fields[f][1] == off, f
        assert nat.HIST_TASK_DTYPE.fields[f][0].itemsize == 8


def test_new_symbols_are_exported():
    for name in ("cubed_hist_bins_lds", "cubed_hist_path", "cubed_hist_chunks"):
        assert name in nat.EXPORTED_SYMBOLS
