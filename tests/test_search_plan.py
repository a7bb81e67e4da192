"""searchsorted on CPU: the API rules, the plan it builds, the task tables it
lowers to (nothing is launched), the host-side path choice and the binding.

The values themselves are checked on the GPU (tests/test_gpu_search.py)."""

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


class SearchDryExecutor(DryExecutor):
    """DryExecutor that also records (instead of running) search launches."""

    def execute_dag(self, *args, **kwargs):
        saved = Lw.SearchLaunch.run
        Lw.SearchLaunch.run = lambda launch, stream, _log=self.launched: _log.append(launch)
        try:
            return super().execute_dag(*args, **kwargs)
        finally:
            Lw.SearchLaunch.run = saved


@pytest.fixture
def sdry(built):
    return SearchDryExecutor()


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


def _search_ops(dag):
    return [(n, p, op) for n, p, op in _ops(dag) if isinstance(p, ir.SearchProgram)]


def _lower(sdry, y):
    sdry.launched.clear()
    arrays_to_plan(y).execute(executor=sdry, array_names=[y.name])
    return [l for l in sdry.launched if isinstance(l, Lw.SearchLaunch)]


# ------------------------------------------------------------------ API rules

KEY = {np.bool_: np.int32, np.int8: np.int32, np.int16: np.int32, np.int32: np.int32, np.int64: np.int64,
       np.uint8: np.uint32, np.uint16: np.uint32, np.uint32: np.uint32, np.uint64: np.uint64,
       np.float32: np.float32, np.float64: np.float64}


def test_is_exported():
    assert xp.searchsorted is not None and "searchsorted" in dir(xp)


@pytest.mark.parametrize("dt", list(KEY))
def test_result_dtype_shape_and_chunks(dt):
    spec = _spec()
    x1 = _arr((20,), (8,), dt, spec)
    for shape, chunks in (((), ()), ((11,), (4,)), ((37, 5, 46), (10, 2, 16))):
        x2 = _arr(shape, chunks, dt, spec)
        for side in ("left", "right"):
            y = xp.searchsorted(x1, x2, side=side)
            assert y.dtype == np.int64 and y.shape == x2.shape and y.chunks == x2.chunks
            progs = [p for _, p, _ in _search_ops(y.plan.dag)]
            assert len(progs) == 3 and all(p.dtype == np.dtype(KEY[dt]) for p in progs)
            assert all(p.right == (side == "right") for p in progs)


def test_mixed_dtypes_promote_then_widen():
    spec = _spec()
    for d1, d2, key in ((np.int8, np.int64, np.int64), (np.uint8, np.int8, np.int32),
                        (np.float32, np.float64, np.float64), (np.bool_, np.bool_, np.int32),
                        (np.uint16, np.uint32, np.uint32)):
        y = xp.searchsorted(_arr((9,), (9,), d1, spec), _arr((5,), (5,), d2, spec))
        (op,) = _search_ops(y.plan.dag)
        assert op[1].dtype == np.dtype(key) and y.dtype == np.int64


def test_argument_errors():
    spec = _spec()
    x1 = _arr((20,), (8,), np.float32, spec)
    x2 = _arr((5,), (5,), np.float32, spec)
    with pytest.raises(ValueError):
        xp.searchsorted(_arr((4, 5), (4, 5), np.float32, spec), x2)
    with pytest.raises(ValueError):
        xp.searchsorted(xp.asarray(3.0, spec=spec), xp.asarray(3.0, spec=spec))
    for side in ("middle", "Left", None, 0):
        with pytest.raises(ValueError):
            xp.searchsorted(x1, x2, side=side)
    # the namespace's own promotion errors stay
    with pytest.raises(TypeError):
        xp.searchsorted(_arr((20,), (8,), np.int64, spec), _arr((5,), (5,), np.uint64, spec))
    with pytest.raises(TypeError):
        xp.searchsorted(_arr((20,), (8,), np.int32, spec), x2)
    # sorter: int64, x1's shape
    with pytest.raises(ValueError):
        xp.searchsorted(x1, x2, sorter=_arr((20,), (8,), np.int32, spec))
    with pytest.raises(ValueError):
        xp.searchsorted(x1, x2, sorter=_arr((19,), (8,), np.int64, spec))


@pytest.mark.parametrize("dt", ["bfloat16", "complex64", "complex128"])
def test_rejected_input_dtypes(dt):
    spec = _spec()
    f = _arr((6,), (2,), np.float32, spec)
    bad = xp.astype(f, getattr(xp, dt))
    with pytest.raises(TypeError):
        xp.searchsorted(bad, f)
    with pytest.raises(TypeError):
        xp.searchsorted(f, bad)
    with pytest.raises(TypeError):
        xp.searchsorted(bad, bad)


def test_zero_sizes_build_no_search_op(sdry):
    spec = _spec(sdry)
    x1 = _arr((20,), (8,), np.float32, spec)
    empty1 = _arr((0,), (1,), np.float32, spec)
    x2 = _arr((6, 4), (4, 4), np.float32, spec)
    z = xp.searchsorted(empty1, x2)          # zero-size x1: zeros
    assert z.shape == (6, 4) and z.dtype == np.int64 and z.chunks == x2.chunks
    assert not _search_ops(z.plan.dag)
    assert not _lower(sdry, z)
    e = xp.searchsorted(x1, _arr((3, 0), (1, 1), np.float32, spec), side="right")  # zero-size x2: empty
    assert e.shape == (3, 0) and e.dtype == np.int64
    assert not _search_ops(e.plan.dag)
    got = e.compute()
    assert got.shape == (3, 0) and got.dtype == np.int64
    assert not [l for l in sdry.launched if isinstance(l, Lw.SearchLaunch)]


# ------------------------------------------------------------------ plan shape


@pytest.mark.parametrize("nb", [1, 2, 5])
@pytest.mark.parametrize("optimize_function", [None, "multiple_inputs"])
def test_nb_chained_ops_of_at_most_three_chunks(nb, optimize_function):
    from cubed_amd.core.optimization import multiple_inputs_optimize_dag

    fn = multiple_inputs_optimize_dag if optimize_function else None
    spec = _spec()
    n = 8 * (nb - 1) + 3  # a ragged last block
    x1 = _arr((n,), (8,), np.int32, spec)
    x2 = _arr((7, 10), (3, 4), np.int32, spec)
    assert x1.numblocks == (nb,)
    y = xp.searchsorted(x1 + 1, x2 + 1) * 2  # elementwise producers and a consumer
    before = _search_ops(y.plan.dag)
    after = _search_ops(y.plan._finalize_dag(optimize_graph=True, optimize_function=fn))
    assert len(before) == len(after) == nb
    for ops in (before, after):
        prev = None
        for b, (name, prog, op) in enumerate(ops):
            assert type(prog) is ir.SearchProgram and op.fusable is False
            assert prog.nargs == (2 if b == 0 else 3) and prog.right is False
            assert op.num_tasks == 3 * 3 and op.target_array.dtype == np.int64
            assert op.target_array.shape == (7, 10) and op.target_array.chunks == (3, 4)
            cfg = op.pipeline.config
            for j in itertools.product(range(3), range(3)):
                keys = cfg.block_function(("out",) + j)
                assert len(keys) == prog.nargs <= 3
                assert all(isinstance(k, tuple) for k in keys)  # whole single chunks
                assert tuple(keys[0][1:]) == j                  # x2[j]
                assert tuple(keys[1][1:]) == (b,)               # x1[b]
                assert cfg.reads_map[keys[0][0]].array.shape == (7, 10)
                assert cfg.reads_map[keys[1][0]].array.shape == (n,)
                if b > 0:
                    assert keys[2] == (prev,) + j               # counts_{b-1}[j]
            # the ordinary check: two copies of every argument chunk and of the output chunk
            want = 100_000_000 + 2 * (12 * 4 + min(8, n) * 4 + 12 * 8) + (2 * 12 * 8 if b else 0)
            assert op.projected_mem == want
            prev = op.target_array.name


def test_chunks_too_large_for_allowed_mem():
    spec = _spec(allowed_mem="200MB", reserved_mem=0)
    x1 = xp.empty((1000,), dtype=xp.float64, chunks=(1000,), spec=spec)
    x2 = xp.empty((4, 20_000_000), dtype=xp.float64, chunks=(1, 20_000_000), spec=spec)
    with pytest.raises(ValueError, match="allowed_mem"):
        xp.searchsorted(x1, x2)
    big1 = xp.empty((40_000_000,), dtype=xp.float64, chunks=(20_000_000,), spec=spec)
    with pytest.raises(ValueError, match="allowed_mem"):
        xp.searchsorted(big1, xp.empty((10,), dtype=xp.float64, chunks=(10,), spec=spec))


# ------------------------------------------------------------------ lowering


@pytest.mark.parametrize("right", [False, True])
def test_task_tables_edge_chunks(sdry, right):
    spec = _spec(sdry)
    x1 = _arr((50,), (16,), np.int32, spec)                 # blocks of 16, 16, 16, 2
    x2 = _arr((37, 5, 46), (10, 2, 16), np.int32, spec)
    y = xp.searchsorted(x1, x2, side="right" if right else "left")
    launches = _lower(sdry, y)
    ops = _search_ops(y.plan.dag)
    assert len(launches) == len(ops) == 4
    blocks = list(itertools.product(range(4), range(3), range(3)))
    counts = [op.target_array for _, _, op in ops]
    sorted_addrs = set()
    for b, launch in enumerate(launches):
        assert launch.ntasks == len(blocks) and launch.right == right
        assert launch.flags == (nat.SEARCH_RIGHT if right else 0)
        assert launch.ktype == ir.dtype_code(np.int32) and launch.path == nat.SEARCH_LDS
        # the value the header defines: ceil(most n_values / CUBED_SEARCH_VALUES)
        assert launch.work == -(-(10 * 2 * 16) // nat.SEARCH_VALUES) == 1
        assert len(set(launch.rows["sorted_base"].tolist())) == 1  # the one chunk b of x1
        sorted_addrs.add(int(launch.rows["sorted_base"][0]))
        for row, blk in zip(launch.rows, blocks):
            ext = [x2.chunks[d][blk[d]] for d in range(3)]
            assert row["n_values"] == ext[0] * ext[1] * ext[2], blk
            assert row["n_sorted"] == x1.chunks[0][b]
            assert row["dst_base"] == counts[b].chunk_addr(blk)
            assert row["acc_base"] == (counts[b - 1].chunk_addr(blk) if b else 0)
            assert row["values_base"] != 0 and row["sorted_base"] != 0
        # the values chunks are the same in every op
        assert launch.rows["values_base"].tolist() == launches[0].rows["values_base"].tolist()
        assert len(set(launch.rows["values_base"].tolist())) == len(blocks)
    assert len(sorted_addrs) == 4


def test_zero_d_values_and_work(sdry):
    spec = _spec(sdry)
    tile = nat.search_tile()
    x1 = _arr((tile + 1,), (tile + 1,), np.float64, spec)
    (launch,) = _lower(sdry, xp.searchsorted(x1, xp.asarray(3.0, spec=spec)))
    assert launch.ntasks == 1 and launch.work == 1 and launch.path == nat.SEARCH_SPLIT
    assert launch.rows[0]["n_values"] == 1 and launch.rows[0]["n_sorted"] == tile + 1
    v = nat.SEARCH_VALUES
    x2 = _arr((2 * v + 1,), (2 * v + 1,), np.float64, spec)
    (launch,) = _lower(sdry, xp.searchsorted(x1, x2))
    assert launch.work == 3 and launch.rows[0]["n_values"] == 2 * v + 1


def test_table_is_owned_by_the_plan(sdry):
    import gc

    spec = _spec(sdry)
    x1 = _arr((50,), (16,), np.float32, spec)
    x2 = _arr((100,), (30,), np.float32, spec)
    for x in (x1, x2):
        arrays_to_plan(x).execute(executor=sdry, array_names=[x.name])
    gc.collect()
    before = sdry.owned_bytes()
    y = xp.searchsorted(x1, x2)
    launches = _lower(sdry, y)
    assert sdry.owned_bytes() >= before + sum(l.rows.nbytes for l in launches)
    del y, launches
    sdry.launched.clear()
    sdry.last_schedule = None
    gc.collect()
    assert sdry.owned_bytes() == before


def test_search_task_checks():
    V = Lw.ArrView
    f4, i8 = np.dtype(np.float32), np.dtype(np.int64)
    s = V(1 << 20, [40], [1], f4)
    vals, dst, acc = V(1 << 21, [3, 5], [5, 1], f4), V(1 << 22, [3, 5], [5, 1], i8), V(1 << 23, [3, 5], [5, 1], i8)
    row = Lw.search_task(s, vals, dst, acc)
    assert tuple(row.tolist()) == (1 << 20, 1 << 21, 1 << 23, 1 << 22, 40, 15)
    assert Lw.search_task(s, vals, dst)["acc_base"] == 0
    with pytest.raises(Lw.LoweringError, match="compact"):
        Lw.search_task(s, V(1 << 21, [3, 5], [8, 1], f4), dst)
    with pytest.raises(Lw.LoweringError, match="compact"):
        Lw.search_task(s, V(1 << 21, [3, 5], [1, 3], f4), dst)
    with pytest.raises(Lw.LoweringError, match="compact"):
        Lw.search_task(V(1 << 20, [40], [2], f4), vals, dst)
    with pytest.raises(Lw.LoweringError, match="1-d"):
        Lw.search_task(V(1 << 20, [4, 10], [10, 1], f4), vals, dst)
    with pytest.raises(Lw.LoweringError, match="counts"):
        Lw.search_task(s, vals, V(1 << 22, [3, 5], [5, 1], np.dtype(np.int32)))
    with pytest.raises(Lw.LoweringError, match="counts"):
        Lw.search_task(s, vals, dst, V(1 << 23, [15], [1], i8))
    with pytest.raises(Lw.LoweringError, match="counts"):
        Lw.search_task(s, vals, dst, V(1 << 23, [3, 5], [5, 1], f4))
    with pytest.raises(Lw.LoweringError):
        Lw.search_task(V(1 << 20, [40], [1], np.dtype(np.float64)), vals, dst)


def test_several_ranks_raise(built):
    from dryrun import FakeComm

    ex = SearchDryExecutor(FakeComm(0, 2))
    spec = _spec(ex)
    y = xp.searchsorted(_arr((50,), (16,), np.float64, spec), _arr((40, 64), (8, 64), np.float64, spec))
    with pytest.raises(Lw.LoweringError, match="searchsorted runs on one GPU only"):
        arrays_to_plan(y).execute(executor=ex, array_names=[y.name])


# ------------------------------------------------------------------ cubed_search_path


def _rows(tasks):
    rows = np.zeros(len(tasks), dtype=nat.SEARCH_TASK_DTYPE)
    for i, t in enumerate(tasks):
        rows[i]["sorted_base"], rows[i]["values_base"] = t.get("sorted", 1 << 20), t.get("values", 1 << 24)
        rows[i]["acc_base"], rows[i]["dst_base"] = t.get("acc", 0), t.get("dst", 1 << 28)
        rows[i]["n_sorted"], rows[i]["n_values"] = t["n"]
    return rows


def _path(tasks, ktype):
    rows = _rows(tasks)
    return nat.lib().cubed_search_path(rows.ctypes.data, len(rows), ktype)


def test_search_path(built):
    tile = nat.search_tile()
    # at most 64 KiB of LDS at 8-byte keys, so two workgroups fit a CU
    assert tile == 4096 and tile & (tile - 1) == 0 and tile * 8 <= 64 * 1024
    F32, F64, I64 = (ir.dtype_code(t) for t in (np.float32, np.float64, np.int64))
    for kt in (np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint64):
        assert _path([dict(n=(tile, 10))], ir.dtype_code(kt)) == nat.SEARCH_LDS
        assert _path([dict(n=(tile + 1, 10))], ir.dtype_code(kt)) == nat.SEARCH_SPLIT
    assert _path([dict(n=(1, 10)), dict(n=(tile, 10)), dict(n=(0, 10), sorted=0)], F32) == nat.SEARCH_LDS
    assert _path([dict(n=(1, 10)), dict(n=(tile + 1, 10)), dict(n=(5, 10))], F32) == nat.SEARCH_SPLIT  # mixed
    assert _path([dict(n=(1, 10)), dict(n=(10 * tile, 0), values=0, dst=0)], F32) == nat.SEARCH_SPLIT
    assert _path([], F32) == nat.SEARCH_LDS
    assert nat.search_path(_rows([dict(n=(tile + 1, 3), acc=1 << 29)]), F64) == nat.SEARCH_SPLIT
    # malformed tables
    assert _path([dict(n=(2, 10))], ir.dtype_code(np.int8)) < 0
    assert _path([dict(n=(2, 10))], 99) < 0
    assert _path([dict(n=(-2, 10))], F32) < 0
    assert _path([dict(n=(2, -10))], F32) < 0
    assert _path([dict(n=(2, 10), sorted=0)], F32) < 0
    assert _path([dict(n=(2, 10), values=0)], F32) < 0
    assert _path([dict(n=(2, 10), dst=0)], F32) < 0
    assert _path([dict(n=(2, 10), sorted=(1 << 20) + 4)], F64) < 0
    assert _path([dict(n=(2, 10), sorted=(1 << 20) + 4)], F32) == nat.SEARCH_LDS
    assert _path([dict(n=(2, 10), values=(1 << 24) + 4)], I64) < 0
    assert _path([dict(n=(2, 10), dst=(1 << 28) + 4)], F32) < 0
    assert _path([dict(n=(2, 10), acc=(1 << 29) + 4)], F32) < 0
    assert b"cubed_search_path" in nat.lib().cubed_last_error()
    with pytest.raises(nat.NativeError, match="cubed_search_path"):
        nat.search_path(_rows([dict(n=(2, 10), dst=0)]), F32)
    L = nat.lib()
    assert L.cubed_search_path(None, 1, F32) < 0
    # the compute entry refuses malformed arguments before any device call
    assert L.cubed_search_chunks(None, 1, F32, 0, 0, 1, None) == -1
    assert b"cubed_search_chunks" in L.cubed_last_error()
    assert L.cubed_search_chunks(1 << 20, 1, 99, 0, 0, 1, None) == -1       # unknown ktype
    assert L.cubed_search_chunks(1 << 20, 1, ir.dtype_code(np.int8), 0, 0, 1, None) == -1
    assert L.cubed_search_chunks(1 << 20, 1, F32, 2, 0, 1, None) == -1      # unknown flag bits
    assert L.cubed_search_chunks(1 << 20, 1, F32, 0, 2, 1, None) == -1      # unknown path
    assert L.cubed_search_chunks(1 << 20, 4, F32, 0, 0, 1 << 30, None) == -1  # grid too large
    assert b"cubed_search_chunks" in L.cubed_last_error()
    assert L.cubed_search_chunks(None, 0, F32, 0, 0, 0, None) == 0


# ------------------------------------------------------------------ struct layout

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "cubed_amd.h"
#define P(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("sizeof_search %zu\n", sizeof(cubed_search_task_t));
  printf("abi %d\n", CUBED_ABI_VERSION);
  printf("tile %d\n", CUBED_SEARCH_TILE);
  printf("values %d\n", CUBED_SEARCH_VALUES);
  printf("right %d\n", CUBED_SEARCH_RIGHT);
  printf("paths %d\n", CUBED_SEARCH_LDS * 10 + CUBED_SEARCH_SPLIT);
  P(cubed_search_task_t, sorted_base); P(cubed_search_task_t, values_base);
  P(cubed_search_task_t, acc_base); P(cubed_search_task_t, dst_base);
  P(cubed_search_task_t, n_sorted); P(cubed_search_task_t, n_values);
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
    assert c.pop("sizeof_search") == nat.SEARCH_TASK_DTYPE.itemsize
    assert c.pop("abi") == nat.ABI_VERSION == 19
    assert c.pop("tile") == nat.search_tile()
    assert c.pop("values") == nat.SEARCH_VALUES
    assert c.pop("right") == nat.SEARCH_RIGHT
    assert c.pop("paths") == nat.SEARCH_LDS * 10 + nat.SEARCH_SPLIT
    fields = {k.split(".")[1]: v for k, v in c.items()}
    assert set(fields) == set(nat.SEARCH_TASK_DTYPE.names)
    for f, off in fields.items():
        assert nat.SEARCH_TASK_DTYPE.fields[f][1] == off, f
        assert nat.SEARCH_TASK_DTYPE.fields[f][0].itemsize == 8


def test_new_symbols_are_exported():
    for name in ("cubed_search_tile", "cubed_search_path", "cubed_search_chunks"):
        assert name in nat.EXPORTED_SYMBOLS
