"""cumulative_sum on CPU: the API rules, the plan it builds, the scan task
tables it lowers to (nothing is launched) and the host-side choice of kernel.

The values themselves are checked on the GPU (tests/test_gpu_scan.py)."""

import gc
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


class ScanDryExecutor(DryExecutor):
    """DryExecutor that also records (instead of running) scan launches."""

    def execute_dag(self, *args, **kwargs):
        saved = Lw.ScanLaunch.run
        Lw.ScanLaunch.run = lambda launch, stream, _log=self.launched: _log.append(launch)
        try:
            return super().execute_dag(*args, **kwargs)
        finally:
            Lw.ScanLaunch.run = saved


@pytest.fixture
def sdry(built):
    return ScanDryExecutor()


def _spec(ex=None, allowed_mem="2GB", reserved_mem="100MB"):
    return cubed.Spec(allowed_mem=allowed_mem, reserved_mem=reserved_mem, executor=ex)


def _arr(shape, chunks, dtype, spec):
    return cubed.from_array(np.zeros(shape, dtype=dtype), chunks=chunks, spec=spec)


# ------------------------------------------------------------------ API rules


@pytest.mark.parametrize("in_dt,want", [
    (np.float32, np.float32), (np.float64, np.float64),
    (np.int8, np.int64), (np.int16, np.int64), (np.int32, np.int64), (np.int64, np.int64),
    (np.uint8, np.uint64), (np.uint16, np.uint64), (np.uint32, np.uint64), (np.uint64, np.uint64),
])
def test_default_result_dtype(in_dt, want):
    x = _arr((6, 4), (2, 4), in_dt, _spec())
    assert xp.cumulative_sum(x, axis=0).dtype == np.dtype(want)


@pytest.mark.parametrize("in_dt,req", [(np.int8, np.int32), (np.float32, np.float64), (np.int32, np.float32),
                                       (np.float64, np.float32), (np.uint8, np.uint16), (np.int64, np.int64)])
def test_explicit_dtype_is_honoured(in_dt, req):
    x = _arr((6, 4), (2, 4), in_dt, _spec())
    assert xp.cumulative_sum(x, axis=1, dtype=req).dtype == np.dtype(req)


def test_axis_rules():
    spec = _spec()
    x2 = _arr((6, 4), (2, 4), np.float64, spec)
    with pytest.raises(ValueError):
        xp.cumulative_sum(x2)
    x0 = xp.asarray(3.0, spec=spec)
    with pytest.raises(ValueError):
        xp.cumulative_sum(x0)
    with pytest.raises(ValueError):
        xp.cumulative_sum(x0, axis=0)
    x1 = _arr((10,), (4,), np.float64, spec)
    assert xp.cumulative_sum(x1).shape == (10,)
    with pytest.raises((ValueError, IndexError)):
        xp.cumulative_sum(x2, axis=2)


def test_include_initial_is_not_implemented():
    x = _arr((10,), (4,), np.float64, _spec())
    with pytest.raises(NotImplementedError):
        xp.cumulative_sum(x, include_initial=True)


@pytest.mark.parametrize("dt", ["bool", "bfloat16", "complex64", "complex128"])
def test_rejected_input_dtypes(dt):
    spec = _spec()
    x = xp.astype(_arr((6,), (2,), np.float32, spec), getattr(xp, dt))
    with pytest.raises(TypeError, match="Only real numeric dtypes"):
        xp.cumulative_sum(x)
    with pytest.raises(TypeError, match="Only real numeric dtypes"):
        xp.cumulative_sum(_arr((6,), (2,), np.float32, spec), dtype=getattr(xp, dt))


def _scan_ops(dag):
    out = []
    for name, d in dag.nodes(data=True):
        p = d.get("pipeline")
        if p is not None and p.function is apply_blockwise and isinstance(p.config.function, ir.ScanProgram):
            out.append((name, d))
    return out


def test_negative_axis_shape_and_chunks():
    x = _arr((37, 5, 46), (10, 2, 16), np.float32, _spec())
    y = xp.cumulative_sum(x, axis=-1)
    assert y.shape == x.shape and y.chunks == x.chunks
    progs = [d["pipeline"].config.function for _, d in _scan_ops(y.plan.dag)]
    assert progs and all(p.axis == 2 for p in progs)


def test_zero_size_input_has_no_scan(sdry):
    x = _arr((0, 4), (1, 4), np.int32, _spec(sdry))
    y = xp.cumulative_sum(x, axis=0)
    assert y.shape == (0, 4) and y.dtype == np.int64
    assert not _scan_ops(y.plan.dag)
    got = y.compute()
    assert got.shape == (0, 4) and got.dtype == np.int64
    assert not [l for l in sdry.launched if isinstance(l, Lw.ScanLaunch)]


# ------------------------------------------------------------------ plan shape


def _op_chain(y):
    """Programs of the ops leading to ``y``, in topological order."""
    import networkx as nx

    dag = y.plan.dag
    out = []
    for name in nx.topological_sort(dag):
        p = dag.nodes[name].get("pipeline")
        if p is not None and p.function is apply_blockwise:
            out.append((name, p.config.function, dag.nodes[name]["primitive_op"]))
    return out


def test_single_block_axis_is_one_scan_op():
    x = _arr((40, 64), (8, 64), np.float64, _spec())
    y = xp.cumulative_sum(x, axis=1)
    ops = _op_chain(y)
    assert len(ops) == 1
    _, prog, op = ops[0]
    assert isinstance(prog, ir.ScanProgram)
    assert (prog.axis, prog.exclusive, prog.carry, prog.dtype) == (1, False, False, np.dtype(np.float64))
    assert op.fusable is False and op.num_tasks == 5


def test_multi_block_axis_is_sums_merge_carry_scan():
    x = _arr((40, 64), (8, 32), np.float32, _spec())
    y = xp.cumulative_sum(x, axis=0)
    ops = _op_chain(y)
    assert len(ops) == 4
    (_, sums, sums_op), (_, merge, _), (_, carry, carry_op), (_, scan, scan_op) = ops
    assert isinstance(sums, ir.ExprProgram) and sums.reduce is not None and sums.reduce.axes == (0,)
    assert sums_op.target_array.dtype == np.float64 and sums_op.target_array.shape == (5, 64)
    assert sums_op.target_array.chunks == (1, 32)
    assert isinstance(merge, ir.PerBlockProgram) or isinstance(merge, ir.ExprProgram)
    assert isinstance(carry, ir.ScanProgram) and carry.exclusive and not carry.carry and carry.axis == 0
    assert carry.dtype == np.float64
    assert carry_op.target_array.shape == (5, 64) and carry_op.target_array.chunks == (5, 32)
    assert isinstance(scan, ir.ScanProgram) and scan.carry and not scan.exclusive
    assert scan.dtype == np.float32 and scan.nargs == 2
    assert not carry_op.fusable and not scan_op.fusable
    assert scan_op.target_array.shape == (40, 64) and scan_op.target_array.chunks == (8, 32)
    # block (3, 1) reads its own chunk and the carry chunk of its column of blocks
    xk, ck = scan_op.pipeline.config.block_function(("out", 3, 1))
    assert xk[1:] == (3, 1) and ck[1:] == (0, 1)
    # the carry chunk is counted in the op's projected memory: two copies each
    # of the input chunk, the output chunk and the carry chunk
    assert scan_op.projected_mem == 100_000_000 + 2 * (8 * 32 * 4) * 2 + 2 * (5 * 32 * 8)


def test_integer_accumulators():
    spec = _spec()
    for dt, acc in ((np.int32, np.int64), (np.uint8, np.uint64)):
        y = xp.cumulative_sum(_arr((40,), (8,), dt, spec))
        scans = [p for _, p, _ in _op_chain(y) if isinstance(p, ir.ScanProgram)]
        assert [p.dtype for p in scans] == [np.dtype(acc)] * 2


@pytest.mark.parametrize("optimize_function", [None, "multiple_inputs"])
def test_scan_ops_survive_optimization(optimize_function):
    from cubed_amd.core.optimization import multiple_inputs_optimize_dag

    fn = multiple_inputs_optimize_dag if optimize_function else None
    spec = _spec()
    x = _arr((40, 64), (8, 32), np.int32, spec)
    # an elementwise producer (the astype to int64) and consumer on each side
    for axis, nscan in ((0, 2), (1, 2)):
        y = xp.cumulative_sum(x + 1, axis=axis) * 2
        before = _scan_ops(y.plan.dag)
        dag = y.plan._finalize_dag(optimize_graph=True, optimize_function=fn)
        after = _scan_ops(dag)
        assert len(before) == len(after) == nscan
        for _, d in after:
            assert d["primitive_op"].fusable is False
    x1 = _arr((40, 64), (8, 64), np.int32, spec)
    y = xp.cumulative_sum(x1 + 1, axis=1) * 2  # nb == 1: a linear chain of three maps
    after = _scan_ops(y.plan._finalize_dag(optimize_graph=True, optimize_function=fn))
    assert len(after) == 1
    assert type(after[0][1]["pipeline"].config.function) is ir.ScanProgram


def test_merged_totals_must_fit_allowed_mem():
    # 1000 blocks of (1, 100000) f64 along axis 0: the merged totals are an
    # 800 MB chunk, the array's own chunks 800 kB
    spec = _spec(allowed_mem="200MB", reserved_mem=0)
    x = xp.empty((1000, 100_000), dtype=xp.float64, chunks=(1, 100_000), spec=spec)
    with pytest.raises(ValueError, match=r"Not enough memory for cumulative_sum. Increase allowed_mem \(200000000\) "
                                         "or decrease chunk size"):
        xp.cumulative_sum(x, axis=0)
    # the other axis has one block: no totals to merge
    assert xp.cumulative_sum(x, axis=1).shape == x.shape


# ------------------------------------------------------------------ lowering


def _lower(sdry, x, axis):
    y = xp.cumulative_sum(x, axis=axis)
    sdry.launched.clear()
    arrays_to_plan(y).execute(executor=sdry, array_names=[y.name])
    return y, [l for l in sdry.launched if isinstance(l, Lw.ScanLaunch)]


def _check_tables(x, y, scans, axis):
    nb = x.numblocks[axis]
    if nb == 1:
        assert len(scans) == 1
        final = scans[0]
    else:
        assert len(scans) == 2
        carry, final = scans
        assert carry.exclusive and not final.exclusive
        merged_blocks = [n if d != axis else 1 for d, n in enumerate(x.numblocks)]
        assert carry.ntasks == int(np.prod(merged_blocks))
        assert not carry.rows["carry_base"].any()
        for row, b in zip(carry.rows, itertools.product(*[range(n) for n in merged_blocks])):
            ext = [x.chunks[d][b[d]] if d != axis else nb for d in range(x.ndim)]
            assert (row["outer"], row["n"], row["inner"]) == \
                (int(np.prod(ext[:axis])), nb, int(np.prod(ext[axis + 1:])))
    blocks = list(itertools.product(*[range(n) for n in x.numblocks]))
    assert final.ntasks == len(blocks) == len(final.rows)
    target = y.zarray_maybe_lazy
    for row, b in zip(final.rows, blocks):
        ext = [x.chunks[d][b[d]] for d in range(x.ndim)]
        outer, n, inner = int(np.prod(ext[:axis])), ext[axis], int(np.prod(ext[axis + 1:]))
        assert (row["outer"], row["n"], row["inner"]) == (outer, n, inner), b
        assert (row["src_n_stride"], row["src_outer_stride"]) == (inner, n * inner)
        assert (row["dst_n_stride"], row["dst_outer_stride"]) == (inner, n * inner)
        assert row["dst_base"] == target.chunk_addr(b)
        if nb == 1:
            assert row["carry_base"] == 0
            continue
        assert row["carry_base"] != 0
        # the carry chunk of b's row of blocks is the output chunk of the
        # carry launch's task for that row; block b starts b[axis] planes in
        cb = tuple(0 if d == axis else b[d] for d in range(x.ndim))
        crow = carry.rows[[tuple(k) for k in itertools.product(*[range(m) for m in merged_blocks])].index(cb)]
        acc_isz = 8
        assert row["carry_base"] == crow["dst_base"] + b[axis] * inner * acc_isz, b
        assert row["carry_outer_stride"] == nb * inner


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_task_tables_3d(sdry, axis):
    x = _arr((37, 5, 46), (10, 2, 16), np.int32, _spec(sdry))
    y, scans = _lower(sdry, x, axis)
    _check_tables(x, y, scans, axis)
    want = {0: nat.SCAN_COLS, 1: nat.SCAN_COLS, 2: nat.SCAN_ROWS}[axis]
    assert scans[-1].path == want  # the 14-wide edge chunks keep the launch at one element per lane


def test_task_tables_1d(sdry):
    x = _arr((10_000,), (1024,), np.float32, _spec(sdry))
    y, scans = _lower(sdry, x, 0)
    _check_tables(x, y, scans, 0)
    assert [s.path for s in scans] == [nat.SCAN_ROWS, nat.SCAN_ROWS]
    assert [s.vtype for s in scans] == [Lw.V_F64, Lw.V_F32]
    assert scans[1].rows["n"].tolist() == [1024] * 9 + [10_000 - 9 * 1024]


def test_single_block_axis_table(sdry):
    x = _arr((40, 64), (8, 64), np.float64, _spec(sdry))
    y, scans = _lower(sdry, x, 1)
    _check_tables(x, y, scans, 1)


def test_aligned_chunks_take_the_wide_columns_kernel(sdry):
    x = _arr((40, 64), (8, 32), np.int64, _spec(sdry))
    y, scans = _lower(sdry, x, 0)
    _check_tables(x, y, scans, 0)
    assert [s.path for s in scans] == [nat.SCAN_COLS_V4, nat.SCAN_COLS_V4]


def test_rechunk_in_front_of_a_scan_is_not_read_through(sdry):
    spec = _spec(sdry)
    x = _arr((40, 64), (8, 64), np.float64, spec)
    y = xp.cumulative_sum(x.rechunk((40, 16)), axis=0)
    sdry.launched.clear()
    arrays_to_plan(y).execute(executor=sdry, array_names=[y.name])
    kinds = [type(l).__name__ for l in sdry.launched]
    assert kinds.count("CopyLaunch") >= 1 and kinds.count("ScanLaunch") == 1
    scan = sdry.launched[-1]
    assert set(zip(scan.rows["outer"].tolist(), scan.rows["n"].tolist(), scan.rows["inner"].tolist())) == \
        {(1, 40, 16)}


def test_tables_are_owned_by_the_plan(sdry):
    spec = _spec(sdry)
    x = _arr((37, 5, 46), (10, 2, 16), np.int64, spec)
    arrays_to_plan(x).execute(executor=sdry, array_names=[x.name])
    gc.collect()
    before = sdry.owned_bytes()
    y, scans = _lower(sdry, x, 0)
    held = sdry.owned_bytes()
    assert held >= before + sum(s.rows.nbytes for s in scans)
    del y, scans
    sdry.launched.clear()
    sdry.last_schedule = None
    gc.collect()
    assert sdry.owned_bytes() == before


def test_several_ranks_raise(built):
    from dryrun import FakeComm

    ex = ScanDryExecutor(FakeComm(0, 2))
    x = _arr((40, 64), (8, 64), np.float64, _spec(ex))
    y = xp.cumulative_sum(x, axis=1)
    with pytest.raises(Lw.LoweringError, match="one GPU"):
        arrays_to_plan(y).execute(executor=ex, array_names=[y.name])


# ------------------------------------------------------------------ cubed_scan_path


def _rows(tasks):
    rows = np.zeros(len(tasks), dtype=nat.SCAN_TASK_DTYPE)
    for i, t in enumerate(tasks):
        outer, n, inner = t["shape"]
        rows[i]["src_base"], rows[i]["dst_base"] = t.get("src", 1 << 20), t.get("dst", 1 << 24)
        rows[i]["carry_base"] = t.get("carry", 0)
        rows[i]["outer"], rows[i]["n"], rows[i]["inner"] = outer, n, inner
        rows[i]["src_outer_stride"] = rows[i]["dst_outer_stride"] = n * inner
        rows[i]["src_n_stride"] = rows[i]["dst_n_stride"] = inner
        rows[i]["carry_outer_stride"] = t.get("planes", 1) * inner
    return rows


def _path(tasks, vtype):
    rows = _rows(tasks)
    return nat.lib().cubed_scan_path(rows.ctypes.data, len(rows), vtype)


def test_scan_path(built):
    assert _path([dict(shape=(5, 300, 1))], Lw.V_I64) == nat.SCAN_ROWS
    assert _path([dict(shape=(1, 1024, 1), carry=1 << 26)], Lw.V_F32) == nat.SCAN_ROWS
    for vt in (Lw.V_F32, Lw.V_F64, Lw.V_I64):
        assert _path([dict(shape=(2, 10, 16))], vt) == nat.SCAN_COLS_V4
        assert _path([dict(shape=(2, 10, 16), carry=1 << 26, planes=4)], vt) == nat.SCAN_COLS_V4
        # 46 = 16 + 16 + 14: one odd chunk narrows the whole launch
        assert _path([dict(shape=(2, 10, 16)), dict(shape=(2, 10, 16)), dict(shape=(2, 10, 14))], vt) == \
            nat.SCAN_COLS
    # 14 f32 columns: 56-byte rows; 6 f32 columns in f32 are not a multiple of 4 elements either
    assert _path([dict(shape=(1, 10, 6))], Lw.V_F32) == nat.SCAN_COLS
    # f64: an 8-byte-aligned base that is not 32-byte aligned
    assert _path([dict(shape=(2, 10, 16), src=(1 << 20) + 8)], Lw.V_F64) == nat.SCAN_COLS
    assert _path([dict(shape=(2, 10, 16), dst=(1 << 24) + 16)], Lw.V_F64) == nat.SCAN_COLS
    assert _path([dict(shape=(2, 10, 16), dst=(1 << 24) + 16)], Lw.V_F32) == nat.SCAN_COLS_V4
    assert _path([dict(shape=(2, 10, 16), carry=(1 << 26) + 8)], Lw.V_F32) == nat.SCAN_COLS
    # a mix of row and column tasks runs on the general kernel
    assert _path([dict(shape=(5, 300, 1)), dict(shape=(2, 10, 16))], Lw.V_I64) == nat.SCAN_COLS
    # empty tasks decide nothing
    assert _path([dict(shape=(0, 10, 3)), dict(shape=(2, 10, 16))], Lw.V_I64) == nat.SCAN_COLS_V4
    assert _path([dict(shape=(2, 10, 16))], 7) < 0
    assert _path([dict(shape=(2, -1, 16))], Lw.V_F64) < 0
    assert _path([dict(shape=(2, 10, 16), src=(1 << 20) + 4)], Lw.V_F64) < 0


# ------------------------------------------------------------------ struct layout

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "cubed_amd.h"
#define P(T, f) printf(#f " %zu\n", offsetof(T, f))
int main(void) {
  printf("sizeof %zu\n", sizeof(cubed_scan_task_t));
  printf("abi %d\n", CUBED_ABI_VERSION);
  printf("paths %d\n", CUBED_SCAN_ROWS * 100 + CUBED_SCAN_COLS * 10 + CUBED_SCAN_COLS_V4);
  P(cubed_scan_task_t, src_base); P(cubed_scan_task_t, dst_base); P(cubed_scan_task_t, carry_base);
  P(cubed_scan_task_t, outer); P(cubed_scan_task_t, n); P(cubed_scan_task_t, inner);
  P(cubed_scan_task_t, src_outer_stride); P(cubed_scan_task_t, src_n_stride);
  P(cubed_scan_task_t, dst_outer_stride); P(cubed_scan_task_t, dst_n_stride);
  P(cubed_scan_task_t, carry_outer_stride);
  return 0;
}
"""


def test_scan_task_layout_matches_binding(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert c.pop("sizeof") == nat.SCAN_TASK_DTYPE.itemsize
    assert c.pop("abi") == nat.ABI_VERSION
    assert c.pop("paths") == nat.SCAN_ROWS * 100 + nat.SCAN_COLS * 10 + nat.SCAN_COLS_V4
    assert set(c) == set(nat.SCAN_TASK_DTYPE.names)
    for f, off in c.items():
        assert nat.SCAN_TASK_DTYPE.fields[f][1] == off, f
