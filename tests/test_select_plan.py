"""nonzero, boolean-mask indexing and count_nonzero on CPU: the API rules, the
plans of the select ops, the task tables they lower to (nothing is launched)
and the binding.

The values themselves are checked on the GPU (tests/test_gpu_select.py)."""

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
from dryrun import DryExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SelectDryExecutor(DryExecutor):
    """DryExecutor that also records (instead of running) the select launches."""

    def execute_dag(self, *args, **kwargs):
        saved = Lw.SelectLaunch.run
        Lw.SelectLaunch.run = lambda launch, stream, _log=self.launched: _log.append(launch)
        try:
            return super().execute_dag(*args, **kwargs)
        finally:
            Lw.SelectLaunch.run = saved


@pytest.fixture
def sdry(built):
    return SelectDryExecutor()


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


def _lower(sdry, *ys):
    sdry.launched.clear()
    arrays_to_plan(*ys).execute(executor=sdry, array_names=[y.name for y in ys])
    return [l for l in sdry.launched if isinstance(l, Lw.SelectLaunch)]


@pytest.fixture
def phase1(monkeypatch):
    """Records the arrays every eager compute of core.ops is given, and reads
    the dry run's per-chunk counts as zeros (a dry run computes nothing and
    has no device to read from)."""
    from cubed_amd.core.array import CoreArray

    calls = []
    real = ops.compute

    def compute(*arrays, **kwargs):
        calls.append(arrays)
        return real(*arrays, **kwargs)

    monkeypatch.setattr(ops, "compute", compute)
    monkeypatch.setattr(CoreArray, "_read_stored", lambda self: np.zeros(self.shape, dtype=self.dtype))
    return calls


# ------------------------------------------------------------------ API rules


def test_the_three_functions_are_exported():
    for name in ("nonzero", "count_nonzero"):
        assert callable(getattr(xp, name)) and name in dir(xp)
    for name in ("select_count", "select_pack"):
        assert callable(getattr(cubed.core, name)) and name in cubed.core.__all__
    # the flattening is shared with the set functions, not copied
    from cubed_amd.array_api import manipulation_functions, set_functions

    assert set_functions._ravel is manipulation_functions._ravel


def test_nonzero_argument_errors():
    spec = _spec()
    with pytest.raises(ValueError, match="zero-dimensional"):
        xp.nonzero(_arr((), (), np.float32, spec))
    for dt in (np.complex64, np.complex128):
        with pytest.raises(TypeError, match="nonzero"):
            xp.nonzero(_arr((6,), (2,), dt, spec))


def test_mask_argument_errors():
    spec = _spec()
    x = _arr((6, 4), (3, 4), np.float32, spec)
    for mask in (np.zeros((6, 5), dtype=bool), _arr((4, 6), (2, 6), np.bool_, spec)):
        with pytest.raises(IndexError, match="did not match"):
            x[mask]
    row = np.zeros(6, dtype=bool)
    for key in ((row, 0), (row, slice(None)), (slice(None), np.zeros(4, dtype=bool)),
                (_arr((6,), (3,), np.bool_, spec), 1), (Ellipsis, np.zeros((6, 4), dtype=bool))):
        with pytest.raises(NotImplementedError, match="sole index"):
            x[key]
    for mask in (row, _arr((6,), (3,), np.bool_, spec)):
        with pytest.raises(NotImplementedError, match="fewer dimensions"):
            x[mask]
    for dt in (np.complex64, np.complex128):
        with pytest.raises(TypeError, match="complex"):
            _arr((6,), (2,), dt, spec)[np.zeros(6, dtype=bool)]


def test_integer_keys_are_as_before():
    spec = _spec()
    x = _arr((6, 4), (3, 4), np.float32, spec)
    assert x[[0, 2, 5]].shape == (3, 4)
    assert x[np.array([1, 0, 1]), 1].shape == (3,)
    assert x[1:4, 2].shape == (3,)


def test_count_nonzero_is_lazy_and_has_no_select_op():
    spec = _spec()
    x = _arr((5, 7, 9), (2, 3, 4), np.float32, spec)
    for kwargs, shape in ((dict(), ()), (dict(axis=0), (7, 9)), (dict(axis=(0, 1)), (9,)),
                          (dict(axis=1, keepdims=True), (5, 1, 9))):
        y = xp.count_nonzero(x, **kwargs)
        assert y.shape == shape and y.dtype == np.int64
        assert _ops(y.plan.dag) and not _ops(y.plan.dag, ir.SelectProgram)
    y = xp.count_nonzero(_arr((5, 7), (2, 3), np.bool_, spec), axis=1)
    assert y.shape == (5,) and y.dtype == np.int64 and not _ops(y.plan.dag, ir.SelectProgram)


# ------------------------------------------------------------------ phase 1


def test_phase_one_is_one_count_and_one_pack(sdry, phase1):
    spec = _spec(sdry)
    x = _arr((37, 46), (10, 16), np.float32, spec)
    res = xp.nonzero(x)
    assert len(phase1) == 1 and len(phase1[0]) == 2
    progs = [p for _, p, _ in _ops(arrays_to_plan(*phase1[0]).dag, ir.SelectProgram)]
    assert sorted((p.kind, p.payload) for p in progs) == [("count", None), ("pack", None)]
    assert all(p.dtype == np.float32 for p in progs)
    launches = [l for l in sdry.launched if isinstance(l, Lw.SelectLaunch)]
    assert sorted(l.kind for l in launches) == ["count", "pack"]
    # nothing selected: (0,) int64 arrays that compute nothing
    assert len(res) == 2 and all(a.shape == (0,) and a.dtype == np.int64 for a in res)
    assert not any(_ops(a.plan.dag, ir.SelectProgram) for a in res)

    phase1.clear()
    sdry.launched.clear()
    v = _arr((37, 46), (10, 16), np.int16, spec)
    for mask in (_arr((37, 46), (10, 16), np.bool_, spec), _arr((37, 46), (37, 5), np.bool_, spec),
                 np.zeros((37, 46), dtype=bool)):
        phase1.clear()
        got = v[mask]
        assert len(phase1) == 1 and len(phase1[0]) == 2
        progs = [p for _, p, _ in _ops(arrays_to_plan(*phase1[0]).dag, ir.SelectProgram)]
        assert sorted((p.kind, p.payload) for p in progs) == [("count", None), ("pack", "values")]
        assert all(p.dtype == np.bool_ for p in progs)
        assert [p.value_dtype for p in progs if p.kind == "pack"] == [np.dtype(np.int16)]
        assert got.shape == (0,) and got.dtype == np.int16


def test_empty_inputs_compute_nothing(sdry, phase1):
    spec = _spec(sdry)
    x = _arr((3, 0), (2, 1), np.float64, spec)
    res = xp.nonzero(x)
    assert len(res) == 2 and all(a.shape == (0,) and a.dtype == np.int64 for a in res)
    got = x[np.zeros((3, 0), dtype=bool)]
    assert got.shape == (0,) and got.dtype == np.float64
    assert phase1 == [] and sdry.launched == []


@pytest.mark.parametrize("nb", [1, 2, 5])
def test_count_and_pack_are_one_op_each(nb):
    spec = _spec()
    c = 1000
    n = (nb - 1) * c + 37
    f = _arr((n,), (c,), np.uint8, spec)
    g = _arr((n,), (c,), np.float64, spec)
    c = f.chunksize[0]
    scratch = Lw.select_scratch_bytes(c, 1, nat.SELECT_TILE_BYTES)
    cases = [
        (ops.select_count(f), "count", None, np.dtype(np.int64), (nb,), ((1,) * nb,), c),
        (ops.select_pack(f), "pack", None, np.dtype(np.int64), (n,), f.chunks, c),
        (ops.select_pack(f, g), "pack", "values", np.dtype(np.float64), (n,), f.chunks, 9 * c),
    ]
    for y, kind, payload, dtype, shape, chunks, in_bytes in cases:
        assert y.shape == shape and y.dtype == dtype and y.chunks == chunks
        for dag in (y.plan.dag, y.plan._finalize_dag(optimize_graph=True)):
            ((name, prog, op),) = _ops(dag, ir.SelectProgram)
            assert (prog.kind, prog.payload) == (kind, payload) and prog.dtype == np.uint8
            assert op.fusable is False and op.num_tasks == nb
            cfg = op.pipeline.config
            for b in range(nb):
                keys = cfg.block_function(("out", b))
                assert all(isinstance(k, tuple) for k in keys)          # whole single chunks
                assert [k[1] for k in keys] == [b] * (2 if payload else 1)
                assert [k[0] for k in keys] == ([f.name, g.name] if payload else [f.name])
            # two copies of every input chunk and of the output chunk, and the tile counts
            out_chunk = 8 if kind == "count" else c * dtype.itemsize
            assert op.projected_mem == 100_000_000 + 2 * in_bytes + 2 * out_chunk + scratch
            assert op.projected_mem <= op.allowed_mem
    with pytest.raises(ValueError, match="values of shape"):
        ops.select_pack(f, _arr((n,), (c // 2 if nb > 1 else 5,), np.float64, spec))
    with pytest.raises(TypeError, match="complex"):
        ops.select_pack(f, _arr((n,), (c,), np.complex64, spec))
    with pytest.raises(TypeError, match="not lowered"):
        ops.select_count(_arr((n,), (c,), np.complex64, spec))
    with pytest.raises(ValueError, match="1-d"):
        ops.select_count(_arr((4, 4), (2, 4), np.uint8, spec))
    with pytest.raises(ValueError, match="allowed_mem"):
        ops.select_pack(_arr((5000,), (2500,), np.float64, _spec(allowed_mem=60_000, reserved_mem=0)))


# ------------------------------------------------------------------ lowering


def _check_tables(sdry, f, g, flat_chunks):
    tile_bytes = nat.select_tile_bytes()
    assert tile_bytes == nat.SELECT_TILE_BYTES
    esize = np.dtype(f.dtype).itemsize
    ys = [ops.select_count(f), ops.select_pack(f), ops.select_pack(f, g)]
    launches = _lower(sdry, *ys)
    assert len(launches) == 3
    by_kind = {(l.kind, l.vsize): l for l in launches}
    F, G = f.zarray, g.zarray
    starts = np.concatenate([[0], np.cumsum(flat_chunks)[:-1]])
    for y, key in zip(ys, (("count", 0), ("pack", 0), ("pack", np.dtype(g.dtype).itemsize))):
        l = by_kind[key]
        assert l.ntasks == len(flat_chunks) and l.esize == esize
        assert l.ignore_sign == (np.dtype(f.dtype).kind == "f")
        assert l.work == -(-max(flat_chunks) * esize // tile_bytes)
        D = y.zarray
        for b, row in enumerate(l.rows):
            assert row["n"] == flat_chunks[b] and row["offset"] == starts[b]
            assert row["src_base"] == F.chunk_addr((b,)) and row["src_base"] % 16 == 0
            assert row["val_base"] == (G.chunk_addr((b,)) if key[1] else 0)
            assert row["dst_base"] == D.chunk_addr((b,))
        # every task has its own scratch for ceil(n * esize / tile bytes) + 1 int64
        sc = np.sort(l.rows["scratch_base"])
        need = (-(-max(flat_chunks) * esize // tile_bytes) + 1) * 8
        assert (sc > 0).all() and (sc % 8 == 0).all() and (np.diff(sc) >= need).all()
        assert l.scratch_bytes == sum(Lw.select_scratch_bytes(n, esize, tile_bytes) for n in flat_chunks)
        assert l.scratch_bytes >= len(flat_chunks) * need
    assert all(isinstance(l, Lw.SelectLaunch) for l in launches)


@pytest.mark.parametrize("dt,vdt", [(np.bool_, np.int64), (np.float32, np.int8), (np.int16, np.float32),
                                    (np.float64, np.uint16)])
def test_task_tables_1d(sdry, dt, vdt):
    spec = _spec(sdry)
    _check_tables(sdry, _arr((4099,), (1000,), dt, spec), _arr((4099,), (1000,), vdt, spec), [1000] * 4 + [99])


def test_task_tables_2d(sdry):
    from cubed_amd.array_api.manipulation_functions import _ravel

    spec = _spec(sdry)
    f = _ravel(_arr((37, 46), (10, 16), np.bool_, spec))
    g = _ravel(_arr((37, 46), (10, 16), np.float32, spec))
    assert f.chunks == ((138,) * 12 + (46,),) == g.chunks
    _check_tables(sdry, f, g, [138] * 12 + [46])


def test_bfloat16_ignores_the_sign(sdry):
    spec = _spec(sdry)
    f = xp.astype(_arr((100,), (40,), np.float32, spec), xp.bfloat16)
    (l,) = _lower(sdry, ops.select_count(f))
    assert l.esize == 2 and l.ignore_sign is True and l.vsize == 0
    assert Lw.select_predicate(np.uint64) == (8, False) and Lw.select_predicate(np.bool_) == (1, False)
    with pytest.raises(Lw.LoweringError, match="not lowered"):
        Lw.select_predicate(np.complex128)


def test_work_follows_the_tile(sdry):
    spec = _spec(sdry)
    for dt in (np.uint8, np.int16, np.float32, np.float64):
        T = nat.select_tile_bytes() // np.dtype(dt).itemsize
        for n, work in ((1, 1), (T - 1, 1), (T, 1), (T + 1, 2), (3 * T + 5, 4)):
            (l,) = _lower(sdry, ops.select_count(_arr((n,), (n,), dt, spec)))
            assert l.work == work and l.ntasks == 1
    T = nat.select_tile_bytes() // 8
    (l,) = _lower(sdry, ops.select_pack(_arr((2 * T + 10,), (T + 5,), np.int64, spec)))
    assert l.work == 2 and l.ntasks == 2


def test_select_task_checks():
    V = Lw.ArrView
    b1, f4, i8 = np.dtype(np.bool_), np.dtype(np.float32), np.dtype(np.int64)
    src, val = V(1 << 20, [9], [1], b1), V(1 << 22, [9], [1], f4)
    one, pos, out = V(1 << 26, [1], [1], i8), V(1 << 24, [9], [1], i8), V(1 << 25, [9], [1], f4)
    assert tuple(Lw.select_task(src, None, one, 24, "count", None).tolist()) == (1 << 20, 0, 1 << 26, 0, 9, 24)
    assert tuple(Lw.select_task(src, None, pos, 7, "pack", None).tolist()) == (1 << 20, 0, 1 << 24, 0, 9, 7)
    assert tuple(Lw.select_task(src, val, out, 0, "pack", "values").tolist()) == \
        (1 << 20, 1 << 22, 1 << 25, 0, 9, 0)
    bad = [
        ((src, None, one, 0, "sum", None), "kind"),
        ((src, val, one, 0, "count", "values"), "kind"),
        ((src, None, pos, 0, "pack", "first"), "kind"),
        ((src, val, out, 0, "pack", None), "value chunk"),
        ((src, None, out, 0, "pack", "values"), "value chunk"),
        ((V(1 << 20, [9], [2], b1), None, one, 0, "count", None), "compact"),
        ((V(1 << 20, [3, 3], [3, 1], b1), None, one, 0, "count", None), "1-d"),
        ((src, V(1 << 22, [8], [1], f4), out, 0, "pack", "values"), "8 values for 9"),
        ((src, None, V(1 << 26, [1], [1], np.dtype(np.int32)), 0, "count", None), "counts into"),
        ((src, None, V(1 << 26, [2], [1], i8), 0, "count", None), "counts into"),
        ((src, None, out, 0, "pack", None), "packs"),
        ((src, None, V(1 << 24, [8], [1], i8), 0, "pack", None), "packs"),
        ((src, val, pos, 0, "pack", "values"), "packs"),
    ]
    for args, msg in bad:
        with pytest.raises(Lw.LoweringError, match=msg):
            Lw.select_task(*args)


def test_lowering_rejects_other_shapes_of_task(sdry):
    from cubed_amd.core.ops import general_blockwise

    spec = _spec(sdry)
    f = _arr((40,), (16,), np.float32, spec)
    f64 = _arr((40,), (16,), np.float64, spec)
    g = _arr((40,), (16,), np.int16, spec)
    g8 = _arr((40,), (8,), np.int16, spec)

    def build(prog, fn, *arrays, shape=(3,), dtype=np.int64, chunks=((1, 1, 1),)):
        return general_blockwise(prog, fn, *arrays, shape=shape, dtype=dtype, chunks=chunks, fusable=False)

    P = ir.SelectProgram(kind="count", dtype=np.dtype(np.float32), nargs=1)
    PV = ir.SelectProgram(kind="pack", payload="values", dtype=np.dtype(np.float32),
                          value_dtype=np.dtype(np.int16), nargs=2)
    assert len(_lower(sdry, build(P, lambda k: [(f.name, k[1])], f))) == 1
    packed = dict(shape=(40,), dtype=np.int16, chunks=((16, 16, 8),))
    cases = [
        (build(P, lambda k: [(f.name, k[1]), (f.name, k[1])], f), "inputs"),
        (build(P, lambda k: [[(f.name, k[1])]], f), "whole single chunks"),
        (build(P, lambda k: [(f.name, 0)], f), "own chunk"),
        (build(P, lambda k: [(f64.name, k[1])], f64), "not a 1-d device array of float32"),
        (build(P, lambda k: [(f.name, k[1])], f, dtype=np.int32), "int32"),
        (build(PV, lambda k: [(f.name, k[1])], f, **packed), "inputs"),
        (build(PV, lambda k: [(f.name, k[1]), (g.name, k[1])], f, g, shape=(40,), dtype=np.int64,
               chunks=((16, 16, 8),)), "int64"),
        (build(PV, lambda k: [(f.name, k[1]), (g8.name, k[1])], f, g8, **packed), "chunked differently"),
        (build(ir.SelectProgram(kind="count", dtype=np.dtype(np.complex64), nargs=1),
               lambda k: [(f.name, k[1])], f), "not lowered"),
    ]
    for y, msg in cases:
        with pytest.raises(Lw.LoweringError, match=msg):
            _lower(sdry, y)


def test_several_ranks_raise(built):
    from dryrun import FakeComm

    ex = SelectDryExecutor(FakeComm(0, 2))
    spec = _spec(ex)
    for y in (ops.select_count(_arr((40,), (8,), np.float64, spec)),
              ops.select_pack(_arr((40,), (8,), np.bool_, spec), _arr((40,), (8,), np.float32, spec))):
        with pytest.raises(Lw.LoweringError, match="one GPU only"):
            arrays_to_plan(y).execute(executor=ex, array_names=[y.name])


# ------------------------------------------------------------------ host-side validation and the binding


def _rows(tasks):
    rows = np.zeros(len(tasks), dtype=nat.SELECT_TASK_DTYPE)
    for i, t in enumerate(tasks):
        rows[i]["src_base"], rows[i]["dst_base"] = t.get("src", 1 << 24), t.get("dst", 1 << 26)
        rows[i]["scratch_base"], rows[i]["n"] = t.get("scratch", 1 << 28), t["n"]
        rows[i]["val_base"], rows[i]["offset"] = t.get("val", 0), t.get("offset", 0)
    return rows


def test_select_work(built):
    B = nat.select_tile_bytes()
    C, P = nat.SELECT_COUNT, nat.SELECT_PACK
    assert nat.select_work(_rows([]), 4, True, C, 0) == 0
    assert nat.select_work(_rows([{"n": 0}]), 4, True, C, 0) == 0
    for esize in (1, 2, 4, 8):
        T = B // esize
        ns = [1, 2 * T + 1, T]
        assert nat.select_work(_rows([{"n": n} for n in ns]), esize, False, C, 0) == 3 == \
            -(-max(ns) * esize // B)
        assert nat.select_work(_rows([{"n": T}]), esize, False, P, 0) == 1
        assert nat.select_work(_rows([{"n": T + 1, "val": 1 << 25}]), esize, True, P, 8) == 2
    assert nat.select_work(_rows([{"n": 5, "val": (1 << 25) + 1}]), 1, False, P, 1) == 1
    bad = [
        (_rows([{"n": -1}]), 4, 0, C, 0, "negative"),
        (_rows([{"n": (1 << 40) + 1}]), 4, 0, C, 0, "too large"),
        (_rows([{"n": 5, "scratch": 0}]), 4, 0, C, 0, "scratch"),
        (_rows([{"n": 5, "scratch": (1 << 28) + 4}]), 4, 0, C, 0, "scratch"),
        (_rows([{"n": 5, "dst": 0}]), 4, 0, C, 0, "destination"),
        (_rows([{"n": 5, "src": 0}]), 4, 0, C, 0, "null chunk"),
        (_rows([{"n": 5, "src": (1 << 24) + 8}]), 4, 0, C, 0, "16 bytes"),
        (_rows([{"n": 5, "src": (1 << 24) + 4}]), 1, 0, P, 0, "16 bytes"),
        (_rows([{"n": 5, "dst": (1 << 26) + 4}]), 4, 0, C, 0, "aligned"),
        (_rows([{"n": 5, "dst": (1 << 26) + 4}]), 4, 0, P, 0, "aligned"),
        (_rows([{"n": 5, "dst": (1 << 26) + 2, "val": 1 << 25}]), 1, 0, P, 4, "aligned"),
        (_rows([{"n": 5, "val": (1 << 25) + 4}]), 1, 0, P, 8, "aligned"),
        (_rows([{"n": 5, "dst": 1 << 24}]), 4, 0, P, 0, "in place"),
        (_rows([{"n": 5, "dst": 1 << 24}]), 4, 0, C, 0, "in place"),
        (_rows([{"n": 5, "dst": 1 << 25, "val": 1 << 25}]), 1, 0, P, 4, "in place"),
        (_rows([{"n": 5, "val": 1 << 25}]), 1, 0, P, 0, "without a value size"),
        (_rows([{"n": 5}]), 1, 0, P, 4, "null values"),
        (_rows([{"n": 5}]), 3, 0, C, 0, "element size"),
        (_rows([{"n": 5}]), 0, 0, C, 0, "element size"),
        (_rows([{"n": 5}]), 16, 0, C, 0, "element size"),
        (_rows([{"n": 5}]), 4, 0, 2, 0, "kind"),
        (_rows([{"n": 5}]), 4, 0, C, 4, "kind"),
        (_rows([{"n": 5, "val": 1 << 25}]), 4, 0, P, 3, "value size"),
        (_rows([{"n": 5}]), 4, 2, C, 0, "sign flag"),
    ]
    for rows, esize, ign, kind, vsize, msg in bad:
        with pytest.raises(nat.NativeError, match=msg):
            nat.select_work(rows, esize, ign, kind, vsize)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "cubed_amd.h"
#define P(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("sizeof_select %zu\n", sizeof(cubed_select_task_t));
  printf("abi %d\n", CUBED_ABI_VERSION);
  printf("tile_bytes %d\n", CUBED_SELECT_TILE_BYTES);
  printf("kinds %d\n", CUBED_SELECT_COUNT * 10 + CUBED_SELECT_PACK);
  P(cubed_select_task_t, src_base); P(cubed_select_task_t, val_base);
  P(cubed_select_task_t, dst_base); P(cubed_select_task_t, scratch_base);
  P(cubed_select_task_t, n); P(cubed_select_task_t, offset);
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
    assert c.pop("sizeof_select") == nat.SELECT_TASK_DTYPE.itemsize
    assert c.pop("abi") == nat.ABI_VERSION == 19
    assert c.pop("tile_bytes") == nat.SELECT_TILE_BYTES == nat.select_tile_bytes()
    assert c.pop("kinds") == nat.SELECT_COUNT * 10 + nat.SELECT_PACK
    fields = {k.split(".")[1]: v for k, v in c.items()}
    assert set(fields) == set(nat.SELECT_TASK_DTYPE.names)
    for f, off in fields.items():
        assert nat.SELECT_TASK_DTYPE.fields[f][1] == off, f
        assert nat.SELECT_TASK_DTYPE.fields[f][0].itemsize == 8


def test_new_symbols_are_exported(built):
    import ctypes

    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in ("cubed_select_tile_bytes", "cubed_select_work", "cubed_select_chunks"):
        assert name in nat.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
