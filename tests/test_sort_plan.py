"""sort / argsort on CPU: the API rules, the block network, the plan they
build, the task tables they lower to (nothing is launched) and the host-side
pass planning.

The values themselves are checked on the GPU (tests/test_gpu_sort.py)."""

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
from cubed_amd.core.ops import sort_network
from cubed_amd.core.plan import arrays_to_plan
from cubed_amd.primitive.blockwise import apply_blockwise
from dryrun import DryExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SortDryExecutor(DryExecutor):
    """DryExecutor that also records (instead of running) sort launches."""

    def execute_dag(self, *args, **kwargs):
        saved = Lw.SortLaunch.run
        Lw.SortLaunch.run = lambda launch, stream, _log=self.launched: _log.append(launch)
        try:
            return super().execute_dag(*args, **kwargs)
        finally:
            Lw.SortLaunch.run = saved


@pytest.fixture
def sdry(built):
    return SortDryExecutor()


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


def _sort_ops(dag):
    return [(n, p, op) for n, p, op in _ops(dag) if isinstance(p, ir.SortProgram)]


# ------------------------------------------------------------------ API rules


@pytest.mark.parametrize("dt", [np.bool_, np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16,
                                np.uint32, np.uint64, np.float32, np.float64])
def test_result_dtypes_and_shapes(dt):
    x = _arr((6, 10), (2, 4), dt, _spec())
    for axis in (0, 1):
        s, a = xp.sort(x, axis=axis), xp.argsort(x, axis=axis, descending=True, stable=False)
        assert s.dtype == np.dtype(dt) and a.dtype == np.int64
        assert s.shape == a.shape == x.shape and s.chunks == a.chunks == x.chunks


def test_negative_and_default_axis():
    x = _arr((37, 5, 46), (10, 2, 16), np.float32, _spec())
    for y in (xp.sort(x), xp.sort(x, axis=-1), xp.argsort(x, axis=-1)):
        progs = [p for _, p, _ in _sort_ops(y.plan.dag)]
        assert progs and all(p.axis == 2 for p in progs)
    with pytest.raises((ValueError, IndexError)):
        xp.sort(x, axis=3)
    with pytest.raises((ValueError, IndexError)):
        xp.argsort(x, axis=-4)


@pytest.mark.parametrize("dt", ["bfloat16", "complex64", "complex128"])
def test_rejected_input_dtypes(dt):
    x = xp.astype(_arr((6,), (2,), np.float32, _spec()), getattr(xp, dt))
    with pytest.raises(TypeError):
        xp.sort(x)
    with pytest.raises(TypeError):
        xp.argsort(x)


def test_zero_d_raises_as_numpy():
    x0 = xp.asarray(3.0, spec=_spec())
    with pytest.raises(ValueError) as theirs:
        np.sort(np.array(3.0))
    # (np.argsort flattens a 0-d array instead; argsort here raises as sort does)
    for f in (xp.sort, xp.argsort):
        with pytest.raises(ValueError) as ours:
            f(x0)
        assert isinstance(ours.value, type(theirs.value))
        with pytest.raises(ValueError):
            f(x0, axis=0)


def test_zero_size_input_has_no_sort_op(sdry):
    x = _arr((0, 4), (1, 4), np.int32, _spec(sdry))
    for axis in (0, 1):
        s, a = xp.sort(x, axis=axis), xp.argsort(x, axis=axis)
        assert s is x
        assert a.shape == (0, 4) and a.dtype == np.int64
        assert not _sort_ops(a.plan.dag)
        got = a.compute()
        assert got.shape == (0, 4) and got.dtype == np.int64
    z = _arr((3, 0), (1, 1), np.float32, _spec(sdry))  # a zero-length axis
    assert xp.sort(z, axis=1) is z and not _sort_ops(xp.argsort(z, axis=1).plan.dag)
    assert not [l for l in sdry.launched if isinstance(l, Lw.SortLaunch)]


# ------------------------------------------------------------------ the block network

ROUNDS = {1: 0, 2: 1, 3: 3, 4: 3, 5: 6, 6: 6, 7: 6, 8: 6, 9: 10, 10: 10, 11: 10, 12: 10, 13: 10, 14: 10,
          15: 10, 16: 10, 17: 15, 100: 28}


def _merge_split_model(blocks, rounds):
    """Drive the network with a stable numpy merge of (key, index) pairs."""
    blocks = [b.copy() for b in blocks]
    for rnd in rounds:
        seen = set()
        new = list(blocks)
        for lo, hi in rnd:
            assert lo < hi < len(blocks) and not {lo, hi} & seen
            seen |= {lo, hi}
            both = np.concatenate([blocks[lo], blocks[hi]])
            both = both[np.lexsort((both["i"], both["v"]))]
            new[lo], new[hi] = both[:len(blocks[lo])], both[len(blocks[lo]):]
        blocks = new
    return np.concatenate(blocks)


@pytest.mark.parametrize("nb", list(range(1, 18)))
def test_sort_network_sorts_ragged_duplicate_heavy_blocks(nb):
    rounds = sort_network(nb)
    assert len(rounds) == ROUNDS[nb]
    rng = np.random.default_rng(nb)
    for chunk, last in ((5, 1), (5, 5), (4, 3), (1, 1)):
        n = (nb - 1) * chunk + min(last, chunk)
        for hi in (2, 4, 1000):
            pairs = np.zeros(n, dtype=[("v", np.int64), ("i", np.int64)])
            pairs["v"], pairs["i"] = rng.integers(0, hi, size=n), np.arange(n)
            blocks = [np.sort(pairs[s:s + chunk], order=["v", "i"]) for s in range(0, n, chunk)]
            assert len(blocks) == nb
            got = _merge_split_model(blocks, rounds)
            assert np.array_equal(got["i"], np.argsort(pairs["v"], kind="stable"))


def test_sort_network_round_counts():
    assert len(sort_network(100)) == ROUNDS[100]
    for nb in (3, 5, 100):
        for rnd in sort_network(nb):
            assert rnd  # a round without a real pair is dropped
    assert sort_network(3) == [[(0, 1)], [(1, 2)], [(0, 1)]]
    with pytest.raises(ValueError):
        sort_network(0)


# ------------------------------------------------------------------ plan shape


def test_one_block_is_one_sort_op():
    x = _arr((40, 64), (8, 64), np.float64, _spec())
    for f, pairs in ((xp.sort, False), (xp.argsort, True)):
        ops = _sort_ops(f(x, axis=1, descending=True).plan.dag)
        assert len(ops) == 1
        _, prog, op = ops[0]
        assert (prog.axis, prog.descending, prog.pairs, prog.dtype, prog.kind, prog.nargs) == \
            (1, True, pairs, np.dtype(np.float64), "chunk", 1)
        assert op.fusable is False and op.num_tasks == 5
    # sort itself adds no other op; argsort ends with the field selection
    assert len(_ops(xp.sort(x, axis=1).plan.dag)) == 1
    last = _ops(xp.argsort(x, axis=1).plan.dag)[-1]
    assert isinstance(last[1], ir.ExprProgram) and last[2].target_array.dtype == np.int64


@pytest.mark.parametrize("n,chunk,rounds", [(40, 16, 3), (40, 8, 6)])
def test_several_blocks_are_chunk_plus_merge_rounds(n, chunk, rounds):
    x = _arr((6, n), (3, chunk), np.float32, _spec())
    ops = _sort_ops(xp.argsort(x, axis=1).plan.dag)
    assert [p.kind for _, p, _ in ops] == ["chunk"] + ["merge"] * rounds
    assert all(p.nargs == 2 for _, p, _ in ops[1:])
    pairs_dtype = np.dtype([("v", np.float32), ("i", np.int64)])
    for _, prog, op in ops:
        assert prog.pairs and op.fusable is False and op.num_tasks == 2 * x.numblocks[1]
        assert op.target_array.dtype == pairs_dtype and op.target_array.chunks == (3, chunk)
    # a merge task reads two chunks and writes one (a compressed and an
    # uncompressed copy of each, as blockwise counts), a chunk task its input,
    # its output and a scratch copy of the output
    cm = 3 * chunk * 12
    assert ops[1][2].projected_mem == 100_000_000 + 6 * cm
    assert ops[0][2].projected_mem == 100_000_000 + 2 * 3 * chunk * 4 + 2 * cm + cm


def test_non_last_axis_adds_the_permutes():
    x = _arr((37, 5, 46), (10, 2, 16), np.int32, _spec())
    ops = _ops(xp.sort(x, axis=0).plan.dag)
    assert [getattr(p, "name", None) for _, p, _ in ops] == ["permute_dims"] + ["sort"] * 4 + ["permute_dims"]
    front, back = ops[0][2].target_array, ops[-1][2].target_array
    assert front.shape == (5, 46, 37) and front.chunks == (2, 16, 10)
    assert back.shape == (37, 5, 46) and back.chunks == (10, 2, 16)
    assert all(p.axis == 2 for _, p, _ in ops[1:-1])
    # a later dim of extent 1 needs no permute
    y = _arr((37, 1), (10, 1), np.int32, _spec())
    assert [p.name for _, p, _ in _ops(xp.sort(y, axis=0).plan.dag)] == ["sort"] * 4


@pytest.mark.parametrize("optimize_function", [None, "multiple_inputs"])
def test_sort_ops_survive_optimization(optimize_function):
    from cubed_amd.core.optimization import multiple_inputs_optimize_dag

    fn = multiple_inputs_optimize_dag if optimize_function else None
    spec = _spec()
    x = _arr((40, 64), (8, 32), np.int32, spec)
    for f in (xp.sort, xp.argsort):
        for axis, nsort in ((0, 1 + 6), (1, 1 + 1)):
            y = f(x + 1, axis=axis) * 2  # an elementwise producer and consumer
            before = _sort_ops(y.plan.dag)
            after = _sort_ops(y.plan._finalize_dag(optimize_graph=True, optimize_function=fn))
            assert len(before) == len(after) == nsort
            for _, prog, op in after:
                assert type(prog) is ir.SortProgram and op.fusable is False


def test_chunk_too_large_for_allowed_mem():
    spec = _spec(allowed_mem="200MB", reserved_mem=0)
    x = xp.empty((4, 20_000_000), dtype=xp.float64, chunks=(1, 20_000_000), spec=spec)
    with pytest.raises(ValueError, match="allowed_mem"):
        xp.sort(x, axis=1)
    with pytest.raises(ValueError, match="allowed_mem"):
        xp.argsort(x, axis=1)


# ------------------------------------------------------------------ lowering


def _lower(sdry, y):
    sdry.launched.clear()
    arrays_to_plan(y).execute(executor=sdry, array_names=[y.name])
    return [l for l in sdry.launched if isinstance(l, Lw.SortLaunch)]


@pytest.mark.parametrize("pairs", [False, True])
def test_task_tables_3d_edge_chunks(sdry, pairs):
    x = _arr((37, 5, 46), (10, 2, 16), np.int32, _spec(sdry))
    y = (xp.argsort if pairs else xp.sort)(x, axis=2, descending=True)
    launches = _lower(sdry, y)
    assert [l.kind for l in launches] == ["chunk", "merge", "merge", "merge"]
    y_sorted = _sort_ops(y.plan.dag)[0][2].target_array  # what the chunk op writes
    assert all(l.pairs == pairs and l.descending and l.ktype == ir.dtype_code(np.int32) for l in launches)
    assert all(l.flags == nat.SORT_DESCENDING | (nat.SORT_PAIRS if pairs else 0) for l in launches)
    blocks = list(itertools.product(range(4), range(3), range(3)))
    chunk = launches[0]
    assert chunk.ntasks == len(blocks) and chunk.passes == 0 and chunk.scratch_bytes == 0
    for row, b in zip(chunk.rows, blocks):
        ext = [x.chunks[d][b[d]] for d in range(3)]
        assert (row["rows"], row["n"]) == (ext[0] * ext[1], ext[2]), b
        assert row["src_row_stride"] == row["dst_row_stride"] == ext[2]
        assert row["index_base"] == 16 * b[2]
        assert row["src_base"] != 0 and row["dst_base"] == y_sorted.chunk_addr(b, "v" if pairs else None)
        assert (row["dst_idx_base"] != 0) == pairs and row["scratch_base"] == 0
    assert len(set(chunk.rows["src_base"].tolist())) == len(blocks)
    assert chunk.work == 1  # at most 20 rows padded to 16 elements: 320 of a tile's 2048
    # rounds of sort_network(3): (0, 1), (1, 2), (0, 1); the other block is copied
    for launch, (lo, hi) in zip(launches[1:], [(0, 1), (1, 2), (0, 1)]):
        assert launch.ntasks == len(blocks)
        for row, b in zip(launch.rows, blocks):
            ext = [x.chunks[d][b[d]] for d in range(3)]
            assert row["rows"] == ext[0] * ext[1]
            if b[2] == lo:
                want = (nat.MERGE_LOW, ext[2], x.chunks[2][hi])
            elif b[2] == hi:
                want = (nat.MERGE_HIGH, x.chunks[2][lo], ext[2])
            else:
                want = (nat.MERGE_COPY, ext[2], 0)
            assert (row["role"], row["na"], row["nb"]) == want, b
            assert row["dst_row_stride"] == ext[2] and row["lo_row_stride"] == row["na"]
            assert (row["hi_base"] == 0) == (row["role"] == nat.MERGE_COPY)
            assert (row["dst_idx_base"] != 0) == pairs and (row["lo_idx_base"] != 0) == pairs
    # the tasks of a round read the chunks the round before wrote
    first, second = launches[1], launches[2]
    i01, i11 = blocks.index((0, 0, 1)), blocks.index((0, 0, 2))
    assert second.rows[i01]["lo_base"] == first.rows[i01]["dst_base"]
    assert second.rows[i01]["hi_base"] == first.rows[i11]["dst_base"]
    assert second.rows[i11]["role"] == nat.MERGE_HIGH and second.rows[i11]["lo_base"] == first.rows[i01]["dst_base"]


def test_in_chunk_passes_get_scratch_owned_by_the_plan(sdry):
    import gc

    tile = nat.sort_tile()
    spec = _spec(sdry)
    x = _arr((3, 3 * tile + 5), (2, 3 * tile + 5), np.float64, spec)
    arrays_to_plan(x).execute(executor=sdry, array_names=[x.name])
    gc.collect()
    before = sdry.owned_bytes()
    y = xp.argsort(x, axis=1)
    (launch,) = _lower(sdry, y)
    assert launch.passes == 2 and launch.ntasks == 2
    n = 3 * tile + 5
    r256 = lambda b: -(-b // 256) * 256  # noqa: E731
    assert launch.scratch_bytes == 2 * r256(2 * n * 8) + 2 * r256(1 * n * 8)
    assert launch.work == 2 * 4
    a, b = launch.rows
    assert a["scratch_base"] % 256 == 0 and a["scratch_idx_base"] == a["scratch_base"] + r256(2 * n * 8)
    assert b["scratch_base"] == a["scratch_idx_base"] + r256(2 * n * 8)
    assert sdry.owned_bytes() >= before + launch.scratch_bytes + launch.rows.nbytes
    del y, launch, a, b
    sdry.launched.clear()
    sdry.last_schedule = None
    gc.collect()
    assert sdry.owned_bytes() == before


def test_rechunk_in_front_of_a_sort_is_not_read_through(sdry):
    x = _arr((40, 64), (8, 64), np.float64, _spec(sdry))
    y = xp.sort(x.rechunk((40, 16)), axis=1)
    sdry.launched.clear()
    arrays_to_plan(y).execute(executor=sdry, array_names=[y.name])
    kinds = [type(l).__name__ for l in sdry.launched]
    assert kinds.count("CopyLaunch") >= 1 and kinds.count("SortLaunch") == 1 + 3


def test_several_ranks_raise(built):
    from dryrun import FakeComm

    ex = SortDryExecutor(FakeComm(0, 2))
    x = _arr((40, 64), (8, 64), np.float64, _spec(ex))
    y = xp.sort(x, axis=1)
    with pytest.raises(Lw.LoweringError, match="sort runs on one GPU only"):
        arrays_to_plan(y).execute(executor=ex, array_names=[y.name])


# ------------------------------------------------------------------ cubed_sort_plan


def _rows(tasks):
    rows = np.zeros(len(tasks), dtype=nat.SORT_TASK_DTYPE)
    for i, t in enumerate(tasks):
        r, n = t["shape"]
        rows[i]["src_base"], rows[i]["dst_base"] = t.get("src", 1 << 20), t.get("dst", 1 << 24)
        rows[i]["dst_idx_base"] = t.get("idx", 0)
        rows[i]["rows"], rows[i]["n"] = r, n
        rows[i]["src_row_stride"] = t.get("sstride", n)
        rows[i]["dst_row_stride"] = t.get("dstride", n)
        rows[i]["index_base"] = t.get("index_base", 0)
    return rows


def _plan(tasks, ktype, pairs=False):
    import ctypes

    rows = _rows(tasks)
    passes, nbytes = ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = nat.lib().cubed_sort_plan(rows.ctypes.data, len(rows), ktype, int(pairs), ctypes.byref(passes),
                                   ctypes.byref(nbytes))
    return rc, passes.value, nbytes.value


def test_sort_plan(built):
    tile = nat.sort_tile()
    assert tile == 2048 and 1024 <= tile <= 4096 and tile & (tile - 1) == 0
    F32, F64, I64 = (ir.dtype_code(t) for t in (np.float32, np.float64, np.int64))
    r256 = lambda b: -(-b // 256) * 256  # noqa: E731
    for n, want in ((1, 0), (tile - 1, 0), (tile, 0), (tile + 1, 1), (2 * tile, 1), (2 * tile + 1, 2),
                    (4 * tile, 2), (4 * tile + 1, 3), (70_001, 6)):
        rc, passes, nbytes = _plan([dict(shape=(3, n))], F32)
        assert (rc, passes) == (0, want), n
        assert nbytes == (r256(3 * n * 4) if want else 0)
    # the pass count of a launch is that of its longest row; every task gets scratch
    tasks = [dict(shape=(2, 100)), dict(shape=(1, tile + 1)), dict(shape=(0, 10 * tile))]
    assert _plan(tasks, F64) == (0, 1, r256(200 * 8) + r256((tile + 1) * 8))
    tasks = [dict(shape=(2, 100), idx=1 << 28), dict(shape=(1, tile + 1), idx=1 << 29)]
    assert _plan(tasks, F32, pairs=True) == \
        (0, 1, r256(200 * 4) + r256(200 * 8) + r256((tile + 1) * 4) + r256((tile + 1) * 8))
    assert _plan(tasks, I64, pairs=True)[2] == 2 * r256(200 * 8) + 2 * r256((tile + 1) * 8)
    assert _plan([], F32) == (0, 0, 0)
    # malformed tables
    assert _plan([dict(shape=(2, 10))], ir.dtype_code(np.int8))[0] < 0
    assert _plan([dict(shape=(2, 10))], 99)[0] < 0
    assert _plan([dict(shape=(2, -1))], F32)[0] < 0
    assert _plan([dict(shape=(-2, 10))], F32)[0] < 0
    assert _plan([dict(shape=(2, 10), src=0)], F32)[0] < 0
    assert _plan([dict(shape=(2, 10), src=(1 << 20) + 4)], F64)[0] < 0
    assert _plan([dict(shape=(2, 10), src=(1 << 20) + 4)], F32)[0] == 0
    assert _plan([dict(shape=(2, 10))], F32, pairs=True)[0] < 0  # no index address
    assert _plan([dict(shape=(2, 10), idx=(1 << 28) + 4)], F32, pairs=True)[0] < 0
    assert _plan([dict(shape=(2, 10), dstride=9)], F32)[0] < 0
    assert _plan([dict(shape=(2, 10), index_base=-1)], F32)[0] < 0
    assert b"cubed_sort_plan" in nat.lib().cubed_last_error()
    L = nat.lib()
    assert L.cubed_sort_plan(None, 1, F32, 0, None, None) < 0
    # the compute entries refuse malformed arguments before any device call
    assert L.cubed_sort_chunks(None, 1, F32, 0, 0, 1, None) == -1
    assert b"cubed_sort_chunks" in L.cubed_last_error()
    assert L.cubed_sort_chunks(1 << 20, 1, 99, 0, 0, 1, None) == -1
    assert L.cubed_sort_chunks(1 << 20, 1, F32, 4, 0, 1, None) == -1
    assert L.cubed_sort_chunks(1 << 20, 1, F32, 0, -1, 1, None) == -1
    assert L.cubed_sort_chunks(1 << 20, 4, F32, 0, 0, 1 << 30, None) == -1
    assert L.cubed_merge_split(None, 1, F32, 0, 1, None) == -1
    assert b"cubed_merge_split" in L.cubed_last_error()
    assert L.cubed_merge_split(1 << 20, 1, 99, 0, 1, None) == -1
    assert L.cubed_merge_split(1 << 20, 4, F32, 0, 1 << 30, None) == -1
    assert L.cubed_sort_chunks(None, 0, F32, 0, 0, 0, None) == 0


def test_sort_work():
    rows = _rows([dict(shape=(1000, 10)), dict(shape=(3, 2048)), dict(shape=(3, 2049)), dict(shape=(0, 99999))])
    assert Lw.sort_work(rows[:1], 2048) == 8      # 1000 rows padded to 16: 16000 / 2048
    assert Lw.sort_work(rows[1:2], 2048) == 3
    assert Lw.sort_work(rows[2:3], 2048) == 6
    assert Lw.sort_work(rows, 2048) == 8


# ------------------------------------------------------------------ struct layout

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "cubed_amd.h"
#define P(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("sizeof_sort %zu\n", sizeof(cubed_sort_task_t));
  printf("sizeof_merge %zu\n", sizeof(cubed_merge_task_t));
  printf("abi %d\n", CUBED_ABI_VERSION);
  printf("tile %d\n", CUBED_SORT_TILE);
  printf("flags %d\n", CUBED_SORT_DESCENDING * 10 + CUBED_SORT_PAIRS);
  printf("roles %d\n", CUBED_MERGE_LOW * 100 + CUBED_MERGE_HIGH * 10 + CUBED_MERGE_COPY);
  P(cubed_sort_task_t, src_base); P(cubed_sort_task_t, dst_base); P(cubed_sort_task_t, dst_idx_base);
  P(cubed_sort_task_t, scratch_base); P(cubed_sort_task_t, scratch_idx_base);
  P(cubed_sort_task_t, rows); P(cubed_sort_task_t, n);
  P(cubed_sort_task_t, src_row_stride); P(cubed_sort_task_t, dst_row_stride);
  P(cubed_sort_task_t, index_base);
  P(cubed_merge_task_t, lo_base); P(cubed_merge_task_t, lo_idx_base);
  P(cubed_merge_task_t, hi_base); P(cubed_merge_task_t, hi_idx_base);
  P(cubed_merge_task_t, dst_base); P(cubed_merge_task_t, dst_idx_base);
  P(cubed_merge_task_t, rows); P(cubed_merge_task_t, na); P(cubed_merge_task_t, nb);
  P(cubed_merge_task_t, lo_row_stride); P(cubed_merge_task_t, hi_row_stride);
  P(cubed_merge_task_t, dst_row_stride); P(cubed_merge_task_t, role);
  return 0;
}
"""


def test_task_layouts_match_binding(built, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert c.pop("sizeof_sort") == nat.SORT_TASK_DTYPE.itemsize
    assert c.pop("sizeof_merge") == nat.MERGE_TASK_DTYPE.itemsize
    assert c.pop("abi") == nat.ABI_VERSION == 19
    assert c.pop("tile") == nat.sort_tile()
    assert c.pop("flags") == nat.SORT_DESCENDING * 10 + nat.SORT_PAIRS
    assert c.pop("roles") == nat.MERGE_LOW * 100 + nat.MERGE_HIGH * 10 + nat.MERGE_COPY
    for struct, dt in (("cubed_sort_task_t", nat.SORT_TASK_DTYPE), ("cubed_merge_task_t", nat.MERGE_TASK_DTYPE)):
        fields = {k.split(".")[1]: v for k, v in c.items() if k.startswith(struct + ".")}
        assert set(fields) == set(dt.names)
        for f, off in fields.items():
            assert dt.fields[f][1] == off, (struct, f)
            assert dt.fields[f][0].itemsize == 8


def test_new_symbols_are_exported():
    for name in ("cubed_sort_tile", "cubed_sort_plan", "cubed_sort_chunks", "cubed_merge_split"):
        assert name in nat.EXPORTED_SYMBOLS
