"""The unique_* set functions on the MI355X executor (``-m gpu``) against numpy.

Parity is UNPINNED against the reference: cubed v0.12.0 has no set functions.
``np.unique(x.ravel(), return_index=True, return_inverse=True,
return_counts=True)`` on the same data (numpy's default ``equal_nan=True``) is
the yardstick.  Every comparison is exact; values are compared with NaN equal
to NaN, and numpy's N-d inverse is compared flattened."""

import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
from cubed_amd import _native as nat
from cubed_amd import ir
from cubed_amd.core import ops
from cubed_amd.primitive.blockwise import apply_blockwise

pytestmark = pytest.mark.gpu

KEY_DTYPES = [np.float32, np.float64, np.int32, np.int64, np.uint32, np.uint64]
FUNCS = ("unique_values", "unique_counts", "unique_inverse", "unique_all")


@pytest.fixture(scope="module")
def ex(gpu_executor):
    return gpu_executor


@pytest.fixture(scope="module")
def T(built):
    return nat.unique_tile()


def _arr(ex, x, chunks=None):
    spec = cubed.Spec(allowed_mem="2GB", reserved_mem=0, executor=ex)
    return cubed.from_array(x, chunks=x.shape if chunks is None else chunks, spec=spec)


def _same(got, exp):
    if got.dtype != exp.dtype or got.shape != exp.shape:
        return False
    return np.array_equal(got, exp, equal_nan=True) if exp.dtype.kind == "f" else np.array_equal(got, exp)


def _check(ex, x, chunks=None, funcs=("unique_all",)):
    """The named functions equal np.unique on x; returns unique_all's result
    on the host (or the last function's)."""
    f = x.ravel()
    values, index, inverse, counts = np.unique(f, return_index=True, return_inverse=True, return_counts=True)
    want = {"values": values, "indices": index.astype(np.int64),
            "inverse_indices": inverse.astype(np.int64).reshape(-1), "counts": counts.astype(np.int64)}
    got = None
    for name in funcs:
        res = getattr(xp, name)(_arr(ex, x, chunks))
        fields = ("values",) if name == "unique_values" else res._fields
        res = (res,) if name == "unique_values" else tuple(res)
        got = {}
        for field, a in zip(fields, res):
            if field == "inverse_indices":
                assert a.shape == x.shape and a.chunks == _arr(ex, x, chunks).chunks, name
            else:
                assert a.shape == values.shape and a.numblocks == res[0].numblocks, (name, field)
            g = got[field] = a.compute()
            e = want[field]
            assert _same(g.reshape(-1) if field == "inverse_indices" else g, e), \
                (name, field, g.dtype, e.dtype, g.shape, e.shape, g.reshape(-1)[:8], e[:8])
        # the representative of a value is its first occurrence in C order, bit for bit
        assert got["values"].tobytes() == f[index].tobytes(), name
    return got


def _data(rng, dtype, n, distinct):
    """n values of about ``distinct`` different ones: for floats with NaNs of two
    payloads, both zeros and both infinities among them."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        pool = rng.standard_normal(max(distinct, 1)).astype(dtype)
        special = np.array([np.nan, -np.nan, -0.0, 0.0, np.inf, -np.inf], dtype=dtype)
        pool[:min(len(special), max(len(pool) - 1, 0))] = special[:min(len(special), max(len(pool) - 1, 0))]
    elif dtype.kind == "u":
        pool = rng.integers(0, np.iinfo(dtype).max, size=max(distinct, 1), dtype=dtype, endpoint=True)
    elif dtype.kind == "b":
        pool = np.array([True, False])
    else:
        info = np.iinfo(dtype)
        pool = rng.integers(info.min, info.max, size=max(distinct, 1), dtype=dtype, endpoint=True)
    return pool[rng.integers(0, len(pool), size=n)]


def _sizes(T):
    return [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5]


# ------------------------------------------------------------------ sizes around the wave and the tile


@pytest.mark.parametrize("dtype", KEY_DTYPES)
@pytest.mark.parametrize("i", range(11))
def test_sizes_in_one_chunk(ex, T, dtype, i):
    n = _sizes(T)[i]
    rng = np.random.default_rng(1000 + i)
    _check(ex, _data(rng, dtype, n, max(2, n // 3)))


@pytest.mark.parametrize("dtype", [np.bool_, np.int8, np.uint8, np.int16, np.uint16])
def test_narrow_dtypes_are_widened_and_cast_back(ex, dtype):
    rng = np.random.default_rng(5)
    got = _check(ex, _data(rng, dtype, 777, 40), chunks=(200,), funcs=FUNCS)
    assert got["values"].dtype == np.dtype(dtype)


# ------------------------------------------------------------------ chunked runs, every function


def _kinds(rng, dtype, n):
    dtype = np.dtype(dtype)
    distinct = rng.permutation(n).astype(dtype) if dtype.kind != "f" else \
        rng.permutation(n).astype(dtype) / dtype.type(4) - dtype.type(n // 8)
    return {"all distinct": distinct,
            "all equal": np.full(n, 7, dtype=dtype),
            "few values": rng.integers(0, 7, size=n).astype(dtype)}


@pytest.mark.parametrize("kind", ["all distinct", "all equal", "few values"])
@pytest.mark.parametrize("dtype", [np.float32, np.int64])
def test_every_function_on_a_chunked_1d_array(ex, dtype, kind):
    x = _kinds(np.random.default_rng(11), dtype, 4099)[kind]
    _check(ex, x, chunks=(1000,), funcs=FUNCS)


@pytest.mark.parametrize("kind", ["all distinct", "all equal", "few values"])
@pytest.mark.parametrize("dtype", [np.float64, np.uint32])
def test_every_function_on_a_chunked_2d_array(ex, dtype, kind):
    x = _kinds(np.random.default_rng(12), dtype, 37 * 46)[kind].reshape(37, 46)
    _check(ex, x, chunks=(10, 16), funcs=FUNCS)


def test_zero_d_and_one_element(ex):
    _check(ex, np.array(3.5, dtype=np.float32), chunks=(), funcs=FUNCS)
    _check(ex, np.array([np.nan], dtype=np.float64), funcs=FUNCS)
    _check(ex, np.array([[-0.0]], dtype=np.float32), funcs=FUNCS)


# ------------------------------------------------------------------ seams, built by hand


def test_a_run_spanning_three_chunks(ex):
    # sorted already, so the sorted array is x itself: the run of 2.0 covers
    # chunk 1 whole, which has no head
    x = np.array([1.0] * 3 + [2.0] * 20 + [3.0] * 5, dtype=np.float32)
    got = _check(ex, x, chunks=(8,), funcs=FUNCS)
    assert got["counts"].tolist() == [3, 20, 5]
    per_chunk = ops.unique_count(_arr(ex, x, (8,))).compute()
    assert per_chunk.tolist() == [2, 0, 1, 0]                      # heads at 0, 3 and 23


def test_a_head_at_a_chunks_first_element(ex):
    x = np.array([1] * 8 + [2] * 8 + [3] * 4 + [4] * 4 + [4] * 3, dtype=np.int32)
    _check(ex, x, chunks=(8,), funcs=FUNCS)
    assert ops.unique_count(_arr(ex, x, (8,))).compute().tolist() == [1, 1, 2, 0]
    # in any order of the input too
    _check(ex, np.random.default_rng(3).permutation(x), chunks=(8,), funcs=FUNCS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nans_straddling_a_seam(ex, dtype):
    qnan = np.array([np.nan], dtype=dtype)
    other = -qnan                                                   # another bit pattern
    x = np.concatenate([np.arange(5, dtype=dtype), qnan, other, qnan, other, other, qnan])   # NaNs at 5..10
    got = _check(ex, x, chunks=(8,), funcs=FUNCS)
    assert got["counts"].tolist() == [1] * 5 + [6] and np.isnan(got["values"][-1])
    assert ops.unique_count(_arr(ex, x, (8,))).compute().tolist() == [6, 0]
    y = np.random.default_rng(4).permutation(np.concatenate([x, x]))
    _check(ex, y, chunks=(8,), funcs=FUNCS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("first", [-0.0, 0.0])
def test_zeros_straddling_a_seam(ex, dtype, first):
    zeros = np.array([first, -first, -0.0, 0.0, 0.0, -0.0], dtype=dtype)
    x = np.concatenate([np.array([-3, -2, -1, -1, -1], dtype=dtype), zeros, np.array([1, 2], dtype=dtype)])
    got = _check(ex, x, chunks=(8,), funcs=FUNCS)                  # zeros at 5..10, the seam at 8
    (z,) = np.flatnonzero(got["values"] == 0)
    assert np.signbit(got["values"][z]) == np.signbit(dtype(first))
    # unsorted: the first zero in C order decides
    y = np.concatenate([x[8:], x[:8]])
    got = _check(ex, y, chunks=(8,), funcs=FUNCS)
    (z,) = np.flatnonzero(got["values"] == 0)
    first_zero = y[np.flatnonzero(y == 0)[0]]
    assert np.signbit(got["values"][z]) == np.signbit(first_zero)
    assert got["indices"][z] == np.flatnonzero(y == 0)[0]


# ------------------------------------------------------------------ the gather


def test_every_chunk_contributes_one_value(ex):
    c, nb = 4, 37
    x = np.repeat(np.arange(nb, dtype=np.int64), c)               # k = 37 > c: four pieces per output chunk
    got = _check(ex, x, chunks=(c,), funcs=FUNCS)
    assert got["counts"].tolist() == [c] * nb
    assert ops.unique_count(_arr(ex, x, (c,))).compute().tolist() == [1] * nb


def test_pieces_straddle_output_chunks(ex):
    rng = np.random.default_rng(9)
    # k > c with uneven heads per chunk, some chunks with none
    x = np.sort(np.concatenate([np.full(40, 5.0), rng.standard_normal(50), np.full(33, 9.0),
                                rng.standard_normal(20) + 20])).astype(np.float32)
    _check(ex, x, chunks=(16,), funcs=FUNCS)
    _check(ex, rng.permutation(x), chunks=(16,), funcs=FUNCS)


# ------------------------------------------------------------------ the kernel's own outputs


@pytest.mark.parametrize("dtype", [np.float32, np.uint64])
def test_pack_fills_the_front_and_zeroes_the_tail(ex, T, dtype):
    c = T + 7
    x = np.sort(_data(np.random.default_rng(21), dtype, 3 * c - 11, 900))
    s = _arr(ex, x, (c,))
    counts = ops.unique_count(s).compute()
    keys = ops.unique_pack(s).compute()
    pos = ops.unique_pack(s, False, "position").compute()
    head = np.ones(len(x), dtype=bool)
    head[1:] = ~((x[1:] == x[:-1]) | ((x[1:] != x[1:]) & (x[:-1] != x[:-1])))
    for b in range(3):
        lo, hi = b * c, min((b + 1) * c, len(x))
        at = lo + np.flatnonzero(head[lo:hi])
        assert counts[b] == len(at)
        want = np.zeros(hi - lo, dtype=x.dtype)
        want[:len(at)] = x[at]
        assert keys[lo:hi].tobytes() == want.tobytes()
        assert pos["v"][lo:hi].tobytes() == want.tobytes()
        want_i = np.zeros(hi - lo, dtype=np.int64)
        want_i[:len(at)] = at
        assert np.array_equal(pos["i"][lo:hi], want_i)


# ------------------------------------------------------------------ phase 2 starts from HBM; reruns


def test_the_results_plan_does_not_sort_again(ex):
    x = _data(np.random.default_rng(31), np.float32, 3000, 500)
    for name in FUNCS:
        res = getattr(xp, name)(_arr(ex, x, (700,)))
        for a in ((res,) if name == "unique_values" else tuple(res)):
            progs = [d["pipeline"].config.function for _, d in a.plan.dag.nodes(data=True)
                     if d.get("pipeline") is not None and d["pipeline"].function is apply_blockwise]
            assert progs and not [p for p in progs if isinstance(p, (ir.SortProgram, ir.UniqueProgram))], name
    v = xp.unique_values(_arr(ex, x, (700,)))
    assert _same(v.compute(), np.unique(x)) and _same(v.compute(), np.unique(x))   # and can be computed twice


def test_two_runs_are_bit_identical(ex, T):
    x = _data(np.random.default_rng(41), np.float64, 3 * T + 5, 2000)
    runs = []
    for _ in range(2):
        res = xp.unique_all(_arr(ex, x, (T + 1,)))
        runs.append([a.compute().tobytes() for a in (res.values, res.indices, res.counts)])
    assert runs[0] == runs[1]
