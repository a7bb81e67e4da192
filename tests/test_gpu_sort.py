"""sort / argsort on the MI355X executor (``-m gpu``) against numpy.

Parity is UNPINNED against the reference: cubed v0.12.0 has neither function.
The order is numpy's stable sort: values ascend, every NaN is greater than
every number and all NaNs tie, -0.0 and 0.0 tie, ties go to the smaller index
along the axis.  ``descending=True`` reverses the value order (NaNs first);
ties still go to the smaller index.  So, exactly,

    argsort ascending   np.argsort(x, axis, kind="stable")
    argsort descending  n - 1 - flip(np.argsort(flip(x, axis), axis, kind="stable"), axis)
    sort                np.take_along_axis(x, expected argsort, axis), compared
                        with equal_nan (which zero sign or NaN payload lands
                        where within a tie is unspecified)
"""

import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
from cubed_amd import _native as nat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex(gpu_executor):
    return gpu_executor


@pytest.fixture(scope="module")
def tile(built):
    return nat.sort_tile()


def _arr(ex, x, chunks, mem="2GB"):
    spec = cubed.Spec(allowed_mem=mem, reserved_mem=0, executor=ex)
    return cubed.from_array(x, chunks=chunks, spec=spec)


def expected_argsort(x, axis, descending):
    if not descending:
        return np.argsort(x, axis=axis, kind="stable")
    n = x.shape[axis]
    return n - 1 - np.flip(np.argsort(np.flip(x, axis), axis=axis, kind="stable"), axis)


def _check(ex, x, chunks, axis=-1, descending=False, which=("argsort", "sort")):
    order = expected_argsort(x, axis, descending)
    if "argsort" in which:
        got = xp.argsort(_arr(ex, x, chunks), axis=axis, descending=descending).compute()
        assert got.dtype == np.int64 and got.shape == x.shape
        assert np.array_equal(got, order)
    if "sort" in which:
        got = xp.sort(_arr(ex, x, chunks), axis=axis, descending=descending).compute()
        assert got.dtype == x.dtype and got.shape == x.shape
        exp = np.take_along_axis(x, order, axis)
        assert np.array_equal(got, exp, equal_nan=x.dtype.kind == "f")


def _sizes(tile):
    return [1, 2, 3, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 5, 70_001]


def _data(rng, n, dtype):
    if np.dtype(dtype).kind == "f":
        # eighths: plenty of duplicates for the index order to matter
        return (np.round(rng.standard_normal(n) * 8) / 8).astype(dtype)
    # int64: multiples of 2^33, so the high words decide
    return rng.integers(-50, 50, size=n).astype(dtype) * np.dtype(dtype).type(2 ** 33 if dtype == np.int64 else 1)


# ------------------------------------------------------------------ 1-d, one chunk


def test_single_chunk_sizes_cover_both_pass_parities(tile):
    passes = []
    for n in _sizes(tile):
        rows = np.zeros(1, dtype=nat.SORT_TASK_DTYPE)
        rows[0]["src_base"], rows[0]["dst_base"] = 1 << 20, 1 << 30
        rows[0]["rows"], rows[0]["n"] = 1, n
        rows[0]["src_row_stride"] = rows[0]["dst_row_stride"] = n
        passes.append(nat.sort_plan(rows, 4, False)[0])  # CUBED_I64
    assert passes[:9] == [0] * 8 + [1]
    assert passes[9] == 2 and passes[10] == int(np.ceil(np.log2(np.ceil(70_001 / tile))))
    assert {p % 2 for p in passes if p} == {0, 1}


@pytest.mark.parametrize("dtype", [np.int64, np.float32])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("i", range(11))
def test_1d_single_chunk(ex, tile, dtype, descending, i):
    n = _sizes(tile)[i]
    x = _data(np.random.default_rng(100 + i), n, dtype)
    _check(ex, x, (n,), descending=descending)


# ------------------------------------------------------------------ 1-d, several chunks


@pytest.mark.parametrize("n,chunk", [(10_000, 1024), (10_000, 3000), (50, 7)])
@pytest.mark.parametrize("descending", [False, True])
def test_1d_several_chunks(ex, n, chunk, descending):
    rng = np.random.default_rng(n + chunk)
    _check(ex, _data(rng, n, np.float32), (chunk,), descending=descending)
    _check(ex, _data(rng, n, np.int64), (chunk,), descending=descending)


# ------------------------------------------------------------------ 3-d


@pytest.fixture(scope="module")
def x3():
    return np.random.default_rng(7).integers(-5, 6, size=(37, 5, 46), dtype=np.int32)


@pytest.mark.parametrize("axis", [0, 1, 2, -1])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("which", ["sort", "argsort"])
def test_int32_3d_edge_chunks(ex, x3, axis, descending, which):
    _check(ex, x3, (10, 2, 16), axis=axis, descending=descending, which=(which,))


# ------------------------------------------------------------------ stability


def test_all_equal_row_in_one_chunk_keeps_its_order(ex, tile):
    n = 3 * tile + 5
    x = np.full((2, n), 3.5, dtype=np.float32)
    for descending in (False, True):
        got = xp.argsort(_arr(ex, x, (2, n)), axis=1, descending=descending).compute()
        assert np.array_equal(got, np.broadcast_to(np.arange(n), (2, n)))


def test_all_equal_array_over_ragged_blocks_keeps_its_order(ex):
    # fails if the block merges compare keys only, not (key, index)
    n = 5 * 1000 - 300
    x = np.full(n, 7, dtype=np.int64)
    for descending in (False, True):
        got = xp.argsort(_arr(ex, x, (1000,)), descending=descending).compute()
        assert np.array_equal(got, np.arange(n))


# ------------------------------------------------------------------ special floats


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("descending", [False, True])
def test_nan_inf_and_signed_zeros(ex, tile, dtype, descending):
    rng = np.random.default_rng(11)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0], dtype=dtype)
    # a NaN with the sign bit set and another payload than numpy's
    odd = np.array([-3], dtype=f"i{np.dtype(dtype).itemsize}").view(dtype)
    assert np.isnan(odd[0]) and np.signbit(odd[0])
    pool = np.concatenate([special, odd])
    n = 2 * tile + 77
    x = pool[rng.integers(0, len(pool), size=n)]
    _check(ex, x, (n,), descending=descending)          # one chunk, merge passes
    _check(ex, x, (tile // 2 + 3,), descending=descending)  # 4 ragged blocks
    x2 = pool[rng.integers(0, len(pool), size=(9, 40))]
    _check(ex, x2, (4, 16), axis=0, descending=descending)
    _check(ex, x2, (4, 16), axis=1, descending=descending)


# ------------------------------------------------------------------ integers, dtypes


@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.bool_])
def test_narrow_dtypes_round_trip(ex, dtype):
    rng = np.random.default_rng(12)
    if dtype == np.bool_:
        x = rng.integers(0, 2, size=(6, 300)).astype(np.bool_)
    else:
        info = np.iinfo(dtype)
        x = rng.integers(info.min, info.max + 1, size=(6, 300)).astype(dtype)
    for descending in (False, True):
        _check(ex, x, (4, 128), axis=1, descending=descending)


def test_uint64_above_2_63(ex):
    rng = np.random.default_rng(13)
    x = rng.integers(2 ** 63 - 5, 2 ** 63 + 5, size=3000, dtype=np.uint64)
    x[::7] = np.iinfo(np.uint64).max
    x[3::11] = 0
    for descending in (False, True):
        _check(ex, x, (1000,), descending=descending)


def test_uint32_and_int64_extremes(ex):
    rng = np.random.default_rng(14)
    i64 = np.iinfo(np.int64)
    pool = np.array([i64.min, i64.min + 1, -1, 0, 1, i64.max - 1, i64.max], dtype=np.int64)
    x = pool[rng.integers(0, len(pool), size=5000)]
    u = rng.integers(2 ** 31 - 3, 2 ** 31 + 3, size=5000).astype(np.uint32)
    u[::5] = np.iinfo(np.uint32).max
    for descending in (False, True):
        _check(ex, x, (5000,), descending=descending)
        _check(ex, x, (1200,), descending=descending)
        _check(ex, u, (1200,), descending=descending)


@pytest.mark.parametrize("descending", [False, True])
def test_float64(ex, descending):
    x = np.round(np.random.default_rng(15).standard_normal((5, 7000)) * 4) / 4
    _check(ex, x, (5, 7000), axis=1, descending=descending)
    _check(ex, x, (2, 2500), axis=1, descending=descending)
    _check(ex, x, (2, 2500), axis=0, descending=descending)


def test_many_short_rows_share_a_workgroup(ex):
    x = np.random.default_rng(16).integers(-3, 4, size=(1000, 10)).astype(np.float32)
    _check(ex, x, (1000, 10), axis=1)
    _check(ex, x, (300, 10), axis=1, descending=True)


# ------------------------------------------------------------------ determinism, composition


def test_same_plan_twice_is_bit_identical(ex):
    x = np.round(np.random.default_rng(17).standard_normal(20_000) * 4).astype(np.float32)
    x[::13] = -0.0
    x[5::17] = np.nan
    for f in (xp.sort, xp.argsort):
        y = f(_arr(ex, x, (3000,)))
        first = y.compute()
        second = y.compute()
        assert first.tobytes() == second.tobytes()
        assert first.tobytes() == f(_arr(ex, x, (3000,))).compute().tobytes()


def test_elementwise_producer_and_consumer(ex):
    x = np.random.default_rng(18).integers(-20, 20, size=(60, 44)).astype(np.float64)
    a = _arr(ex, x, (16, 44))
    got = (xp.sort(a * 2.0, axis=0) + 1.0).compute()
    assert np.array_equal(got, np.sort(x * 2.0, axis=0) + 1.0)
    got = xp.sort(a.rechunk((60, 11)), axis=0).compute()
    assert np.array_equal(got, np.sort(x, axis=0))
