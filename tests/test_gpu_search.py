"""searchsorted on the MI355X executor (``-m gpu``) against numpy.

Parity is UNPINNED against the reference: cubed v0.12.0 has no searchsorted.
``x1`` ascends in the order of ``xp.sort``, which is the order
``np.searchsorted`` uses as well: every NaN after every number and all NaNs
tied, -0.0 and 0.0 tied.  Every comparison is exact (int64 indices; only key
comparisons decide them, so no tolerance enters)."""

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
def T(built):
    return nat.search_tile()


def _arr(ex, x, chunks, mem="2GB"):
    spec = cubed.Spec(allowed_mem=mem, reserved_mem=0, executor=ex)
    return cubed.from_array(x, chunks=chunks, spec=spec)


def _check(ex, x1, x2, chunks1=None, chunks2=None, sides=("left", "right")):
    chunks1 = x1.shape if chunks1 is None else chunks1
    chunks2 = x2.shape if chunks2 is None else chunks2
    for side in sides:
        got = xp.searchsorted(_arr(ex, x1, chunks1), _arr(ex, x2, chunks2), side=side).compute()
        exp = np.searchsorted(x1, x2, side=side)
        assert got.dtype == np.int64 and got.shape == x2.shape
        assert np.array_equal(got, exp), (side, np.flatnonzero((got != exp).ravel())[:5])


def _sorted(rng, n, dtype, spread=50):
    """n sorted keys with many duplicates: eighths for floats; multiples of
    2^33 for int64, so that the high words decide."""
    if np.dtype(dtype).kind == "f":
        return np.sort((rng.integers(-spread, spread, size=n) / 8).astype(dtype))
    unit = 2 ** 33 if np.dtype(dtype) == np.int64 else 1
    return np.sort(rng.integers(-spread, spread, size=n).astype(dtype) * np.dtype(dtype).type(unit))


def _values(rng, x1, m):
    """m values: x1's own, values between them, below all and above all."""
    if x1.dtype.kind == "f":
        half, out = x1.dtype.type(1 / 16), x1.dtype.type(1000)
    else:
        half = x1.dtype.type(2 ** 32 if x1.dtype == np.int64 else 0)
        out = x1.dtype.type(2 ** 40 if x1.dtype == np.int64 else 1000)
    pool = np.concatenate([x1, x1 + half, x1 - half, [x1[0] - out, x1[-1] + out]]).astype(x1.dtype)
    v = pool[rng.integers(0, len(pool), size=m)]
    if m >= 4:
        v[:4] = [x1[0] - out, x1[-1] + out, x1[0], x1[-1]]
    return v


def _n_sorted(T):
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]


# ------------------------------------------------------------------ 1-d, one chunk of each


@pytest.mark.parametrize("dtype", [np.float32, np.int64])
@pytest.mark.parametrize("i", range(9))
def test_sorted_sizes_around_the_tile(ex, T, dtype, i):
    n = _n_sorted(T)[i]
    rng = np.random.default_rng(200 + i)
    x1 = _sorted(rng, n, dtype)
    _check(ex, x1, _values(rng, x1, 1000))


@pytest.mark.parametrize("dtype", [np.float32, np.int64])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 4099])
def test_value_counts_around_the_lane_steps(ex, T, dtype, m):
    rng = np.random.default_rng(300 + m)
    for n in (T, T + 1):
        x1 = _sorted(rng, n, dtype, spread=400)
        _check(ex, x1, _values(rng, x1, m))


# ------------------------------------------------------------------ split-path boundaries


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.uint64])
def test_all_equal_sorted_chunk(ex, T, dtype):
    n = 3 * T + 5
    x1 = np.full(n, 7, dtype=dtype)
    x2 = np.array([7, 6, 8, 7], dtype=dtype)
    for side, want in (("left", [0, 0, n, 0]), ("right", [n, 0, n, n])):
        got = xp.searchsorted(_arr(ex, x1, (n,)), _arr(ex, x2, (4,)), side=side).compute()
        assert got.tolist() == want == np.searchsorted(x1, x2, side=side).tolist()


def _neighbours(v, dtype):
    if np.dtype(dtype).kind == "f":
        v = np.dtype(dtype).type(v)
        return [np.nextafter(v, -np.inf, dtype=dtype), v, np.nextafter(v, np.inf, dtype=dtype)]
    return [v - 1, v, v + 1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int64])
def test_duplicate_runs_across_the_splitters(ex, T, dtype):
    n = 3 * T + 5  # stride 4: splitters at 3, 7, 11, ...
    # one run that covers every splitter position
    x1 = np.full(n, 2.5 if np.dtype(dtype).kind == "f" else 2 ** 40, dtype=dtype)
    x1[:2] = x1[0] - 3
    x1[-2:] = x1[-3] + 3
    x2 = np.array(_neighbours(x1[5], dtype) + _neighbours(x1[0], dtype) + _neighbours(x1[-1], dtype), dtype=dtype)
    _check(ex, x1, x2)
    # runs of 6 and of 5: their ends fall on every position relative to a splitter
    for run in (6, 5):
        x1 = (np.arange(n) // run).astype(dtype)
        vals = np.unique(x1)[:: 7]
        x2 = np.array([w for v in vals for w in _neighbours(v, dtype)], dtype=dtype)
        _check(ex, x1, x2)
    # a longer chunk: stride 1025, the last bucket short
    n = 1025 * T - 1000
    x1 = (np.arange(n) // 700).astype(dtype)
    x2 = np.array([w for v in np.unique(x1)[:: 41] for w in _neighbours(v, dtype)] + [x1[-1]], dtype=dtype)
    _check(ex, x1, x2)


# ------------------------------------------------------------------ floats


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_inf_and_signed_zeros(ex, T, dtype):
    rng = np.random.default_rng(21)
    special = np.array([-np.inf] * 3 + [np.inf] * 3 + [-0.0, 0.0] * 4 + [np.nan] * 6, dtype=dtype)
    # a NaN with the sign bit set and another payload than numpy's
    odd = np.array([-3], dtype=f"i{np.dtype(dtype).itemsize}").view(dtype)
    assert np.isnan(odd[0]) and np.signbit(odd[0])
    x2 = np.array([np.nan, odd[0], 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 0.125, -0.125, 1e30, -1e30], dtype=dtype)
    small = np.array([-np.inf, -0.0, 0.0, 1, 1, 1, np.inf, np.nan, np.nan], dtype=dtype)
    assert np.searchsorted(small, x2[:4], side="left").tolist() == [7, 7, 1, 1]
    assert np.searchsorted(small, x2[:4], side="right").tolist() == [9, 9, 3, 3]
    _check(ex, small, x2)
    for n in (T, 3 * T + 5):  # both paths
        body = (rng.integers(-20, 20, size=n - len(special) - 1) / 8).astype(dtype)
        x1 = np.sort(np.concatenate([body, special, odd]))
        assert len(x1) == n and np.isnan(x1[-7:]).all()
        _check(ex, x1, x2)
        _check(ex, x1, x1[rng.integers(0, n, size=500)])
    allnan = np.full(T + 9, np.nan, dtype=dtype)
    _check(ex, allnan, x2)


# ------------------------------------------------------------------ integers, dtypes


def test_uint64_on_both_sides_of_2_63(ex, T):
    rng = np.random.default_rng(22)
    for n in (3000, 3 * T + 5):
        x1 = rng.integers(2 ** 63 - 5, 2 ** 63 + 5, size=n, dtype=np.uint64)
        x1[::7] = np.iinfo(np.uint64).max
        x1[3::11] = 0
        x1 = np.sort(x1)
        x2 = np.concatenate([np.arange(2 ** 63 - 7, 2 ** 63 + 7, dtype=np.uint64),
                             np.array([0, 1, np.iinfo(np.uint64).max, np.iinfo(np.uint64).max - 1], dtype=np.uint64)])
        _check(ex, x1, x2)


def test_uint32_on_both_sides_of_2_31(ex, T):
    rng = np.random.default_rng(23)
    for n in (3000, 3 * T + 5):
        x1 = rng.integers(2 ** 31 - 3, 2 ** 31 + 3, size=n).astype(np.uint32)
        x1[::5] = np.iinfo(np.uint32).max
        x1 = np.sort(x1)
        x2 = np.concatenate([np.arange(2 ** 31 - 5, 2 ** 31 + 5).astype(np.uint32),
                             np.array([0, np.iinfo(np.uint32).max], dtype=np.uint32)])
        _check(ex, x1, x2)


def test_int64_extremes(ex):
    i64 = np.iinfo(np.int64)
    pool = np.array([i64.min, i64.min + 1, -1, 0, 1, i64.max - 1, i64.max], dtype=np.int64)
    x1 = np.sort(pool[np.random.default_rng(24).integers(0, len(pool), size=5000)])
    _check(ex, x1, pool)
    _check(ex, x1, pool, chunks1=(1200,))


def test_narrow_and_mixed_dtypes(ex):
    rng = np.random.default_rng(25)
    b1 = np.sort(rng.integers(0, 2, size=300).astype(np.bool_))
    _check(ex, b1, np.array([False, True, True, False]), chunks1=(128,))
    _check(ex, np.zeros(5, dtype=np.bool_), np.array([False, True]))
    i8 = np.sort(rng.integers(-128, 128, size=300).astype(np.int8))
    _check(ex, i8, np.array([-2 ** 40, -129, -128, -1, 0, 1, 127, 128, 2 ** 40] + i8[::9].tolist(), dtype=np.int64),
           chunks1=(128,))
    u8 = np.sort(rng.integers(0, 256, size=300).astype(np.uint8))
    _check(ex, u8, np.arange(-128, 128).astype(np.int8), chunks1=(128,))   # 200 stays above -56
    _check(ex, np.sort(np.arange(-128, 128).astype(np.int8)), u8[::3])     # and the other way round
    f32 = np.sort((rng.integers(-50, 50, size=300) / 8).astype(np.float32))
    f64 = np.concatenate([f32.astype(np.float64) + 1e-12, f32.astype(np.float64) - 1e-12, f32.astype(np.float64)])
    _check(ex, f32, f64)  # values float32 cannot hold: the search runs in float64
    third = np.float32(1) / np.float32(3)
    _check(ex, np.array([0, third, third, 1], dtype=np.float32), np.array([1 / 3, float(third)]))


# ------------------------------------------------------------------ several blocks of x1


@pytest.mark.parametrize("n,chunk", [(10_000, 1024), (10_000, 3000), (50, 7)])
def test_several_blocks_of_the_sorted_array(ex, n, chunk):
    rng = np.random.default_rng(n + chunk)
    for dtype, spread in ((np.float32, 20), (np.int64, 3)):
        x1 = _sorted(rng, n, dtype, spread=spread)
        # a run of duplicates spans a block boundary
        assert any(x1[b - 1] == x1[b] for b in range(chunk, n, chunk))
        x2 = _values(rng, x1, 1000)
        _check(ex, x1, x2, chunks1=(chunk,), chunks2=(300,))


# ------------------------------------------------------------------ N-d and 0-d values


def test_3d_values_edge_chunks_and_0d(ex):
    rng = np.random.default_rng(27)
    x1 = np.sort(rng.integers(-5, 6, size=40).astype(np.int32))
    x2 = rng.integers(-7, 8, size=(37, 5, 46)).astype(np.int32)
    _check(ex, x1, x2, chunks1=(16,), chunks2=(10, 2, 16))
    for v in (-9, 0, 3, 99):
        _check(ex, x1, np.array(v, dtype=np.int32), chunks1=(16,), chunks2=())


# ------------------------------------------------------------------ sorter


def test_sorter(ex):
    rng = np.random.default_rng(28)
    x1 = (rng.integers(-30, 30, size=3000) / 8).astype(np.float32)
    sorter = np.argsort(x1, kind="stable")
    x2 = _values(rng, np.sort(x1), 500)
    for side in ("left", "right"):
        got = xp.searchsorted(_arr(ex, x1, (1000,)), _arr(ex, x2, (200,)), side=side,
                              sorter=_arr(ex, sorter, (1000,))).compute()
        assert np.array_equal(got, np.searchsorted(x1, x2, side=side, sorter=sorter))


# ------------------------------------------------------------------ composition, determinism


def test_with_sort_in_one_plan_twice(ex):
    a = (np.random.default_rng(29).integers(-300, 300, size=5000) / 8).astype(np.float32)
    x = _arr(ex, a, (1024,))
    y = xp.searchsorted(xp.sort(x), x, side="left")
    first = y.compute()
    assert np.array_equal(first, np.searchsorted(np.sort(a), a))
    assert first.tobytes() == y.compute().tobytes()
    x = _arr(ex, a, (1024,))
    assert first.tobytes() == xp.searchsorted(xp.sort(x), x, side="left").compute().tobytes()


def test_elementwise_producer_and_consumer(ex):
    rng = np.random.default_rng(30)
    x1 = np.sort(rng.integers(-20, 20, size=500).astype(np.float64))
    x2 = rng.integers(-25, 25, size=(60, 44)).astype(np.float64)
    got = (xp.searchsorted(_arr(ex, x1, (128,)) * 2.0, _arr(ex, x2, (16, 44)) + 1.0, side="right") + 1).compute()
    assert np.array_equal(got, np.searchsorted(x1 * 2.0, x2 + 1.0, side="right") + 1)


# ------------------------------------------------------------------ zero sizes


def test_zero_sizes(ex):
    x1 = np.sort(np.random.default_rng(31).standard_normal(100).astype(np.float32))
    x2 = np.ones((6, 4), dtype=np.float32)
    got = xp.searchsorted(_arr(ex, np.zeros(0, dtype=np.float32), (1,)), _arr(ex, x2, (4, 4))).compute()
    assert got.dtype == np.int64 and np.array_equal(got, np.zeros((6, 4), dtype=np.int64))
    got = xp.searchsorted(_arr(ex, x1, (30,)), _arr(ex, np.zeros((3, 0), dtype=np.float32), (1, 1))).compute()
    assert got.shape == (3, 0) and got.dtype == np.int64
