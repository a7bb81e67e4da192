"""histogram on the MI355X executor (``-m gpu``) against numpy.

Parity is UNPINNED against the reference: cubed v0.12.0 has no histogram.
``np.histogram`` on the same data is the yardstick, for the counts and for the
edges.  Every comparison is exact: the counts are integers that only
comparisons with the edges decide, and the edges are numpy's own."""

import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
from cubed_amd import _native as nat

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 3.0  # 0.0 is an edge for every power-of-two bin count from 4 on


@pytest.fixture(scope="module")
def ex(gpu_executor):
    return gpu_executor


@pytest.fixture(scope="module")
def L(built):
    return nat.hist_bins_lds()


def _arr(ex, x, chunks=None, mem="2GB"):
    spec = cubed.Spec(allowed_mem=mem, reserved_mem=0, executor=ex)
    return cubed.from_array(x, chunks=x.shape if chunks is None else chunks, spec=spec)


def _check(ex, x, bins, range=None, chunks=None):
    """Counts and edges of xp.histogram equal np.histogram's; returns the counts."""
    hist, edges = xp.histogram(_arr(ex, x, chunks), bins, range=range)
    got, got_e = hist.compute(), edges.compute()
    # numpy counts bool as uint8 too, with a warning
    exp, exp_e = np.histogram(x.view(np.uint8) if x.dtype == np.bool_ else x, bins, range=range)
    assert got.dtype == np.int64 and got.shape == exp.shape and hist.numblocks == (1,)
    assert got_e.dtype == exp_e.dtype and np.array_equal(got_e, exp_e)
    assert np.array_equal(got, exp), (np.flatnonzero(got != exp)[:5], got[got != exp][:5], exp[got != exp][:5])
    return got


def _adversarial(rng, dtype, nbins, n=20000, lo=LO, hi=HI):
    """n values drawn uniformly from one unit beyond the range on both sides,
    and every edge, its two neighbours, NaN, the infinities and both zeros."""
    e = np.histogram_bin_edges(np.empty(0, dtype), nbins, (lo, hi))
    assert e.dtype == np.dtype(dtype)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dtype=dtype)
    x = np.concatenate([rng.uniform(lo - 1, hi + 1, size=n).astype(dtype), e,
                        np.nextafter(e, dtype(-np.inf)), np.nextafter(e, dtype(np.inf)), special])
    assert x.dtype == np.dtype(dtype)
    return rng.permutation(x)


def _nbins(L):
    return [1, 2, 63, 64, 65, L - 1, L, L + 1, 3 * L + 5, 100000]


# ------------------------------------------------------------------ bin counts around the paths


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("i", range(10))
def test_bin_counts_with_adversarial_values(ex, L, dtype, i):
    nbins = _nbins(L)[i]
    x = _adversarial(np.random.default_rng(100 + i), dtype, nbins)
    got = _check(ex, x, nbins, (LO, HI))
    assert got.sum() < x.size  # NaN, the infinities and the values beyond the range are dropped


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_sizes_of_x(ex, L, dtype, n):
    rng = np.random.default_rng(200 + n)
    for nbins in (10, L + 1):
        x = _adversarial(rng, dtype, nbins)[:n]
        _check(ex, x, nbins, (LO, HI))
        _check(ex, x, np.histogram_bin_edges(x[:0], nbins, (LO, HI)))


# ------------------------------------------------------------------ explicit edges


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_explicit_edges_with_duplicates(ex, L, dtype):
    rng = np.random.default_rng(300)
    edges = np.array([-1.0, -0.5, 0.0, 0.0, 0.125, 1.0, 1.0, 1.0, 2.5, 3.0, 3.0], dtype=dtype)  # interior and last
    x = np.concatenate([_adversarial(rng, dtype, 8), edges, np.nextafter(edges, dtype(-np.inf)),
                        np.nextafter(edges, dtype(np.inf))])
    got = _check(ex, x, edges)
    assert got[2] == 0 and got[5] == 0 and got[6] == 0 and got[9] > 0  # zero-width bins: only the last counts
    # many non-uniform edges: the LDS search and, past L, the search in global memory
    for nb in (1000, L + 1):
        e = np.sort(rng.uniform(LO, HI, size=nb + 1).astype(dtype))
        e[nb // 2] = e[nb // 2 - 1]
        x = np.concatenate([_adversarial(rng, dtype, 8), e, np.nextafter(e, dtype(-np.inf)),
                            np.nextafter(e, dtype(np.inf))])
        _check(ex, x, e)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_linspace_edges_passed_back(ex, L, dtype):
    for i, nbins in enumerate((7, 100, L, L + 1)):
        x = _adversarial(np.random.default_rng(400 + i), dtype, nbins)
        by_int = _check(ex, x, nbins, (LO, HI))
        by_edges = _check(ex, x, np.histogram_bin_edges(x[:0], nbins, (LO, HI)))
        assert np.array_equal(by_int, by_edges)


def test_float32_values_with_float64_edges_and_the_reverse(ex):
    rng = np.random.default_rng(450)
    x32 = _adversarial(rng, np.float32, 8)
    e64 = np.array([-1.0, -1 / 3, 0.1, 0.7, 3.0])
    _check(ex, x32, e64)
    _check(ex, x32.astype(np.float64) + 1e-9, e64.astype(np.float32))


# ------------------------------------------------------------------ integer and bool input


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.uint8, np.bool_])
def test_integer_and_bool_input(ex, dtype):
    rng = np.random.default_rng(500)
    if dtype is np.bool_:
        x, lo, hi = rng.integers(0, 2, size=5003).astype(dtype), 0, 1
    elif dtype is np.uint8:
        x, lo, hi = rng.integers(0, 256, size=5003).astype(dtype), 10, 200
    elif dtype is np.int64:
        # within +-2^52 the conversion to float64 is exact, so this pins the kernel, not the rounding
        lo, hi = -2 ** 52, 2 ** 52
        x = np.concatenate([rng.integers(lo, hi, size=5000), [lo, hi, lo + 1, hi - 1, 0]]).astype(dtype)
        lo, hi = -2 ** 51, 2 ** 52
    else:
        x, lo, hi = rng.integers(-1000, 1000, size=5003).astype(dtype), -500, 700
    for bins in (1, 2, 7, 100):
        _check(ex, x, bins, (lo, hi), chunks=(1024,))
    _check(ex, x, [lo, lo + (hi - lo) // 3, hi], chunks=(1024,))  # integer edges stay integer, as numpy's


# ------------------------------------------------------------------ contention


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_value_in_one_bin(ex, L, dtype):
    n = 200000
    for nbins in (100, L + 1):
        e = np.histogram_bin_edges(np.empty(0, dtype), nbins, (LO, HI))
        inside = _check(ex, np.full(n, e[37] + (e[38] - e[37]) / 4, dtype=dtype), nbins, (LO, HI))
        assert inside[37] == n and inside.sum() == n
        last = _check(ex, np.full(n, e[-1], dtype=dtype), nbins, (LO, HI))
        assert last[-1] == n and last.sum() == n
        for out in (np.nextafter(e[-1], dtype(np.inf)), np.nextafter(e[0], dtype(-np.inf))):
            assert not _check(ex, np.full(n, out, dtype=dtype), nbins, (LO, HI)).any()


def test_runs_of_equal_bins_inside_a_wave(ex):
    # runs of every length from 1 to 130 values, so that runs start and end at every lane
    x = np.concatenate([np.full(k, (k % 10) / 2.5 - 0.9, dtype=np.float32) for k in range(1, 131)])
    _check(ex, x, 10, (LO, HI))
    _check(ex, x, np.histogram_bin_edges(x[:0], 10, (LO, HI)))


# ------------------------------------------------------------------ n-d, several chunks


def test_nd_ragged_chunks_lazy_producer_and_density(ex):
    rng = np.random.default_rng(600)
    shape, chunks = (37, 300, 41), (16, 128, 41)
    a = rng.uniform(-2, 2, size=shape).astype(np.float32)
    b = rng.uniform(-2, 2, size=shape).astype(np.float32)
    _check(ex, a, 50, (LO, HI), chunks=chunks)
    _check(ex, a.astype(np.float64), 50, (LO, HI), chunks=chunks)
    hist, edges = xp.histogram(_arr(ex, a, chunks) * _arr(ex, b, chunks), 33, range=(LO, HI))
    exp, exp_e = np.histogram(a * b, 33, range=(LO, HI))
    assert np.array_equal(hist.compute(), exp) and np.array_equal(edges.compute(), exp_e)
    dens, edges = xp.histogram(_arr(ex, a, chunks), 50, range=(LO, HI), density=True)
    exp, exp_e = np.histogram(a, 50, range=(LO, HI), density=True)
    got = dens.compute()
    assert got.dtype == np.float64 and np.array_equal(edges.compute(), exp_e)
    np.testing.assert_allclose(got, exp, rtol=1e-15, atol=0)


def test_zero_d_and_empty(ex):
    spec = cubed.Spec(allowed_mem="2GB", reserved_mem=0, executor=ex)
    hist, _ = xp.histogram(xp.asarray(0.5, spec=spec), 4, range=(0, 1))
    assert hist.compute().tolist() == [0, 0, 1, 0]
    hist, edges = xp.histogram(_arr(ex, np.zeros((0, 3), np.float32), (1, 3)), 4, range=(0, 1))
    assert hist.compute().tolist() == [0, 0, 0, 0] and edges.compute().tolist() == [0, 0.25, 0.5, 0.75, 1]


# ------------------------------------------------------------------ determinism


def test_two_runs_are_identical(ex, L):
    x = _adversarial(np.random.default_rng(700), np.float32, L + 1, n=100000)
    for bins in (100, L + 1):
        first = _check(ex, x, bins, (LO, HI), chunks=(30000,))
        second = _check(ex, x, bins, (LO, HI), chunks=(30000,))
        assert np.array_equal(first, second)
