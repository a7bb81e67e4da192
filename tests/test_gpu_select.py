"""nonzero, boolean-mask indexing and count_nonzero on the MI355X executor
(``-m gpu``) against numpy.

Parity is UNPINNED against the reference: cubed v0.12.0 has none of the three.
``np.nonzero(x)``, ``x[mask]`` and ``np.count_nonzero`` on the same data are the
yardstick.  Every comparison is exact."""

import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
from cubed_amd import _native as nat
from cubed_amd import ir
from cubed_amd.core import ops
from cubed_amd.primitive.blockwise import apply_blockwise

pytestmark = pytest.mark.gpu

SIZE_DTYPES = [np.uint8, np.bool_, np.int16, np.float32, np.float64]
PATTERNS = ("none", "all", "half", "first", "last")


@pytest.fixture(scope="module")
def ex(gpu_executor):
    return gpu_executor


@pytest.fixture(scope="module")
def tile_bytes(built):
    return nat.select_tile_bytes()


def _arr(ex, x, chunks=None):
    spec = cubed.Spec(allowed_mem="2GB", reserved_mem=0, executor=ex)
    return cubed.from_array(x, chunks=x.shape if chunks is None else chunks, spec=spec)


def _host(x):
    """x as numpy sees its values (bfloat16 widened exactly to float32)."""
    return ir.bf16_to_numpy(x) if ir.is_bf16(x.dtype) else x


def _check_nonzero(ex, x, chunks=None):
    want = np.nonzero(_host(x))
    got = xp.nonzero(_arr(ex, x, chunks))
    assert isinstance(got, tuple) and len(got) == x.ndim
    out = []
    for d, (g, w) in enumerate(zip(got, want)):
        assert g.ndim == 1 and g.dtype == np.int64 and g.shape == w.shape, (d, g.shape, w.shape)
        h = g.compute()
        assert h.dtype == np.int64 and h.shape == w.shape and np.array_equal(h, w), (d, h[:8], w[:8])
        out.append(h)
    return out


def _check_mask(ex, v, mask, chunks=None, mask_chunks=None, as_numpy=False):
    want = _host(v)[mask]
    m = mask if as_numpy else _arr(ex, mask, mask_chunks if mask_chunks is not None else chunks)
    got = _arr(ex, v, chunks)[m]
    assert got.ndim == 1 and got.shape == want.shape
    assert got.dtype == v.dtype
    h = got.compute()
    assert h.shape == want.shape and h.dtype == want.dtype and h.tobytes() == want.tobytes()
    return h


def _pattern(rng, name, n, dtype):
    dtype = np.dtype(dtype)
    x = np.zeros(n, dtype=dtype)
    one = True if dtype.kind == "b" else (dtype.type(-3) if dtype.kind in "if" else dtype.type(200))
    if name == "all":
        x[:] = one
    elif name == "half":
        x[rng.random(n) < 0.5] = one
    elif name == "first":
        x[0] = one
    elif name == "last":
        x[-1] = one
    return x


def _sizes(tile_bytes, esize):
    V = 16 // esize
    R, T = 64 * V, tile_bytes // esize
    return [1, V - 1, V, V + 1, R - 1, R, R + 1, T - 1, T, T + 1, 3 * T + 5]


# ------------------------------------------------------------------ sizes around the vector, the round and the tile


@pytest.mark.parametrize("dtype", SIZE_DTYPES)
@pytest.mark.parametrize("i", range(11))
def test_sizes_in_one_chunk(ex, tile_bytes, dtype, i):
    n = _sizes(tile_bytes, np.dtype(dtype).itemsize)[i]
    rng = np.random.default_rng(2000 + i)
    values = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
    for name in PATTERNS:
        x = _pattern(rng, name, n, dtype)
        (got,) = _check_nonzero(ex, x)
        assert len(got) == {"none": 0, "all": n, "first": 1, "last": 1}.get(name, len(got)), name
        _check_mask(ex, values, x != 0)


# ------------------------------------------------------------------ special values


@pytest.mark.parametrize("dtype", ["float32", "float64", "bfloat16"])
def test_float_specials(ex, dtype):
    if dtype == "bfloat16":
        bits = np.array([0x0000, 0x8000, 0x7fc0, 0xffc0, 0x7f80, 0xff80, 0x0001, 0x8001], dtype=np.uint16)
        x = np.tile(bits, 5).view(ir.bfloat16)
        assert np.isnan(_host(x)[2]) and np.isnan(_host(x)[3]) and _host(x)[6] > 0 > _host(x)[7]
    else:
        dt = np.dtype(dtype)
        tiny = np.nextafter(dt.type(0), dt.type(1))
        x = np.tile(np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, tiny, -tiny], dtype=dt), 5)
        assert tiny > 0 and tiny / 2 == 0
    (got,) = _check_nonzero(ex, x, chunks=(16,))
    assert got.tolist() == [8 * r + j for r in range(5) for j in range(2, 8)]
    mask = np.arange(len(x)) % 3 == 0
    _check_mask(ex, x, mask, chunks=(16,))


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64])
def test_integer_specials(ex, dtype):
    info = np.iinfo(dtype)
    x = np.tile(np.array([0, info.min, -1, info.max], dtype=dtype), 9)
    (got,) = _check_nonzero(ex, x, chunks=(10,))
    assert got.tolist() == [j for j in range(36) if j % 4]
    _check_mask(ex, x, x < 0, chunks=(10,))


def test_uint64_top_bit(ex):
    x = np.zeros(50, dtype=np.uint64)
    x[[3, 17, 49]] = np.uint64(1) << np.uint64(63)
    (got,) = _check_nonzero(ex, x, chunks=(20,))
    assert got.tolist() == [3, 17, 49]
    for dtype in (np.uint8, np.uint16, np.uint32):
        y = np.zeros(50, dtype=dtype)
        y[[0, 31]] = np.iinfo(dtype).max // 2 + 1
        assert _check_nonzero(ex, y, chunks=(20,))[0].tolist() == [0, 31]


# ------------------------------------------------------------------ chunked arrays


def test_chunked_1d_with_an_all_zero_chunk(ex):
    rng = np.random.default_rng(51)
    x = rng.integers(-1, 2, size=4099).astype(np.float32)
    x[2000:3000] = 0
    (got,) = _check_nonzero(ex, x, chunks=(1000,))
    assert not ((got >= 2000) & (got < 3000)).any() and (got >= 3000).any()
    _check_mask(ex, rng.standard_normal(4099), x != 0, chunks=(1000,))


@pytest.mark.parametrize("dtype", [np.bool_, np.int32, np.float64])
def test_chunked_2d(ex, dtype):
    rng = np.random.default_rng(52)
    x = (rng.random((37, 46)) < 0.3).astype(dtype)
    _check_nonzero(ex, x, chunks=(10, 16))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_chunked_3d(ex, dtype):
    rng = np.random.default_rng(53)
    x = (rng.integers(0, 3, size=(5, 7, 9)) * (rng.random((5, 7, 9)) < 0.6)).astype(dtype)
    got = _check_nonzero(ex, x, chunks=(2, 3, 4))
    assert len(got) == 3 and len(got[0]) == np.count_nonzero(x)


# ------------------------------------------------------------------ x[mask]


@pytest.mark.parametrize("dtype", ["int8", "uint8", "bool", "int16", "bfloat16", "int32", "float32", "uint64",
                                   "float64"])
def test_mask_over_every_value_size(ex, dtype):
    rng = np.random.default_rng(61)
    if dtype == "bfloat16":
        v = ir.numpy_to_bf16(rng.standard_normal((37, 46)).astype(np.float32))
    elif dtype == "bool":
        v = rng.random((37, 46)) < 0.5
    elif np.dtype(dtype).kind == "f":
        v = rng.standard_normal((37, 46)).astype(dtype)
    else:
        info = np.iinfo(dtype)
        v = rng.integers(info.min, info.max, size=(37, 46), dtype=dtype, endpoint=True)
    mask = rng.random((37, 46)) < 0.4
    _check_mask(ex, v, mask, chunks=(10, 16))                                   # the mask in x's chunks
    _check_mask(ex, v, mask, chunks=(10, 16), mask_chunks=(37, 5))              # in other chunks
    _check_mask(ex, v, mask, chunks=(10, 16), as_numpy=True)                    # a numpy mask


def test_lazy_masks(ex):
    rng = np.random.default_rng(62)
    v = rng.standard_normal((37, 46)).astype(np.float32)
    v[rng.random((37, 46)) < 0.2] = np.nan
    x = _arr(ex, v, (10, 16))
    got = x[x > 0]
    want = v[v > 0]
    assert got.shape == want.shape and got.dtype == np.float32 and got.compute().tobytes() == want.tobytes()
    got = x[~xp.isnan(x)]
    want = v[~np.isnan(v)]
    assert got.shape == want.shape and got.compute().tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", [np.int16, np.float64])
def test_nothing_and_everything_selected(ex, dtype):
    v = np.arange(4099).astype(dtype)
    got = _check_mask(ex, v, np.zeros(4099, dtype=bool), chunks=(1000,))
    assert got.shape == (0,) and got.dtype == np.dtype(dtype)
    got = _check_mask(ex, v, np.ones(4099, dtype=bool), chunks=(1000,))
    assert got.shape == (4099,)
    for d in xp.nonzero(_arr(ex, np.zeros((6, 5), dtype=dtype), (4, 2))):
        assert d.shape == (0,) and d.dtype == np.int64 and d.compute().shape == (0,)


def test_pieces_straddle_output_chunks(ex):
    # k > c with uneven counts per chunk, some chunks with none
    c = 16
    counts = [1, 16, 0, 1, 16, 2, 0, 0, 3, 9, 16, 7]
    mask = np.zeros(len(counts) * c, dtype=bool)
    rng = np.random.default_rng(63)
    for b, k in enumerate(counts):
        mask[b * c + rng.permutation(c)[:k]] = True
    v = rng.integers(-1000, 1000, size=len(mask)).astype(np.int32)
    assert ops.select_count(_arr(ex, mask, (c,))).compute().tolist() == counts
    _check_mask(ex, v, mask, chunks=(c,))
    _check_nonzero(ex, mask, chunks=(c,))


# ------------------------------------------------------------------ the kernel's own outputs


@pytest.mark.parametrize("dtype,vdtype", [(np.bool_, np.float32), (np.float32, np.int8), (np.int16, np.int64),
                                          (np.float64, np.uint16)])
def test_pack_fills_the_front_and_zeroes_the_tail(ex, tile_bytes, dtype, vdtype):
    c = tile_bytes // np.dtype(dtype).itemsize + 7
    n = 3 * c - 11
    rng = np.random.default_rng(71)
    x = (rng.random(n) < 0.37).astype(dtype)
    v = rng.integers(1, 100, size=n).astype(vdtype)
    f, g = _arr(ex, x, (c,)), _arr(ex, v, (c,))
    counts = ops.select_count(f).compute()
    pos = ops.select_pack(f).compute()
    vals = ops.select_pack(f, g).compute()
    assert counts.dtype == np.int64 and pos.dtype == np.int64 and vals.dtype == np.dtype(vdtype)
    for b in range(3):
        lo, hi = b * c, min((b + 1) * c, n)
        at = lo + np.flatnonzero(x[lo:hi])
        assert counts[b] == len(at)
        want = np.zeros(hi - lo, dtype=np.int64)
        want[:len(at)] = at
        assert np.array_equal(pos[lo:hi], want)
        want = np.zeros(hi - lo, dtype=vdtype)
        want[:len(at)] = v[at]
        assert vals[lo:hi].tobytes() == want.tobytes()


# ------------------------------------------------------------------ phase 2 starts from HBM; reruns


def test_the_results_plan_does_not_select_again(ex):
    rng = np.random.default_rng(81)
    x = (rng.random((37, 46)) < 0.5).astype(np.float32)
    a = _arr(ex, x, (10, 16))
    results = list(xp.nonzero(a)) + [a[a != 0]]
    for r in results:
        progs = [d["pipeline"].config.function for _, d in r.plan.dag.nodes(data=True)
                 if d.get("pipeline") is not None and d["pipeline"].function is apply_blockwise]
        assert progs and not [p for p in progs if isinstance(p, ir.SelectProgram)]
    want = np.nonzero(x)
    for r, w in zip(results, want):
        assert np.array_equal(r.compute(), w) and np.array_equal(r.compute(), w)   # and can be computed twice
    assert np.array_equal(results[2].compute(), x[x != 0])


def test_two_runs_are_bit_identical(ex, tile_bytes):
    T = tile_bytes // 4
    rng = np.random.default_rng(91)
    x = (rng.random(3 * T + 5) < 0.5).astype(np.float32)
    v = rng.standard_normal(3 * T + 5)
    runs = []
    for _ in range(2):
        (pos,) = xp.nonzero(_arr(ex, x, (T + 1,)))
        vals = _arr(ex, v, (T + 1,))[_arr(ex, x != 0, (T + 1,))]
        runs.append([pos.compute().tobytes(), vals.compute().tobytes()])
    assert runs[0] == runs[1]
    assert runs[0][0] == np.flatnonzero(x).astype(np.int64).tobytes()


# ------------------------------------------------------------------ count_nonzero


@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.bool_])
def test_count_nonzero(ex, dtype):
    rng = np.random.default_rng(101)
    x = (rng.integers(-2, 3, size=(5, 7, 9)) * (rng.random((5, 7, 9)) < 0.6)).astype(dtype)
    a = _arr(ex, x, (2, 3, 4))
    for kwargs in (dict(), dict(axis=0), dict(axis=(0, 1)), dict(keepdims=True), dict(axis=2, keepdims=True)):
        got = xp.count_nonzero(a, **kwargs)
        want = np.asarray(np.count_nonzero(x, **kwargs)).astype(np.int64)
        assert got.dtype == np.int64 and got.shape == want.shape
        assert np.array_equal(np.asarray(got.compute()), want), kwargs
