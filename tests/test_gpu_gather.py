"""take_along_axis on the MI355X executor (``-m gpu``) against numpy.

Every comparison is ``np.array_equal`` on the bits of the result against
``np.take_along_axis``: elements are moved, never computed, so no tolerance
enters.  An index outside ``[-n, n)`` cannot raise in a lazy call; the
documented result there is a zero element."""

import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
import cubed_amd.lowering as Lw
from cubed_amd import _native as nat
from cubed_amd import ir

pytestmark = pytest.mark.gpu

UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def ex(gpu_executor):
    return gpu_executor


@pytest.fixture(scope="module")
def T(built):
    return nat.gather_tile_bytes()


def _arr(ex, x, chunks, mem="2GB"):
    spec = cubed.Spec(allowed_mem=mem, reserved_mem=0, executor=ex)
    return cubed.from_array(x, chunks=chunks, spec=spec)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def _expected_bits(x, idx, axis):
    """np.take_along_axis on the bits of x; zero where the index is outside [-n, n)."""
    n = x.shape[axis]
    i = idx.astype(np.int64)
    valid = (i >= -n) & (i < n)
    exp = np.take_along_axis(_bits(x), np.where(valid, i, 0), axis)
    exp[~valid] = 0
    return exp


def _check(ex, x, idx, axis, xchunks=None, ichunks=None):
    xchunks = x.shape if xchunks is None else xchunks
    ichunks = idx.shape if ichunks is None else ichunks
    y = xp.take_along_axis(_arr(ex, x, xchunks), _arr(ex, idx, ichunks), axis=axis)
    got = y.compute()
    assert ir.is_bf16(y.dtype) if ir.is_bf16(x.dtype) else y.dtype == x.dtype
    if ir.is_bf16(x.dtype):
        # compute() hands bfloat16 out widened to float32, exactly; narrowing it back is exact too
        assert got.dtype == np.float32
        got = ir.numpy_to_bf16(got)
    assert got.dtype == x.dtype and got.shape == idx.shape
    exp = _expected_bits(x, idx, axis)
    assert np.array_equal(_bits(got), exp), np.flatnonzero((_bits(got) != exp).ravel())[:5]
    return y


def _values(rng, shape, dtype):
    """Random elements of every bit pattern class the dtype has."""
    dtype = "bfloat16" if dtype is ir.bfloat16 else dtype
    if dtype == "bfloat16":
        return ir.numpy_to_bf16(rng.standard_normal(shape).astype(np.float32))
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return rng.random(shape) < 0.5
    if dt.kind == "f":
        return rng.standard_normal(shape).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=shape, dtype=dt, endpoint=True)


def _perms(rng, rows, n):
    return np.stack([rng.permutation(n) for _ in range(rows)]).astype(np.int64)


# ------------------------------------------------------------------ one chunk, last axis


def _n_src(T, esize):
    return [1, T // esize - 1, T // esize, T // esize + 1, 3 * (T // esize) + 5, 63, 64, 65]


@pytest.mark.parametrize("dtype", [np.float32, np.int64])
@pytest.mark.parametrize("i", range(8))
def test_row_sizes_around_the_tile(ex, T, dtype, i):
    n = _n_src(T, np.dtype(dtype).itemsize)[i]
    rng = np.random.default_rng(100 + i)
    _check(ex, _values(rng, (3, n), dtype), _perms(rng, 3, n), -1)


@pytest.mark.parametrize("dtype", ["bool", "int16", "bfloat16", "float32", "float64"])
def test_every_element_size(ex, dtype):
    rng = np.random.default_rng(7)
    x = _values(rng, (5, 1001), dtype)
    idx = _perms(rng, 5, 1001)
    _check(ex, x, idx, 1)
    _check(ex, x, idx, 1, xchunks=(2, 300), ichunks=(2, 300))


@pytest.mark.parametrize("shape", [(3, 37), (3, 5, 7)])
def test_misaligned_chunks(ex, shape):
    rng = np.random.default_rng(11)
    for dtype in (np.int8, np.int16, np.float32, np.float64):
        x = _values(rng, shape, dtype)
        for axis in range(len(shape)):
            idx = rng.integers(0, shape[axis], size=shape)
            _check(ex, x, idx, axis)


@pytest.mark.parametrize("axis", [0, 1, 2, -1])
def test_every_axis_ragged_blocks(ex, axis):
    rng = np.random.default_rng(13)
    x = _values(rng, (7, 13, 11), np.float32)
    idx = rng.integers(0, x.shape[axis], size=x.shape)
    _check(ex, x, idx, axis, xchunks=(3, 5, 4), ichunks=(3, 5, 4))


# ------------------------------------------------------------------ index extents


def test_index_extents(ex):
    rng = np.random.default_rng(17)
    x = _values(rng, (6, 50), np.float64)
    for axis, n in ((0, 6), (1, 50)):
        for n_idx in (1, 3 * n):
            shape = [6, 50]
            shape[axis] = n_idx
            idx = rng.integers(0, n, size=shape)
            _check(ex, x, idx, axis)
            _check(ex, x, idx, axis, xchunks=(4, 20), ichunks=(4, 20))
    # indices chunked differently from x along the axis, and off it (rechunked)
    idx = rng.integers(0, 50, size=(6, 50))
    y = _check(ex, x, idx, 1, xchunks=(4, 20), ichunks=(4, 7))
    assert y.chunks == ((4, 2), (7,) * 7 + (1,))
    y = _check(ex, x, idx, 1, xchunks=(4, 20), ichunks=(5, 7))
    assert y.chunks == ((4, 2), (7,) * 7 + (1,))


# ------------------------------------------------------------------ index values


def test_equal_identity_reverse(ex):
    rng = np.random.default_rng(19)
    x = _values(rng, (4, 300), np.float32)
    for chunks in ((4, 300), (3, 128)):
        for row in (np.full(300, 217), np.arange(300), np.arange(300)[::-1]):
            idx = np.broadcast_to(row, (4, 300)).astype(np.int64).copy()
            _check(ex, x, idx, 1, xchunks=chunks, ichunks=chunks)


def test_negative_indices_two_blocks(ex):
    rng = np.random.default_rng(23)
    x = _values(rng, (5, 40), np.int32)
    idx = rng.integers(-40, 40, size=(5, 90))
    idx[0, :80] = np.arange(-40, 40)
    _check(ex, x, idx, 1, xchunks=(5, 20), ichunks=(5, 90))
    x0, idx0 = np.ascontiguousarray(x.T), np.ascontiguousarray(idx.T)
    _check(ex, x0, idx0, 0, xchunks=(20, 5), ichunks=(90, 5))


@pytest.mark.parametrize("itype", [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64])
def test_every_index_dtype(ex, itype):
    rng = np.random.default_rng(29)
    x = _values(rng, (3, 100), np.float32)
    lo = -100 if np.dtype(itype).kind == "i" else 0
    idx = rng.integers(lo, 100, size=(3, 100)).astype(itype)
    _check(ex, x, idx, 1, xchunks=(3, 40), ichunks=(3, 40))


@pytest.mark.parametrize("chunk", [90, 30])  # 1 and 3 blocks
def test_out_of_range_gives_zero(ex, chunk):
    rng = np.random.default_rng(31)
    n = 90
    i64 = np.iinfo(np.int64)
    bad = np.array([n, n + 1, -n - 1, i64.min, i64.max, i64.min + n, i64.max - n, 1 << 40], dtype=np.int64)
    for dtype in (np.float32, np.int64):
        x = _values(rng, (4, n), dtype)
        x[x == 0] = 1  # a zero in the result is then an out-of-range place
        idx = rng.integers(-n, n, size=(4, 200))
        at = rng.choice(200, size=(4, len(bad)), replace=True)
        for r in range(4):
            idx[r, at[r]] = bad
        _check(ex, x, idx, 1, xchunks=(4, chunk), ichunks=(4, 64))
        _check(ex, np.ascontiguousarray(x.T), np.ascontiguousarray(idx.T), 0, xchunks=(chunk, 4), ichunks=(64, 4))


# ------------------------------------------------------------------ bits


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_bit_patterns_survive(ex, dtype):
    dt = np.dtype(dtype)
    u = UINT[dt.itemsize]
    mant = 23 if dt.itemsize == 4 else 52
    exp_all = (0xff if dt.itemsize == 4 else 0x7ff) << mant
    sign = 1 << (8 * dt.itemsize - 1)
    pats = [0, sign, exp_all, exp_all | sign, 1, sign | 1, (1 << mant) - 1]         # zeros, infinities, denormals
    pats += [exp_all | (1 << (mant - 1)) | p for p in (0, 1, 2, 0x1234)]              # quiet NaNs, distinct payloads
    pats += [exp_all | p for p in (1, 0x55)] + [sign | exp_all | (1 << (mant - 1)) | 7]  # signalling, negative NaNs
    x = np.tile(np.array(pats, dtype=u), (3, 4)).view(dt)
    assert np.isnan(x).sum() == 3 * 4 * 7
    rng = np.random.default_rng(37)
    idx = rng.integers(-x.shape[1], x.shape[1], size=(3, 200))
    _check(ex, x, idx, 1)
    _check(ex, x, idx, 1, xchunks=(2, 20), ichunks=(2, 64))


# ------------------------------------------------------------------ composition


@pytest.fixture(scope="module")
def ties_and_nans():
    rng = np.random.default_rng(41)
    x = (rng.integers(-20, 20, size=(64, 50)) / 4).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = np.nan
    return x


@pytest.mark.parametrize("axis", [0, -1])
@pytest.mark.parametrize("blocks", [1, 3])
def test_argsort_applied_is_sort(ex, ties_and_nans, axis, blocks):
    x = ties_and_nans
    chunks = (64, 50) if blocks == 1 else ((22, 50) if axis == 0 else (64, 17))
    a = _arr(ex, x, chunks)
    got = xp.take_along_axis(a, xp.argsort(a, axis=axis), axis=axis).compute()
    want = xp.sort(a, axis=axis).compute()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got), _bits(np.sort(x, axis=axis)))


@pytest.mark.parametrize("axis", [0, -1])
@pytest.mark.parametrize("blocks", [1, 3])
def test_argmax_applied_is_max(ex, axis, blocks):
    rng = np.random.default_rng(43)
    x = rng.standard_normal((64, 50)).astype(np.float32)
    chunks = (64, 50) if blocks == 1 else ((22, 50) if axis == 0 else (64, 17))
    a = _arr(ex, x, chunks)
    got = xp.take_along_axis(a, xp.argmax(a, axis=axis, keepdims=True), axis=axis).compute()
    want = xp.max(a, axis=axis, keepdims=True).compute()
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(got, x.max(axis=axis, keepdims=True))


def test_lazy_indices_compute_once(ex):
    rng = np.random.default_rng(47)
    x = _values(rng, (6, 40), np.float32)
    yv = rng.standard_normal((6, 40)).astype(np.float32)
    a, b = _arr(ex, x, (6, 16)), _arr(ex, yv, (6, 16))
    idx = xp.argsort(b, axis=1) % 7
    got = xp.take_along_axis(a, idx, axis=1).compute()
    exp = np.take_along_axis(x, np.argsort(yv, axis=1, kind="stable") % 7, 1)
    assert np.array_equal(_bits(got), _bits(exp))


# ------------------------------------------------------------------ the two forms


def test_both_forms_agree(ex, T, monkeypatch):
    rng = np.random.default_rng(53)
    n = T // 4 - 3  # an odd row length inside the tile: rows start off 16 bytes
    x = _values(rng, (5, n), np.float32)
    idx = rng.integers(-n, n, size=(5, 2 * n + 1))
    seen = []

    class Recording(Lw.GatherLaunch):
        forced = None

        def __init__(self, rows, esize, device, sink=None, path=None):
            super().__init__(rows, esize, device, sink, path=self.forced)
            seen.append(self.path)

    monkeypatch.setattr(Lw, "GatherLaunch", Recording)
    lds = xp.take_along_axis(_arr(ex, x, x.shape), _arr(ex, idx, idx.shape), axis=1).compute()
    Recording.forced = nat.GATHER_DIRECT
    direct = xp.take_along_axis(_arr(ex, x, x.shape), _arr(ex, idx, idx.shape), axis=1).compute()
    assert seen == [nat.GATHER_LDS, nat.GATHER_DIRECT]
    assert np.array_equal(_bits(lds), _bits(direct))
    assert np.array_equal(_bits(lds), _expected_bits(x, idx, 1))
