"""cumulative_sum on the MI355X executor (``-m gpu``) against numpy's cumsum.

Parity is UNPINNED against the reference: cubed v0.12.0 has no
cumulative_sum; the semantics are numpy's ``cumsum`` along one axis.

Integer cases (and float32 data whose every partial sum is an integer below
2**24) are exact.  Float bounds are derived, not measured: every output is a
sum over some tree of at most n - 1 f64 additions, so its error is at most
gamma_{n-1}(2**-53) * A with A the cumulative sum of |x|; numpy's own f64
cumsum has the same bound and a float32 result adds one final rounding.  So

    f64:  |got - ref| <= 4 * n * 2**-53 * A
    f32:  |got - ref| <= 2**-24 * |ref| * (1 + 1e-6) + 4 * n * 2**-53 * A

(4 = 2 for the two sides x 2 for gamma's denominator and slack).  The f32
bound fails if f32 values are accumulated in f32; that is intended.
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


def _arr(ex, x, chunks, mem="2GB"):
    spec = cubed.Spec(allowed_mem=mem, reserved_mem=0, executor=ex)
    return cubed.from_array(x, chunks=chunks, spec=spec)


def _exact(got, x, axis, dtype):
    exp = np.cumsum(x, axis=axis, dtype=dtype)
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(got, exp)


# ------------------------------------------------------------------ exact cases


@pytest.mark.parametrize("axis", [0, 1, 2, -1])
def test_int32_3d_edge_chunks(ex, axis):
    # columns kernel at one element per lane (14-wide edge chunks), rows
    # kernel on the last axis, carries over 4, 3 and 3 blocks
    rng = np.random.default_rng(1)
    x = rng.integers(-1000, 1000, size=(37, 5, 46), dtype=np.int32)
    got = xp.cumulative_sum(_arr(ex, x, (10, 2, 16)), axis=axis).compute()
    _exact(got, x, axis, np.int64)


def test_int64_aligned_columns(ex):
    # columns kernel, 4 elements per lane
    rng = np.random.default_rng(2)
    x = rng.integers(-2**40, 2**40, size=(40, 64), dtype=np.int64)
    got = xp.cumulative_sum(_arr(ex, x, (8, 32)), axis=0).compute()
    _exact(got, x, 0, np.int64)


def test_int64_rows_tiles_and_tail(ex):
    # rows kernel: 300 = one 256-element tile + a 44-element tail, a carry
    # over 4 blocks and a 100-wide edge chunk (int64 rows always start on 16
    # bytes; the float32 test below has rows that do not)
    rng = np.random.default_rng(3)
    x = rng.integers(-2**40, 2**40, size=(5, 1000), dtype=np.int64)
    got = xp.cumulative_sum(_arr(ex, x, (2, 300)), axis=1).compute()
    _exact(got, x, 1, np.int64)


def test_float32_rows_unaligned_starts(ex):
    # rows of 301 float32: consecutive rows start 1204 bytes apart, so three
    # of every four take the element-at-a-time loads; small integers keep
    # every partial sum exact
    rng = np.random.default_rng(4)
    x = rng.integers(-8, 9, size=(7, 903)).astype(np.float32)
    got = xp.cumulative_sum(_arr(ex, x, (4, 301)), axis=1).compute()
    _exact(got, x, 1, np.float32)


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 10_000])
def test_int64_1d(ex, n):
    rng = np.random.default_rng(n)
    x = rng.integers(-2**40, 2**40, size=(n,), dtype=np.int64)
    got = xp.cumulative_sum(_arr(ex, x, (1024,))).compute()
    _exact(got, x, 0, np.int64)


def test_uint64_wraps_like_numpy(ex):
    rng = np.random.default_rng(5)
    x = rng.integers(2**63, 2**63 + 2**20, size=(9, 50), dtype=np.uint64)
    for axis, chunks in ((0, (2, 50)), (1, (9, 16))):
        got = xp.cumulative_sum(_arr(ex, x, chunks), axis=axis).compute()
        with np.errstate(over="ignore"):
            _exact(got, x, axis, np.uint64)
    assert np.cumsum(x, axis=0)[1].max() < 2**22  # the sums did wrap


def test_int8_to_requested_int32(ex):
    rng = np.random.default_rng(6)
    x = rng.integers(-128, 128, size=(300, 6), dtype=np.int8)
    got = xp.cumulative_sum(_arr(ex, x, (64, 6)), axis=0, dtype=np.int32).compute()
    _exact(got, x, 0, np.int32)
    # a narrow result wraps as narrow arithmetic does
    got = xp.cumulative_sum(_arr(ex, x, (64, 6)), axis=0, dtype=np.int8).compute()
    _exact(got, x, 0, np.int8)


def test_float32_small_integers_are_exact(ex):
    rng = np.random.default_rng(7)
    x = rng.integers(-8, 9, size=(50, 7, 12)).astype(np.float32)
    got = xp.cumulative_sum(_arr(ex, x, (10, 7, 12)), axis=0).compute()
    _exact(got, x, 0, np.float32)


def test_int64_4d_outer_and_inner(ex):
    rng = np.random.default_rng(8)
    x = rng.integers(-2**40, 2**40, size=(3, 20, 4, 6), dtype=np.int64)
    got = xp.cumulative_sum(_arr(ex, x, (2, 6, 4, 4)), axis=1).compute()
    _exact(got, x, 1, np.int64)


# ------------------------------------------------------------------ float cases


def _check_float(got, x, axis):
    ref = np.cumsum(x.astype(np.float64), axis=axis)
    A = np.cumsum(np.abs(x).astype(np.float64), axis=axis)
    n = x.shape[axis]
    assert got.dtype == x.dtype and got.shape == x.shape
    err = np.abs(got.astype(np.float64) - ref)
    bound = 4 * n * 2.0 ** -53 * A
    if x.dtype == np.float32:
        bound = 2.0 ** -24 * np.abs(ref) * (1 + 1e-6) + bound
    worst = np.max(err - bound)
    print(f"cumulative_sum {x.dtype} {x.shape} axis {axis}: max err {err.max():.3e}, "
          f"max (err - bound) {worst:.3e}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("axis", [0, 1])
def test_float64_normal(ex, axis):
    x = np.random.default_rng(11).standard_normal((180, 150))
    got = xp.cumulative_sum(_arr(ex, x, (32, 40)), axis=axis).compute()
    _check_float(got, x, axis)


def test_float32_smoke_shape(ex):
    x = np.random.default_rng(12).standard_normal((50, 37, 40)).astype(np.float32)
    got = xp.cumulative_sum(_arr(ex, x, (10, 37, 40)), axis=0).compute()
    _check_float(got, x, 0)


def test_float32_long_rows(ex):
    x = np.random.default_rng(13).standard_normal((6, 1500)).astype(np.float32)
    got = xp.cumulative_sum(_arr(ex, x, (6, 512)), axis=1).compute()
    _check_float(got, x, 1)


# ------------------------------------------------------------------ determinism, composition


def test_same_plan_twice_is_bit_identical(ex):
    x = np.random.default_rng(14).standard_normal((180, 150)).astype(np.float32)
    y = xp.cumulative_sum(_arr(ex, x, (32, 40)), axis=1)
    first = y.compute()
    second = y.compute()
    assert np.array_equal(first, second)
    z = xp.cumulative_sum(_arr(ex, x, (32, 40)), axis=1)
    assert np.array_equal(first, z.compute())


def test_elementwise_producer_and_reduction_consumer(ex):
    rng = np.random.default_rng(15)
    u, v, a = rng.standard_normal((3, 60, 44))
    got = xp.cumulative_sum(_arr(ex, u, (16, 44)) * _arr(ex, v, (16, 44)), axis=0).compute()
    _check_float(got, u * v, 0)
    got = xp.sum(xp.cumulative_sum(_arr(ex, a, (16, 20)), axis=1), axis=0).compute()
    np.testing.assert_allclose(got, np.sum(np.cumsum(a, axis=1), axis=0), rtol=1e-12, atol=1e-12)


def test_scan_of_a_rechunked_array(ex):
    x = np.random.default_rng(16).integers(-2**40, 2**40, size=(48, 40), dtype=np.int64)
    a = _arr(ex, x, (6, 40))
    r = a.rechunk((48, 8))  # not requested: only the scan reads it
    got = xp.cumulative_sum(r, axis=0).compute()
    _exact(got, x, 0, np.int64)
    got = xp.cumulative_sum(a.rechunk((12, 10)), axis=1).compute()
    _exact(got, x, 1, np.int64)


# ------------------------------------------------------------------ raw ABI


def test_raw_scan_chunks_exclusive_then_carry(ex):
    import torch

    outer, n, inner = 3, 70, 5
    rng = np.random.default_rng(17)
    x = rng.integers(-2**40, 2**40, size=(outer, n, inner), dtype=np.int64)
    carry = rng.integers(-2**40, 2**40, size=(outer, 4, inner), dtype=np.int64)  # 4 planes; use plane 2
    dev = ex.device
    d_x = torch.from_numpy(x).to(dev)
    d_c = torch.from_numpy(carry).to(dev)
    d_out = torch.zeros_like(d_x)
    L = nat.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run(exclusive, with_carry):
        rows = np.zeros(1, dtype=nat.SCAN_TASK_DTYPE)
        rows[0]["src_base"], rows[0]["dst_base"] = d_x.data_ptr(), d_out.data_ptr()
        rows[0]["outer"], rows[0]["n"], rows[0]["inner"] = outer, n, inner
        rows[0]["src_outer_stride"] = rows[0]["dst_outer_stride"] = n * inner
        rows[0]["src_n_stride"] = rows[0]["dst_n_stride"] = inner
        if with_carry:
            rows[0]["carry_base"] = d_c.data_ptr() + 2 * inner * 8
            rows[0]["carry_outer_stride"] = 4 * inner
        path = L.cubed_scan_path(rows.ctypes.data, 1, 2)
        assert path == nat.SCAN_COLS
        table = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
        d_out.zero_()
        nat.check(L.cubed_scan_chunks(table.data_ptr(), 1, 2, int(exclusive), path, outer * inner, stream),
                  "cubed_scan_chunks")
        torch.cuda.synchronize(dev)
        return d_out.cpu().numpy()

    inclusive = np.cumsum(x, axis=1)
    got = run(exclusive=True, with_carry=False)
    assert np.array_equal(got[:, 0], np.zeros((outer, inner), np.int64))
    assert np.array_equal(got[:, 1:], inclusive[:, :-1])
    got = run(exclusive=False, with_carry=True)
    assert np.array_equal(got, inclusive + carry[:, 2:3, :])
