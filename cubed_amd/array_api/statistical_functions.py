"""Statistical functions (cubed/array_api/statistical_functions.py:22-156).

``mean`` keeps the reference's structured ``{n: int64, total: float64}``
intermediate (stored SoA in HBM) and its reduction rounds; the chunk
functions are the program builders of cubed_amd.chunkfuncs."""

import numpy as np

from ..chunkfuncs import (NumpyReduction, _mean_aggregate, _mean_combine, _mean_func, _var_combine,
                          _var_func, _VarAggregate)
from ..core import reduction, scan
from ..core.ops import validate_axis
from .dtypes import (
    _numeric_dtypes,
    _real_floating_dtypes,
    _real_numeric_dtypes,
    _signed_integer_dtypes,
    _unsigned_integer_dtypes,
    bfloat16,
    complex64,
    complex128,
    float32,
    float64,
    int64,
    uint64,
)

_np_max = NumpyReduction("max", "max")
_np_min = NumpyReduction("min", "min")
_np_sum = NumpyReduction("sum", "sum")
_np_prod = NumpyReduction("prod", "prod")


def max(x, /, *, axis=None, keepdims=False):
    if x.dtype not in _real_numeric_dtypes:
        raise TypeError("Only real numeric dtypes are allowed in max")
    return reduction(x, _np_max, axis=axis, dtype=x.dtype, keepdims=keepdims)


def min(x, /, *, axis=None, keepdims=False):
    if x.dtype not in _real_numeric_dtypes:
        raise TypeError("Only real numeric dtypes are allowed in min")
    return reduction(x, _np_min, axis=axis, dtype=x.dtype, keepdims=keepdims)


def mean(x, /, *, axis=None, keepdims=False, use_new_impl=False):
    if x.dtype not in _real_floating_dtypes:
        raise TypeError("Only real floating-point dtypes are allowed in mean")
    dtype = x.dtype
    intermediate_dtype = [("n", np.int64), ("total", np.float64)]
    extra_func_kwargs = dict(dtype=intermediate_dtype)
    return reduction(x, _mean_func, combine_func=_mean_combine, aggegrate_func=_mean_aggregate,
                     axis=axis, intermediate_dtype=intermediate_dtype, dtype=dtype,
                     keepdims=keepdims, use_new_impl=use_new_impl,
                     extra_func_kwargs=extra_func_kwargs)


def _default_sum_dtype(dt):
    if dt in _signed_integer_dtypes:
        return int64
    if dt in _unsigned_integer_dtypes:
        return uint64
    if dt == float32:
        return float64
    if dt == complex64:
        return complex128
    return dt


def _partials_dtype(dtype):
    """The dtype a sum / prod keeps between its rounds.  The kernels
    accumulate floats in float64 whatever the result dtype; a float32 or
    bfloat16 result keeps its per-chunk partials in float64 too and is
    rounded once, by the final astype -- partials stored in the result dtype
    would add one rounding per partial and combine round (a float32 sum over
    (7, 13) in (3, 5) chunks was off by two spacings)."""
    return float64 if np.dtype(dtype) in (float32, bfloat16) else dtype


def prod(x, /, *, axis=None, dtype=None, keepdims=False):
    if x.dtype not in _numeric_dtypes:
        raise TypeError("Only numeric dtypes are allowed in prod")
    if dtype is None:
        dtype = _default_sum_dtype(x.dtype)
    partials = _partials_dtype(dtype)
    return reduction(x, _np_prod, axis=axis, intermediate_dtype=partials, dtype=dtype, keepdims=keepdims,
                     extra_func_kwargs=dict(dtype=partials))


def sum(x, /, *, axis=None, dtype=None, keepdims=False):
    if x.dtype not in _numeric_dtypes:
        raise TypeError("Only numeric dtypes are allowed in sum")
    if dtype is None:
        dtype = _default_sum_dtype(x.dtype)
    partials = _partials_dtype(dtype)
    return reduction(x, _np_sum, axis=axis, intermediate_dtype=partials, dtype=dtype, keepdims=keepdims,
                     extra_func_kwargs=dict(dtype=partials))


def cumulative_sum(x, /, *, axis=None, dtype=None, include_initial=False):
    """Array API ``cumulative_sum`` (2023.12; not in the reference v0.12.0):
    numpy's ``cumsum`` along one axis, same shape and chunks as ``x``.

    Unlike ``sum``, float32 stays float32 (the result is full-size); signed
    integers give int64, unsigned ones uint64.  The scan itself runs on
    float32, float64 or 64-bit integer values -- floats always accumulate in
    float64 -- so any other input or requested dtype is converted by an
    ``astype`` before or after it (a wrapped 64-bit sum truncated to a narrow
    integer is the wrapped narrow sum)."""
    from .data_type_functions import astype

    if x.dtype not in _real_numeric_dtypes or x.dtype == bfloat16:
        raise TypeError("Only real numeric dtypes (other than bfloat16) are allowed in cumulative_sum")
    if dtype is None:
        dtype = x.dtype if x.dtype in (float32, float64) else _default_sum_dtype(x.dtype)
    elif np.dtype(dtype) not in _real_numeric_dtypes or np.dtype(dtype) == bfloat16:
        raise TypeError("Only real numeric dtypes (other than bfloat16) are allowed as the dtype "
                        "of cumulative_sum")
    dtype = np.dtype(dtype)
    if x.ndim == 0:
        raise ValueError("cumulative_sum needs an array of at least one dimension")
    if axis is None:
        if x.ndim != 1:
            raise ValueError("axis must be given for cumulative_sum of an array of more than one dimension")
        axis = 0
    axis = validate_axis(axis, x.ndim)
    if include_initial:
        raise NotImplementedError("cumulative_sum with include_initial=True is not supported: its "
                                  "shape does not fit the regular chunk grid")
    if dtype in (float32, float64):
        value_dtype = dtype
    else:
        value_dtype = uint64 if dtype in _unsigned_integer_dtypes else int64
    if x.size == 0:
        from .creation_functions import empty

        return empty(x.shape, dtype=dtype, chunks=x.chunks, spec=x.spec)
    result = scan(astype(x, value_dtype, copy=False), axis)
    return astype(result, dtype, copy=False)


def histogram(x, /, bins, *, range=None, density=False, weights=None):
    """``np.histogram`` of all elements of ``x`` (any shape and chunking):
    ``(hist, bin_edges)``, both one-chunk arrays; ``hist`` is int64 of shape
    ``(nbins,)``, or float64 with ``density=True``.

    ``bins`` is an int, and then ``range=(lo, hi)`` is required because ``x``
    is lazy and its extremes are not known, or a host 1-d array-like of
    non-decreasing edges, and then ``range`` is ignored as numpy ignores it.
    The edges are numpy's own, ``np.histogram_bin_edges`` of an empty array of
    ``x``'s dtype, so their dtype (float32 for float32 ``x``, else float64), a
    widened degenerate range and every ``ValueError`` are numpy's.  ``x`` is
    converted to the edges' dtype and counted by numpy's definition: bin ``i``
    holds ``e[i] <= v < e[i+1]``, the last bin also ``v == e[nbins]``; NaN and
    values outside ``[e[0], e[nbins]]`` are counted nowhere.

    The dtypes are those ``sort`` accepts.  ``weights`` is not supported: a
    float sum per bin through atomics would depend on the order of arrival.
    The reference has no histogram, so parity is unpinned; numpy is the
    yardstick."""
    from ..core.array import CoreArray
    from ..core.ops import from_array
    from ..core.ops import histogram as _histogram
    from .creation_functions import zeros
    from .data_type_functions import astype
    from .elementwise_functions import divide, multiply
    from .sorting_functions import _KEY_DTYPE

    if np.dtype(x.dtype) not in _KEY_DTYPE:
        raise TypeError("Only boolean, integer, float32 and float64 dtypes are allowed in histogram")
    if weights is not None:
        raise NotImplementedError("histogram with weights is not supported: a float sum per bin through "
                                  "atomics depends on the order of arrival")
    if isinstance(bins, CoreArray):
        raise TypeError("histogram: bins must be an int or a host array of edges; compute() the array first")
    uniform = np.ndim(bins) == 0
    if uniform and range is None:
        raise ValueError("histogram: range=(lo, hi) is required with an int bins, because x is lazy and "
                         "its minimum and maximum are not known")
    # numpy itself counts bool as uint8 (and says so in a warning that is no news here)
    like = np.empty(0, dtype=np.uint8 if x.dtype == np.bool_ else x.dtype)
    edges = np.histogram_bin_edges(like, bins, range if uniform else None)
    nbins = len(edges) - 1
    if nbins < 1:
        raise ValueError("histogram: bins must hold at least two edges")
    bin_edges = from_array(edges, chunks=edges.shape, spec=x.spec)
    if x.size == 0:
        hist = zeros((nbins,), dtype=int64, chunks=(nbins,), spec=x.spec)
    else:
        # explicit edges keep the dtype they came with; the comparison runs in float32 only
        # where both sides are float32, else in float64 as numpy's promotion has it
        key_dtype = float32 if edges.dtype == x.dtype == np.dtype(float32) else float64
        key_edges = bin_edges if edges.dtype == np.dtype(key_dtype) else \
            from_array(edges.astype(key_dtype), chunks=edges.shape, spec=x.spec)
        hist = _histogram(x, key_edges, nbins, uniform)
    if density:
        widths = from_array(np.diff(edges).astype(np.float64), chunks=(nbins,), spec=x.spec)
        counts = astype(hist, float64)
        hist = divide(counts, multiply(sum(counts), widths))
    return hist, bin_edges


def _var_std(x, axis, correction, keepdims, use_new_impl, sqrt):
    if x.dtype not in _real_floating_dtypes:
        raise TypeError(f"Only real floating-point dtypes are allowed in {'std' if sqrt else 'var'}")
    intermediate_dtype = [("n", np.int64), ("mu", np.float64), ("M2", np.float64)]
    return reduction(x, _var_func, combine_func=_var_combine,
                     aggegrate_func=_VarAggregate(correction, sqrt), axis=axis,
                     intermediate_dtype=intermediate_dtype, dtype=x.dtype, keepdims=keepdims,
                     use_new_impl=use_new_impl, extra_func_kwargs=dict(dtype=intermediate_dtype))


def var(x, /, *, axis=None, correction=0.0, keepdims=False, use_new_impl=False):
    """Array API ``var`` (not in the reference v0.12.0, api_status.md:74):
    one fused pass of the {n, mu, M2} triple reduction (Welford per element,
    Chan's update across chunks, merge rounds and GPUs) in f64, then
    M2 / max(n - correction, 0), cast to x's dtype.  Matches numpy's
    ``var(ddof=correction)`` computed in f64."""
    return _var_std(x, axis, correction, keepdims, use_new_impl, sqrt=False)


def std(x, /, *, axis=None, correction=0.0, keepdims=False, use_new_impl=False):
    """Array API ``std`` (api_status.md:72): the square root of ``var``'s
    aggregate, same single pass."""
    return _var_std(x, axis, correction, keepdims, use_new_impl, sqrt=True)
