"""Array API sorting functions (2022.12).  The reference has neither (its
api_status.md lists both as missing), so parity is unpinned; the semantics are
numpy's stable sort."""

import numpy as np

from ..core.ops import sort as _sort
from ..core.ops import validate_axis
from .dtypes import (
    bool as _bool,
    float32,
    float64,
    int8,
    int16,
    int32,
    int64,
    uint8,
    uint16,
    uint32,
    uint64,
)

# the kernels' key types; narrower integers and bool are widened (exactly)
_KEY_DTYPE = {
    _bool: int32, int8: int32, int16: int32, int32: int32, int64: int64,
    uint8: uint32, uint16: uint32, uint32: uint32, uint64: uint64,
    float32: float32, float64: float64,
}


def _sorted(x, axis, descending, pairs, what):
    from .creation_functions import empty
    from .data_type_functions import astype

    key_dtype = _KEY_DTYPE.get(np.dtype(x.dtype))
    if key_dtype is None:
        raise TypeError(f"Only boolean, integer, float32 and float64 dtypes are allowed in {what}")
    axis = validate_axis(axis, x.ndim)
    if isinstance(axis, tuple):
        raise TypeError(f"{what} takes a single axis")
    if x.size == 0:
        if not pairs:
            return x
        return empty(x.shape, dtype=int64, chunks=x.chunks, spec=x.spec)
    result = _sort(astype(x, key_dtype, copy=False), axis, bool(descending), pairs)
    return result if pairs else astype(result, x.dtype, copy=False)


def sort(x, /, *, axis=-1, descending=False, stable=True):
    """``x`` sorted along ``axis``, same shape, chunks and dtype.  Values
    ascend; every NaN is greater than every number (all NaNs tie, as do -0.0
    and 0.0); ``descending`` reverses that order, so NaNs come first.  The
    result is always stable (``stable=False`` behaves identically)."""
    return _sorted(x, axis, descending, False, "sort")


def argsort(x, /, *, axis=-1, descending=False, stable=True):
    """The int64 indices along ``axis`` that sort ``x`` in the order of
    ``sort``.  Ties go to the smaller index, ascending and descending, so the
    result is always stable (``stable=False`` behaves identically)."""
    return _sorted(x, axis, descending, True, "argsort")
