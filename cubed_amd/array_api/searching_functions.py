from ..core.ops import arg_reduction, elemwise
from .data_type_functions import result_type


def argmax(x, /, *, axis=None, keepdims=False):
    return arg_reduction(x, "argmax", axis=axis, keepdims=keepdims)


def argmin(x, /, *, axis=None, keepdims=False):
    return arg_reduction(x, "argmin", axis=axis, keepdims=keepdims)


def where(condition, x1, x2, /):
    """elemwise(where, condition, x1, x2) (searching_functions.py:30-32)."""
    dtype = result_type(x1, x2)
    return elemwise("where", condition, x1, x2, dtype=dtype)


def nonzero(x, /):
    """The indices of the elements of ``x`` that are not zero: a tuple of
    ``x.ndim`` int64 1-d arrays, in C order -- ``np.nonzero(x)``.  bool, every
    integer width, float32, float64 and bfloat16; -0.0 is zero, NaNs of either
    sign, infinities and denormals are not.  A 0-d ``x`` raises ValueError and a
    complex one TypeError.

    The reference has no nonzero, so parity is unpinned; numpy is the
    yardstick.  The shape of the result depends on the data, so the function is
    EAGER like ``unique_values``: while the call executes it counts the
    selected elements of every chunk of the flattened ``x`` and packs their
    flat positions (``core.ops.select_count`` / ``select_pack``) on
    ``x.spec.executor`` and reads the counts to the host.  The arrays returned
    are lazy and start from the packed positions in HBM; for ``ndim > 1`` they
    are ``(pos // stride_d) % shape_d`` of the flat positions.  One GPU.  To
    only count, use ``count_nonzero``, which is lazy."""
    import math

    from ..core.ops import select_nonzero
    from .creation_functions import empty
    from .dtypes import _real_numeric_dtypes, bool as _bool, int64
    from .manipulation_functions import _ravel

    if x.dtype not in _real_numeric_dtypes and x.dtype != _bool:
        raise TypeError("Only boolean and real numeric dtypes are allowed in nonzero")
    if x.ndim == 0:
        raise ValueError("nonzero is not supported for zero-dimensional arrays; use "
                         "nonzero(reshape(x, (1,))) instead")
    pos = select_nonzero(_ravel(x)) if x.size else None
    if pos is None:
        return tuple(empty((0,), dtype=int64, chunks=(1,), spec=x.spec) for _ in range(x.ndim))
    if x.ndim == 1:
        return (pos,)
    out = []
    for d in range(x.ndim):
        stride = math.prod(x.shape[d + 1:])
        idx = pos if d == x.ndim - 1 else pos // stride
        out.append(idx if d == 0 else idx % int(x.shape[d]))
    return tuple(out)


def count_nonzero(x, /, *, axis=None, keepdims=False):
    """The int64 number of elements of ``x`` that are not zero, over ``axis``
    (an int, a tuple of ints or None for all) -- ``np.count_nonzero`` (Array
    API 2024.12).  Lazy and of a shape that does not depend on the data: the
    ``sum`` of ``astype(x != 0, int64)``; nothing runs on the select kernel."""
    from .data_type_functions import astype
    from .dtypes import bool as _bool, int64
    from .statistical_functions import sum as _sum

    flags = x if x.dtype == _bool else x != 0
    return _sum(astype(flags, int64), axis=axis, dtype=int64, keepdims=keepdims)


def searchsorted(x1, x2, /, *, side="left", sorter=None):
    """For every element ``v`` of ``x2`` (any shape) the index at which it
    would be inserted into the sorted 1-d ``x1`` to keep it sorted: the number
    of elements of ``x1`` that sort strictly before ``v`` (``side="left"``) or
    before or tied with ``v`` (``side="right"``), as int64 with the shape and
    chunks of ``x2`` -- ``np.searchsorted(x1, x2, side)``.

    ``x1`` ascends in the order of ``sort``: every NaN after every number and
    all NaNs tied, -0.0 and 0.0 tied.  The dtypes are those ``sort`` accepts;
    ``x1`` and ``x2`` are promoted together by ``result_type`` (whose errors
    stay: int32 with float32, int64 with uint64) and bool and narrow integers
    are then widened exactly.

    ``sorter``, if given, is an int64 array of ``x1``'s shape and ``x1`` becomes
    ``take(x1, sorter, axis=0)``.  ``take`` evaluates an array index eagerly,
    while the plan is built, so ``sorter`` is computed then.

    The reference has no searchsorted, so parity is unpinned; numpy is the
    yardstick.  ``x1`` in ``nb`` blocks costs ``nb`` passes over ``x2`` (see
    ``core.ops.searchsorted``); no task reads more than three chunks."""
    import numpy as np

    from ..core.ops import searchsorted as _searchsorted
    from .creation_functions import empty, zeros
    from .data_type_functions import astype
    from .dtypes import int64
    from .indexing_functions import take
    from .sorting_functions import _KEY_DTYPE

    for x in (x1, x2):
        if np.dtype(x.dtype) not in _KEY_DTYPE:
            raise TypeError("Only boolean, integer, float32 and float64 dtypes are allowed in searchsorted")
    if x1.ndim != 1:
        raise ValueError(f"searchsorted: x1 must be one-dimensional, not {x1.ndim}-d")
    if side not in ("left", "right"):
        raise ValueError(f"searchsorted: side must be 'left' or 'right', not {side!r}")
    key_dtype = _KEY_DTYPE[np.dtype(result_type(x1, x2))]
    if sorter is not None:
        if np.dtype(sorter.dtype) != np.dtype(int64) or sorter.shape != x1.shape:
            raise ValueError("searchsorted: sorter must be an int64 array of x1's shape")
        x1 = take(x1, sorter, axis=0)
    if x2.size == 0:
        return empty(x2.shape, dtype=int64, chunks=x2.chunks, spec=x2.spec)
    if x1.size == 0:
        return zeros(x2.shape, dtype=int64, chunks=x2.chunks, spec=x2.spec)
    return _searchsorted(astype(x1, key_dtype, copy=False), astype(x2, key_dtype, copy=False), side == "right")
