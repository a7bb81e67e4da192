"""Array API set functions (2022.12).  The reference has none of them, so
parity is unpinned; numpy is the yardstick: with ``f = x.ravel()`` the results
are those of ``np.unique(f, return_index=True, return_inverse=True,
return_counts=True)`` with numpy's default ``equal_nan=True``.

All NaNs are ONE value, which comes last.  The Array API wants every NaN to be
distinct; this project follows its own sort order (NaNs last and tied) and
numpy's default instead.  -0.0 and 0.0 are one value too; the representative
returned is the first occurrence in C order (the sort is stable), and so is
``indices``.

The shape of the results depends on the data, so these functions are EAGER:
while the call executes they run the first part of the plan -- the sort, the
count of the run heads per chunk and their packing -- on ``x.spec.executor``,
as ``index()`` does for an array index, and read the per-chunk counts to the
host.  What they return is lazy again: it starts from the packed arrays that
are already in HBM (``core.ops.from_device``) and never sorts a second time."""

from collections import namedtuple

import numpy as np

from .dtypes import int64
from .manipulation_functions import _ravel  # noqa: F401  (shared with nonzero and x[mask])

UniqueAllResult = namedtuple("UniqueAllResult", ["values", "indices", "inverse_indices", "counts"])
UniqueCountsResult = namedtuple("UniqueCountsResult", ["values", "counts"])
UniqueInverseResult = namedtuple("UniqueInverseResult", ["values", "inverse_indices"])


def _unique(x, what, index=False, inverse=False, counts=False):
    """(values, indices, inverse_indices, counts); the ones not asked for are
    None."""
    from ..core.array import compute
    from ..core.ops import from_device, rechunk, searchsorted, unique_count, unique_gather, unique_pack
    from ..core.ops import sort as _sort
    from .creation_functions import asarray, empty
    from .data_type_functions import astype
    from .manipulation_functions import concat
    from .sorting_functions import _KEY_DTYPE

    key_dtype = _KEY_DTYPE.get(np.dtype(x.dtype))
    if key_dtype is None:
        raise TypeError(f"Only boolean, integer, float32 and float64 dtypes are allowed in {what}")
    spec = x.spec
    n = x.size
    if n == 0:
        none = empty((0,), dtype=int64, chunks=(1,), spec=spec)
        return (empty((0,), dtype=x.dtype, chunks=(1,), spec=spec), none if index else None,
                empty(x.shape, dtype=int64, chunks=x.chunks, spec=spec) if inverse else None,
                none if counts else None)

    # ---- phase 1, computed now: sort, count the run heads, pack them
    xk = astype(x, key_dtype, copy=False)
    f = _ravel(xk)
    s = _sort(f, 0, False, index, index)  # {v, i} pairs when the first occurrences are wanted
    head_counts = unique_count(s, index)
    packs = {}
    if index:
        packs["index"] = unique_pack(s, True, "index")
    if counts:
        packs["position"] = unique_pack(s, index, "position")
    if not packs:
        packs["keys"] = unique_pack(s, False, None)
    compute(head_counts, *packs.values(), _return_in_memory_array=False)
    per_chunk = head_counts._read_stored()
    k = int(per_chunk.sum())

    # ---- phase 2, lazy: gather the heads, starting from the packed arrays in HBM
    packed = {name: from_device(p.zarray, spec) for name, p in packs.items()}
    name = next(iter(packed))
    values_key = unique_gather(packed[name], per_chunk, None if name == "keys" else "v")
    values = astype(values_key, x.dtype, copy=False)
    indices = unique_gather(packed["index"], per_chunk, "i") if index else None
    inverse_indices = searchsorted(values_key, xk, False) if inverse else None
    run_lengths = None
    if counts:
        # a run ends where the next one starts; the last one at n
        pos = unique_gather(packed["position"], per_chunk, "i")
        end = asarray(np.array([n], dtype=np.int64), chunks=(1,), spec=spec)
        nxt = end if k == 1 else rechunk(concat([pos[1:], end]), pos.chunksize)
        run_lengths = nxt - pos
    return values, indices, inverse_indices, run_lengths


def unique_values(x, /):
    """The distinct elements of ``x`` (any shape), ascending, 1-d with
    ``x.dtype``: ``np.unique(x)``.  All NaNs are one value, the last (numpy's
    ``equal_nan=True``, not the Array API's distinct NaNs); -0.0 and 0.0 are
    one value, returned as the first of them in C order.  Eager: the sort and
    the compaction run on ``x.spec.executor`` while the call executes; the
    result is lazy and starts from the packed heads in HBM.  bool and narrow
    integers are widened exactly and cast back; bfloat16 and complex raise
    TypeError.  One GPU."""
    return _unique(x, "unique_values")[0]


def unique_counts(x, /):
    """``(values, counts)``: ``unique_values(x)`` and, int64 of the same shape
    and chunks, how often each occurs -- ``np.unique(x, return_counts=True)``;
    the one NaN entry counts every NaN.  Eager like ``unique_values``."""
    values, _, _, counts = _unique(x, "unique_counts", counts=True)
    return UniqueCountsResult(values, counts)


def unique_inverse(x, /):
    """``(values, inverse_indices)``: ``unique_values(x)`` and, int64 with
    ``x``'s shape and chunks, the position of every element of ``x`` in
    ``values`` -- ``np.unique(x, return_inverse=True)``; every NaN maps to the
    one NaN entry.  Eager like ``unique_values``."""
    values, _, inverse, _ = _unique(x, "unique_inverse", inverse=True)
    return UniqueInverseResult(values, inverse)


def unique_all(x, /):
    """``(values, indices, inverse_indices, counts)``: ``np.unique(x.ravel(),
    return_index=True, return_inverse=True, return_counts=True)``.  ``indices``
    (int64, ``values``' shape and chunks) are the first occurrences in C
    order: the sort is stable.  Eager like ``unique_values``."""
    return UniqueAllResult(*_unique(x, "unique_all", index=True, inverse=True, counts=True))
