"""take (array_api/indexing_functions.py:1-2): an integer-list index along
one axis, lowered like any other index region.  take_along_axis (Array API
2024.12; the reference notes its absence, core/ops.py:1124,1145): a lazy int64
index array applied along one axis on the device."""


def take(x, indices, /, *, axis):
    return x[(slice(None),) * axis + (indices,)]


def take_along_axis(x, indices, /, *, axis=-1):
    """``np.take_along_axis(x, indices, axis)``: the element of ``x`` that
    ``indices`` names along ``axis`` at every place of ``indices``, moved as
    bits (NaN payloads and -0.0 survive).

    ``x`` and ``indices`` have the same number of dimensions, at least one,
    and the same extent in every dimension but ``axis`` (numpy would broadcast
    them; that is not implemented).  Along ``axis`` ``indices`` may have any
    extent.  The result has the shape of ``indices``, the dtype of ``x``, the
    chunk length of ``indices`` along ``axis`` and the chunks of ``x``
    elsewhere; ``indices`` is rechunked to those if it has others.

    ``x``: bool, any integer, bfloat16, float32 or float64 (complex raises
    ``TypeError``).  ``indices``: any integer dtype, widened to int64 (uint64
    is read as int64); bool and floating indices raise ``TypeError``.  With
    ``n = x.shape[axis]`` an index ``-n <= i < 0`` means ``i + n``.

    **Out-of-range indices.**  The call is lazy, so it cannot raise numpy's
    ``IndexError``: an index outside ``[-n, n)`` gives a zero element, and
    never an access outside a chunk.  A nonempty ``indices`` over ``n == 0``
    does raise ``IndexError``, when the call is made.

    ``x`` in ``nb`` blocks along ``axis`` costs ``nb`` passes over ``indices``
    (see ``core.ops.take_along_axis``); no task reads more than three chunks."""
    import numpy as np

    from ..core.array import CoreArray
    from ..core.ops import from_array, rechunk, validate_axis
    from ..core.ops import take_along_axis as _take_along_axis
    from .creation_functions import empty
    from .data_type_functions import astype
    from .dtypes import int64

    xdtype = np.dtype(x.dtype)
    if xdtype.names or xdtype.kind == "c" or xdtype.itemsize not in (1, 2, 4, 8):
        raise TypeError(f"take_along_axis of a {xdtype} array is not supported")
    if not isinstance(indices, (CoreArray, np.ndarray)):
        raise TypeError("take_along_axis: indices must be an array")
    if np.dtype(indices.dtype).kind not in "iu":
        raise TypeError(f"take_along_axis: indices must have an integer dtype, not {np.dtype(indices.dtype)}")
    if isinstance(axis, (tuple, list)):
        raise TypeError("take_along_axis takes a single axis")
    if x.ndim != indices.ndim:
        raise ValueError(f"take_along_axis: x has {x.ndim} dimensions and indices {indices.ndim}; they must match")
    if x.ndim == 0:
        raise ValueError("take_along_axis: x must have at least one dimension")
    axis = validate_axis(axis, x.ndim)
    off = [d for d in range(x.ndim) if d != axis]
    if any(x.shape[d] != indices.shape[d] for d in off):
        raise NotImplementedError(
            f"take_along_axis: indices of shape {tuple(indices.shape)} over x of shape {tuple(x.shape)} along axis "
            f"{axis}: numpy would broadcast the other dimensions, which is not supported; they must be equal")
    if isinstance(indices, np.ndarray):
        chunks = tuple(indices.shape[d] if d == axis else x.chunksize[d] for d in range(x.ndim))
        indices = from_array(indices, chunks=chunks, spec=x.spec)
    if indices.size == 0:
        chunks = tuple(indices.chunks[d] if d == axis else x.chunks[d] for d in range(x.ndim))
        return empty(indices.shape, dtype=x.dtype, chunks=chunks, spec=x.spec)
    if x.shape[axis] == 0:
        raise IndexError(f"take_along_axis: cannot index axis {axis} of extent 0 with a nonempty indices array")
    if any(indices.chunks[d] != x.chunks[d] for d in off):
        indices = rechunk(indices, tuple(indices.chunksize[d] if d == axis else x.chunksize[d]
                                         for d in range(x.ndim)))
        if any(indices.chunks[d] != x.chunks[d] for d in off):
            raise NotImplementedError("take_along_axis: x has irregular chunks that indices cannot be rechunked to")
    return _take_along_axis(x, astype(indices, int64, copy=False), axis)
