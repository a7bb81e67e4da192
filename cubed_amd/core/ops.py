"""Core ops: the public blockwise / reduction / rechunk API.

Mirrors cubed/core/ops.py (from_array :40, blockwise :185-302,
general_blockwise :305-356, elemwise :359-371, index :374-517, map_blocks
:520-643, map_direct :646-699, rechunk :702-758, merge_chunks :761-787,
reduction :790-903, reduction_new/partial_reduce/tree_reduce :906-1090,
squeeze :1156, unify_chunks :1172-1219) with the same signatures, chunk
inference, projected-memory errors and reduction rounds.  What changes is the
chunk function: each op attaches an IR program (cubed_amd/ir.py) so the
MI355X executor can lower the pipeline to one kernel launch.
"""

from __future__ import annotations

import builtins
import math
import numbers
from functools import partial
from itertools import product
from numbers import Integral, Number
from typing import TYPE_CHECKING, Any, Sequence, Union

import numpy as np

from .. import ir
from ..chunkfuncs import ChunkMap, ChunkReduction, as_chunk_reduction
from ..primitive.blockwise import blockwise as primitive_blockwise
from ..primitive.blockwise import general_blockwise as primitive_general_blockwise
from ..primitive.rechunk import rechunk as primitive_rechunk
from ..storage import DeviceArray, HostArray
from ..utils import (
    chunk_memory,
    common_blockdim,
    get_item,
    normalize_chunks,
    offset_to_block_id,
    to_chunksize,
)
from .array import CoreArray, check_array_specs, compute, gensym
from .plan import Plan, new_temp_path

if TYPE_CHECKING:
    from ..array_api.array_object import Array


def _Array():
    from ..array_api.array_object import Array

    return Array


# ------------------------------------------------------------------ sources


def from_array(x, chunks="auto", asarray=None, spec=None) -> "Array":
    """Create an array from an in-memory array-like; chunks are uploaded to
    HBM by the executor (reference: map_blocks(_from_array), core/ops.py:40-85)."""
    if isinstance(x, CoreArray):
        raise ValueError("Array is already a Cubed array. Use 'asarray' or 'rechunk' instead.")
    from ..ir import check_input_dtype

    check_input_dtype(x.dtype)
    previous_chunks = getattr(x, "chunks", None)
    outchunks = normalize_chunks(chunks, x.shape, dtype=x.dtype, previous_chunks=previous_chunks)
    host = HostArray(np.asarray(x) if (asarray or asarray is None) else x, to_chunksize(outchunks) if x.ndim else ())
    name = gensym()
    from .array import CoreArray as _CA  # noqa: F401

    spec = spec or _default_spec()
    target = DeviceArray(x.shape, x.dtype, to_chunksize(outchunks) if x.ndim else (), name=name)
    op = upload_op(host, target, spec)
    plan = Plan._new(name, "from_array", target, op, False)
    return _Array()(name, target, spec, plan)


def _default_spec():
    from ..spec import Spec

    return Spec(None, allowed_mem=200_000_000, reserved_mem=100_000_000)


def upload_stage(item, *, config=None):
    raise TypeError("uploads run only through the MI355X executor")


class UploadSpec:
    def __init__(self, source: HostArray, target: DeviceArray):
        self.source = source
        self.target = target


def upload_op(host: HostArray, target: DeviceArray, spec):
    from ..primitive.types import PrimitiveOperation
    from ..runtime.types import CubedPipeline

    pipeline = CubedPipeline(upload_stage, gensym("upload"), [], UploadSpec(host, target))
    projected = spec.reserved_mem + 2 * chunk_memory(target.dtype, target.chunks)
    return PrimitiveOperation(pipeline=pipeline, target_array=target, projected_mem=projected,
                              allowed_mem=spec.allowed_mem, reserved_mem=spec.reserved_mem,
                              num_tasks=target.nchunks, fusable=False)


def from_zarr(store, spec=None) -> "Array":
    from .. import zarr_io

    return zarr_io.from_zarr(store, spec=spec)


def store(sources, targets, executor=None, **kwargs):
    from .. import zarr_io

    return zarr_io.store(sources, targets, executor=executor, **kwargs)


def to_zarr(x, store, executor=None, **kwargs):
    from .. import zarr_io

    return zarr_io.to_zarr(x, store, executor=executor, **kwargs)


# ------------------------------------------------------------------ lowering of callables


def _lower_callable(func, arrays, inds, out_ind, dtype, kwargs):
    """IR program for ``func`` called on chunks of ``arrays`` laid out by
    ``inds`` in the output space ``out_ind``.  Numpy ufuncs lower to
    expressions; everything else becomes an OpaqueProgram (the executor then
    refuses the plan)."""
    if isinstance(func, ir.Program):
        return func
    if isinstance(func, _BlockIdFunc):
        # the last argument is the block-offsets array map_blocks appended
        meta = tuple((np.dtype(a.dtype), a.ndim) for a in arrays[:-1])
        return ir.PerBlockProgram(func=func.func, kwargs=dict(kwargs), args_meta=meta,
                                  inds=tuple(inds[:-1]), out_ind=tuple(out_ind), dtype=dtype,
                                  nargs=len(arrays))
    if isinstance(func, partial) and not func.args:
        base = func.func
        kwargs = {**func.keywords, **kwargs}
    else:
        base = func
    name = ir.NUMPY_ELEMENTWISE.get(base)
    if name is not None and not kwargs:
        space = len(out_ind)
        pos = {idx: i for i, idx in enumerate(out_ind)}
        args = []
        for i, (a, ind) in enumerate(zip(arrays, inds)):
            if ind is None or any(idx not in pos for idx in ind):
                return ir.OpaqueProgram(func=func, nargs=len(arrays))
            args.append(ir.Arg(i, a.dtype, tuple(pos[idx] for idx in ind)))
        try:
            e = ir.apply_op(name, args, dtype)
        except NotImplementedError:
            return ir.OpaqueProgram(func=func, nargs=len(arrays))
        return ir.ExprProgram(ndim=space, nargs=len(args), outputs=e,
                              out_axes=tuple(range(space)), name=name)
    # a numpy reduction applied per chunk with keepdims (map_blocks(np.max,
    # x, axis=0, keepdims=True)): the per-chunk reduce program of reduction()
    red = as_chunk_reduction(base)
    if red is not None and len(arrays) == 1 and kwargs.get("keepdims") and \
            set(kwargs) <= {"axis", "keepdims", "dtype"} and tuple(inds[0] or ()) == tuple(out_ind):
        ax = kwargs.get("axis")
        nd = arrays[0].ndim
        ax = tuple(range(nd)) if ax is None else tuple(a % nd for a in (ax if isinstance(ax, tuple) else (ax,)))
        extra = {"dtype": kwargs["dtype"]} if kwargs.get("dtype") is not None else {}
        try:
            return red.program(nd, arrays[0].dtype, ax, keepdims=True, **extra)
        except (NotImplementedError, TypeError, ValueError):
            pass
    from ..tracing import trace_callable

    traced = trace_callable(func, arrays, inds, out_ind, dtype, kwargs)
    if traced is not None:
        return traced
    return ir.OpaqueProgram(func=func, nargs=len(arrays))


# ------------------------------------------------------------------ blockwise


def blockwise(func, out_ind, *args: Any, dtype=None, adjust_chunks=None, new_axes=None,
              align_arrays=True, target_store=None, extra_func_kwargs=None, **kwargs) -> "Array":
    arrays = args[::2]
    assert len(arrays) > 0
    new_axes = new_axes or {}
    new = (set(out_ind) - {a for arg in args[1::2] if arg is not None for a in arg}
           - set(new_axes or ()))
    if new:
        raise ValueError("Unknown dimension", new)
    if align_arrays:
        chunkss, arrays = unify_chunks(*args)
    else:
        chunkss = {}
        for arg, ind in zip(arrays, args[1::2]):
            arg_chunks = normalize_chunks(arg.chunks, shape=arg.shape, dtype=arg.dtype)
            for c, i in zip(arg_chunks, ind):
                if i not in chunkss or len(c) > len(chunkss[i]):
                    chunkss[i] = c
    for k, v in new_axes.items():
        if not isinstance(v, tuple):
            v = (v,)
        chunkss[k] = v
    chunks = [chunkss[i] for i in out_ind]
    if adjust_chunks:
        for i, ind in enumerate(out_ind):
            if ind in adjust_chunks:
                aj = adjust_chunks[ind]
                if callable(aj):
                    chunks[i] = tuple(map(aj, chunks[i]))
                elif isinstance(aj, numbers.Integral):
                    chunks[i] = tuple(aj for _ in chunks[i])
                elif isinstance(aj, (tuple, list)):
                    if len(aj) != len(chunks[i]):
                        raise ValueError(
                            f"Dimension {i} has {len(chunks[i])} blocks, adjust_chunks "
                            f"specified with {len(aj)} blocks")
                    chunks[i] = tuple(aj)
                else:
                    raise NotImplementedError("adjust_chunks values must be callable, int, or tuple")
    _chunks = tuple(chunks)
    shape = tuple(map(sum, _chunks))

    zargs = list(args)
    zargs[::2] = [a.zarray_maybe_lazy for a in arrays]
    in_names = [a.name for a in arrays]
    extra_source_arrays = kwargs.pop("extra_source_arrays", [])
    source_arrays = list(arrays) + list(extra_source_arrays)
    extra_projected_mem = kwargs.pop("extra_projected_mem", 0)
    fusable = kwargs.pop("fusable", True)

    program = _lower_callable(func, arrays, args[1::2], out_ind, dtype,
                              {**kwargs, **(extra_func_kwargs or {})})
    name = gensym()
    spec = check_array_specs(arrays)
    if target_store is None:
        target_store = new_temp_path(name=name, spec=spec)
    op = primitive_blockwise(
        program, out_ind, *zargs, allowed_mem=spec.allowed_mem, reserved_mem=spec.reserved_mem,
        extra_projected_mem=extra_projected_mem, target_store=target_store, shape=shape,
        dtype=dtype, chunks=_chunks, new_axes=new_axes, in_names=in_names, out_name=name,
        extra_func_kwargs=extra_func_kwargs, fusable=fusable)
    if isinstance(op.target_array, DeviceArray):
        op.target_array.name = name
    plan = Plan._new(name, "blockwise", op.target_array, op, False, *source_arrays)
    return _Array()(name, op.target_array, spec, plan)


def general_blockwise(func, block_function, *arrays, shape, dtype, chunks, target_store=None,
                      extra_func_kwargs=None, **kwargs) -> "Array":
    assert len(arrays) > 0
    zargs = [a.zarray_maybe_lazy for a in arrays]
    in_names = [a.name for a in arrays]
    extra_source_arrays = kwargs.pop("extra_source_arrays", [])
    source_arrays = list(arrays) + list(extra_source_arrays)
    extra_projected_mem = kwargs.pop("extra_projected_mem", 0)
    fusable = kwargs.pop("fusable", True)
    name = gensym()
    spec = check_array_specs(arrays)
    if target_store is None:
        target_store = new_temp_path(name=name, spec=spec)
    program = func if isinstance(func, ir.Program) else ir.OpaqueProgram(func=func, nargs=len(arrays))
    op = primitive_general_blockwise(
        program, block_function, *zargs, allowed_mem=spec.allowed_mem,
        reserved_mem=spec.reserved_mem, extra_projected_mem=extra_projected_mem,
        target_store=target_store, shape=shape, dtype=dtype, chunks=chunks, in_names=in_names,
        extra_func_kwargs=extra_func_kwargs, fusable=fusable)
    if isinstance(op.target_array, DeviceArray):
        op.target_array.name = name
    plan = Plan._new(name, "blockwise", op.target_array, op, False, *source_arrays)
    return _Array()(name, op.target_array, spec, plan)


def elemwise(func, *args: "Array", dtype=None) -> "Array":
    """Apply an elementwise op to broadcast array arguments.  ``func`` is an
    op name (ir.UNARY_OPS / ir.BINARY_OPS / "where") or a numpy ufunc."""
    shapes = [arg.shape for arg in args]
    out_ndim = len(np.broadcast_shapes(*shapes))
    expr_inds = tuple(range(out_ndim))[::-1]
    if dtype is None:
        raise ValueError("dtype must be specified for elemwise")
    opname = func if isinstance(func, str) else ir.NUMPY_ELEMENTWISE.get(func)
    if opname is not None:
        program = ir.elementwise_program(opname, [a.dtype for a in args],
                                         [a.ndim for a in args], dtype)
    else:
        program = func
    pairs = []
    for a in args:
        pairs += [a, tuple(range(a.ndim)[::-1])]
    return blockwise(program, expr_inds, *pairs, dtype=dtype)


# ------------------------------------------------------------------ index


def _is_int(x):
    return isinstance(x, (Integral, np.integer)) and not isinstance(x, bool)


def index(x, key):
    """Subset an array along one or more axes (basic indexing: slices with
    step >= 1, integers, None, Ellipsis, and one integer list), or select
    the elements under a boolean mask of ``x``'s shape (the sole index; eager,
    see ``_index_mask``)."""
    if _is_bool_key(key):
        return _index_mask(x, key)
    if not isinstance(key, tuple):
        key = (key,)
    if any(_is_bool_key(ind) for ind in key):
        # never read a boolean array as integer indices
        raise NotImplementedError("a boolean array index next to other indices is not supported: "
                                  "a boolean mask must be the sole index and have the array's shape")
    if all(isinstance(ind, slice) and ind == slice(None) for ind in key):
        return x
    where_none = [i for i, ind in enumerate(key) if ind is None]
    for i, a in enumerate(where_none):
        n = sum(_is_int(ind) for ind in key[:a])
        if n:
            where_none[i] -= n
    key = tuple(ind for ind in key if ind is not None)
    selection = tuple(
        s.compute().tolist() if isinstance(s, CoreArray) else s for s in key)
    selection = tuple(s.tolist() if isinstance(s, np.ndarray) else s for s in selection)
    # replace ellipsis
    if any(s is Ellipsis for s in selection):
        i = [k for k, s in enumerate(selection) if s is Ellipsis][0]
        n_missing = x.ndim - (len(selection) - 1)
        selection = selection[:i] + (slice(None),) * n_missing + selection[i + 1:]
    selection = selection + (slice(None),) * (x.ndim - len(selection))
    if any(isinstance(s, slice) and s.step is not None and s.step < 1 for s in selection):
        raise NotImplementedError(f"Slice step must be >= 1: {key}")
    if sum(isinstance(s, list) for s in selection) > 1:
        raise NotImplementedError("Only one integer array index is allowed.")

    # normalized selection + output geometry (zarr OrthogonalIndexer semantics)
    norm = []
    shape, chunks, merged = [], [], []
    for d, s in enumerate(selection):
        n = x.shape[d]
        dcl = x.chunksize[d]
        if isinstance(s, slice):
            start, stop, step = s.indices(n)
            length = max(0, (stop - start + (step - 1)) // step)
            norm.append(slice(start, stop, step))
            shape.append(length)
            cl = max(dcl // step, 1)
            chunks.append(cl)
            if step == 1 or dcl // step < 1:
                merged.append(dcl)
            else:
                merged.append((dcl // step) * step)
        elif isinstance(s, list):
            lst = [int(v) + n if int(v) < 0 else int(v) for v in s]
            norm.append(lst)
            shape.append(len(lst))
            chunks.append(dcl)
            merged.append(dcl)
        elif _is_int(s):
            v = int(s)
            if v < 0:
                v += n
            if not 0 <= v < n:
                raise IndexError(f"index {s} is out of bounds for axis {d} with size {n}")
            norm.append(v)
        else:
            raise NotImplementedError(f"unsupported index {s!r}")
    shape = tuple(shape)
    target_chunks = normalize_chunks(tuple(chunks), shape, dtype=x.dtype)
    extra_projected_mem = x.chunkmem
    out = map_direct(
        _read_index_region(norm, target_chunks), x, shape=shape, dtype=x.dtype,
        chunks=target_chunks, extra_projected_mem=extra_projected_mem,
        target_chunks=target_chunks, selection=tuple(norm))
    merged = tuple(merged)
    if tuple(chunks) != merged:
        out = merge_chunks(out, merged)
    for axis in where_none:
        from ..array_api.manipulation_functions import expand_dims

        out = expand_dims(out, axis=axis)
    return out


class _read_index_region:
    """Region of ``x`` that output block ``block_id`` of ``x[selection]``
    reads (core/ops.py:489-517 _target_chunk_selection)."""

    def __init__(self, selection, target_chunks):
        self.selection = selection
        self.target_chunks = target_chunks

    def __call__(self, block_id):
        sel = []
        i = 0
        for s in self.selection:
            if isinstance(s, slice):
                starts = [s.start]
                for c in self.target_chunks[i]:
                    starts.append(starts[-1] + c * s.step)
                j = block_id[i]
                sel.append(slice(starts[j], starts[j + 1], s.step))
                i += 1
            elif isinstance(s, list):
                st = [0]
                for c in self.target_chunks[i]:
                    st.append(st[-1] + c)
                j = block_id[i]
                sel.append(s[st[j]:st[j + 1]])
                i += 1
            else:
                sel.append(s)
        return tuple(sel)


# ------------------------------------------------------------------ map_blocks


class _BlockIdProgram:
    """Marker for program builders that need the task's block id: the
    builder gets ``block_arg`` = index of the offsets argument."""

    def __init__(self, build, nargs_without_offsets):
        self.build = build
        self.nargs = nargs_without_offsets


def map_blocks(func, *args: "Array", dtype=None, chunks=None, drop_axis=[], new_axis=None,
               spec=None, **kwargs) -> "Array":
    """Apply a function to corresponding blocks from multiple input arrays."""
    if len(args) == 0:
        from ..array_api.creation_functions import empty_virtual_array

        shape = tuple(map(sum, chunks))
        args = (empty_virtual_array(shape, dtype=dtype, chunks=chunks, spec=spec),)
    if isinstance(func, _BlockIdProgram) or _has_block_id(func):
        from ..array_api.creation_functions import offsets_virtual_array

        arg0 = args[0]
        offsets = offsets_virtual_array(arg0.numblocks, arg0.spec)
        new_args = args + (offsets,)
        if isinstance(func, _BlockIdProgram):
            func = func.build(len(args))
        else:
            func = _BlockIdFunc(func)
        return _map_blocks(func, *new_args, dtype=dtype, chunks=chunks, drop_axis=drop_axis,
                           new_axis=new_axis, **kwargs)
    return _map_blocks(func, *args, dtype=dtype, chunks=chunks, drop_axis=drop_axis,
                       new_axis=new_axis, **kwargs)


class _BlockIdFunc:
    """A user function taking ``block_id``: lowered per block (PerBlockProgram)."""

    def __init__(self, func):
        self.func = func


def _has_block_id(func) -> bool:
    import inspect

    if isinstance(func, (ir.Program, ChunkMap, ChunkReduction)):
        return False
    try:
        return "block_id" in inspect.signature(func).parameters
    except (TypeError, ValueError):
        return False


def _map_blocks(func, *args: "Array", dtype=None, chunks=None, drop_axis=[], new_axis=None,
                **kwargs) -> "Array":
    new_axes = {}
    if isinstance(drop_axis, Number):
        drop_axis = [drop_axis]
    if isinstance(new_axis, Number):
        new_axis = [new_axis]
    arrs = args
    argpairs = [(a, tuple(range(a.ndim))[::-1]) if isinstance(a, CoreArray) else (a, None)
                for a in args]
    out_ind = tuple(range(max(a.ndim for a in arrs)))[::-1] if arrs else ()
    if drop_axis:
        ndim_out = len(out_ind)
        if any(i < -ndim_out or i >= ndim_out for i in drop_axis):
            raise ValueError(f"drop_axis out of range (drop_axis={drop_axis}, but output is {ndim_out}d).")
        drop_axis = [i % ndim_out for i in drop_axis]
        out_ind = tuple(x for i, x in enumerate(out_ind) if i not in drop_axis)
    if new_axis is None and chunks is not None and len(out_ind) < len(chunks):
        new_axis = range(len(chunks) - len(out_ind))
    if new_axis:
        temp_out_ind = list(out_ind)
        for ax in sorted(new_axis):
            n = len(temp_out_ind) + len(drop_axis)
            temp_out_ind.insert(ax, n)
            new_axes[n] = chunks[ax] if chunks is not None else 1
        out_ind = tuple(temp_out_ind)
        if max(new_axis) > max(out_ind):
            raise ValueError("New_axis values do not fill in all dimensions")
    if chunks is not None:
        if len(chunks) != len(out_ind):
            raise ValueError(f"Provided chunks have {len(chunks)} dims; expected {len(out_ind)} dims")
        adjust_chunks = dict(zip(out_ind, chunks))
    else:
        adjust_chunks = None
    pairs = []
    for a, ind in argpairs:
        pairs += [a, ind]
    return blockwise(func, out_ind, *pairs, dtype=dtype, adjust_chunks=adjust_chunks,
                     new_axes=new_axes, align_arrays=False, **kwargs)


def map_direct(func, *args: "Array", shape, dtype, chunks, extra_projected_mem, spec=None,
               **kwargs) -> "Array":
    """Apply ``func`` over the blocks of a new array, reading side inputs
    directly.  ``func(block_id) -> region`` of the first side input (the only
    form the MI355X lowering needs: merge_chunks and index)."""
    from ..array_api.creation_functions import empty_virtual_array

    if spec is None and len(args) > 0 and hasattr(args[0], "spec"):
        spec = args[0].spec
    out = empty_virtual_array(shape, dtype=dtype, chunks=chunks, spec=spec)
    kwargs.pop("target_chunks", None)
    kwargs.pop("selection", None)
    field = kwargs.pop("field", None)  # read one field of a structured source (concat regions only)
    ndim = len(shape)
    src = args[0]
    region_fn = func
    # space dims of the region: source dims not removed by integer indexing
    sel = getattr(func, "selection", None)
    if sel is not None:
        axes, k = [], 0
        for s in sel:
            if _is_int(s):
                axes.append(None)
            else:
                axes.append(k)
                k += 1
        axes = tuple(axes)
    else:
        axes = tuple(range(src.ndim))

    def build(block_arg):
        if isinstance(region_fn, ConcatRegions):
            leaf = ir.Concat(src.name, np.dtype(dtype), tuple(range(ndim)), region_fn, block_arg,
                             field=field, sources=tuple(a.zarray_maybe_lazy for a in args),
                             axis=region_fn.axis)
        else:
            leaf = ir.Region(src.name, src.dtype, axes, region_fn, block_arg,
                             target=src.zarray_maybe_lazy)
        return ir.ExprProgram(ndim=ndim, nargs=block_arg + 1, outputs=leaf,
                              out_axes=tuple(range(ndim)), name="map_direct")

    return map_blocks(_BlockIdProgram(build, 1), out, dtype=dtype, chunks=chunks,
                      extra_source_arrays=args, extra_projected_mem=extra_projected_mem,
                      fusable=False, **kwargs)


class ConcatRegions:
    """Regions read by output block ``block_id`` of ``concat(arrays, axis)``
    (_read_concat_chunk / _array_slices, array_api/manipulation_functions.py
    :107-132): a list of (array index, region of that array, offset along
    ``axis`` inside the output block).  The block spans
    [block_id[axis] * chunk, + its extent) of the concatenated axis."""

    def __init__(self, out_chunks, axis, offsets):
        self.out_chunks = out_chunks
        self.axis = axis
        self.offsets = offsets

    def __call__(self, block_id):
        from bisect import bisect

        starts = [tuple(np.cumsum((0,) + c[:-1])) for c in self.out_chunks]
        base = [slice(int(starts[d][b]), int(starts[d][b]) + self.out_chunks[d][b])
                for d, b in enumerate(block_id)]
        ax = self.axis
        lo, hi = base[ax].start, base[ax].stop
        parts = []
        pos = lo
        while pos < hi:
            i = bisect(self.offsets, pos) - 1
            stop = min(hi, self.offsets[i + 1])
            if stop > pos:
                region = list(base)
                region[ax] = slice(pos - self.offsets[i], stop - self.offsets[i], 1)
                parts.append((i, tuple(region), pos - lo))
            pos = stop
        return parts


class GatherRegions(ConcatRegions):
    """Regions read by output block ``j`` of ``unique_gather``: every piece
    names the one source array (index 0).  Block ``b`` of the 1-d source, whose
    chunks are ``in_chunks``, holds ``counts[b]`` wanted elements at its front;
    the output is their concatenation, ``k = sum(counts)`` elements in chunks
    of ``out_chunks``.  A piece is (0, region of the source, offset inside the
    output block); blocks with a zero count contribute none."""

    def __init__(self, out_chunks, in_chunks, counts):
        ends = np.cumsum(np.asarray(counts, dtype=np.int64))
        super().__init__(out_chunks, 0, [0] + [int(v) for v in ends])
        self.in_starts = [0] + [int(v) for v in np.cumsum(np.asarray(in_chunks, dtype=np.int64))[:-1]]

    def __call__(self, block_id):
        from bisect import bisect

        j = block_id[0]
        lo = sum(self.out_chunks[0][:j])
        hi = lo + self.out_chunks[0][j]
        parts = []
        pos = lo
        while pos < hi:
            # the last block whose first output position is <= pos: zero-count
            # blocks share their start with the next one and are skipped
            b = bisect(self.offsets, pos) - 1
            stop = min(hi, self.offsets[b + 1])
            at = self.in_starts[b] + pos - self.offsets[b]
            parts.append((0, (slice(at, at + stop - pos, 1),), pos - lo))
            pos = stop
        return parts


# ------------------------------------------------------------------ rechunk / merge


def rechunk(x, chunks, target_store=None):
    normalized_chunks = normalize_chunks(chunks, x.shape, dtype=x.dtype)
    if x.chunks == normalized_chunks:
        return x
    target_chunks = to_chunksize(normalized_chunks)
    name = gensym()
    spec = x.spec
    if target_store is None:
        target_store = new_temp_path(name=name, spec=spec)
    name_int = f"{name}-int"
    temp_store = new_temp_path(name=name_int, spec=spec)
    ops = primitive_rechunk(x.zarray_maybe_lazy, target_chunks=target_chunks,
                            allowed_mem=spec.allowed_mem, reserved_mem=spec.reserved_mem,
                            target_store=target_store, temp_store=temp_store)
    Array = _Array()
    if len(ops) == 1:
        op = ops[0]
        op.target_array.name = name
        plan = Plan._new(name, "rechunk", op.target_array, op, False, x)
        return Array(name, op.target_array, spec, plan)
    op1 = ops[0]
    op1.target_array.name = name_int
    plan1 = Plan._new(name_int, "rechunk", op1.target_array, op1, False, x)
    x_int = Array(name_int, op1.target_array, spec, plan1)
    op2 = ops[1]
    op2.target_array.name = name
    plan2 = Plan._new(name, "rechunk", op2.target_array, op2, False, x_int)
    return Array(name, op2.target_array, spec, plan2)


class _merged_region:
    def __init__(self, target_chunks):
        self.target_chunks = target_chunks

    def __call__(self, block_id):
        return get_item(self.target_chunks, block_id)


def merge_chunks(x, chunks):
    target_chunksize = chunks
    if len(target_chunksize) != x.ndim:
        raise ValueError(
            f"Chunks {target_chunksize} must have same number of dimensions as array ({x.ndim})")
    if not all(c1 % c0 == 0 for c0, c1 in zip(x.chunksize, target_chunksize)):
        raise ValueError(f"Chunks {target_chunksize} must be a multiple of array's chunks {x.chunksize}")
    target_chunks = normalize_chunks(chunks, x.shape, dtype=x.dtype)
    return map_direct(_merged_region(target_chunks), x, shape=x.shape, dtype=x.dtype,
                      chunks=target_chunks, extra_projected_mem=0, target_chunks=target_chunks)


# ------------------------------------------------------------------ reductions


def _reduction_program(func, ndim, in_dtype, axis, extra_func_kwargs):
    r = as_chunk_reduction(func)
    if r is None:
        return ir.OpaqueProgram(func=func, nargs=1)
    return r.program(ndim, in_dtype, axis, keepdims=True, **(extra_func_kwargs or {}))


def _map_program(func, ndim, in_dtype, out_dtype):
    if isinstance(func, ChunkMap):
        return func.program(ndim, in_dtype, out_dtype)
    name = ir.NUMPY_ELEMENTWISE.get(func)
    if name is not None:
        return ir.elementwise_program(name, [in_dtype], [ndim], out_dtype)
    return ir.OpaqueProgram(func=func, nargs=1)


def reduction(x: "Array", func, combine_func=None, aggegrate_func=None, axis=None,
              intermediate_dtype=None, dtype=None, keepdims=False, use_new_impl=False,
              split_every=None, extra_func_kwargs=None) -> "Array":
    """Apply a function to reduce an array along one or more axes
    (core/ops.py:790-903: per-chunk reduce, then merge+combine rounds sized by
    allowed_mem, then aggregate / squeeze / astype)."""
    if use_new_impl:
        return reduction_new(x, func, combine_func, aggegrate_func, axis, intermediate_dtype,
                             dtype, keepdims, split_every, extra_func_kwargs)
    if combine_func is None:
        combine_func = func
    if axis is None:
        axis = tuple(range(x.ndim))
    if isinstance(axis, Integral):
        axis = (axis,)
    axis = validate_axis(axis, x.ndim)
    if intermediate_dtype is None:
        intermediate_dtype = dtype
    inds = tuple(range(x.ndim))
    result = x
    allowed_mem = x.spec.allowed_mem
    max_mem = allowed_mem - x.spec.reserved_mem

    adjust_chunks = {i: (1,) * len(c) if i in axis else c for i, c in enumerate(result.chunks)}
    prog = _reduction_program(func, x.ndim, x.dtype, axis, extra_func_kwargs)
    result = blockwise(prog, inds, result, inds, dtype=intermediate_dtype,
                       adjust_chunks=adjust_chunks)

    while any(n > 1 for i, n in enumerate(result.numblocks) if i in axis):
        target_chunks = list(result.chunksize)
        chunk_mem = chunk_memory(intermediate_dtype, result.chunksize)
        for i, s in enumerate(result.shape):
            if i in axis:
                assert result.chunksize[i] == 1
                if len(axis) > 1:
                    target_chunks[i] = min(s, x.chunksize[i])
                else:
                    target_chunk_size = (max_mem - chunk_mem) // (chunk_mem * 4)
                    if target_chunk_size <= 1:
                        raise ValueError(
                            f"Not enough memory for reduction. Increase allowed_mem ({allowed_mem}) "
                            "or decrease chunk size")
                    target_chunks[i] = min(s, target_chunk_size)
        if all(target_chunks[i] == result.chunksize[i] for i in axis):
            # multi-axis with unit source chunks along a reduced axis: the
            # per-axis target above would merge nothing (and loop forever);
            # merge along the first unfinished axis by the memory bound
            i = next(i for i in axis if result.numblocks[i] > 1)
            target_chunk_size = (max_mem - chunk_mem) // (chunk_mem * 4)
            if target_chunk_size <= 1:
                raise ValueError(
                    f"Not enough memory for reduction. Increase allowed_mem ({allowed_mem}) "
                    "or decrease chunk size")
            target_chunks[i] = min(result.shape[i], target_chunk_size)
        result = merge_chunks(result, tuple(target_chunks))
        if any(s > 1 for i, s in enumerate(result.chunksize) if i in axis):
            adjust_chunks = {i: (1,) * len(c) if i in axis else c for i, c in enumerate(result.chunks)}
            prog = _reduction_program(combine_func, x.ndim, result.dtype, axis, extra_func_kwargs)
            result = blockwise(prog, inds, result, inds, dtype=intermediate_dtype,
                               adjust_chunks=adjust_chunks)

    if aggegrate_func is not None:
        result = map_blocks(_map_program(aggegrate_func, result.ndim, result.dtype, dtype),
                            result, dtype=dtype)
    if not keepdims:
        axis_to_squeeze = tuple(i for i in axis if result.shape[i] == 1)
        if len(axis_to_squeeze) > 0:
            result = squeeze(result, axis_to_squeeze)
    from ..array_api import astype

    return astype(result, dtype, copy=False)


def reduction_new(x: "Array", func, combine_func=None, aggegrate_func=None, axis=None,
                  intermediate_dtype=None, dtype=None, keepdims=False, split_every=None,
                  extra_func_kwargs=None) -> "Array":
    """Tree reduction with ``split_every`` (core/ops.py:906-963)."""
    if combine_func is None:
        combine_func = func
    if axis is None:
        axis = tuple(range(x.ndim))
    if isinstance(axis, Integral):
        axis = (axis,)
    axis = validate_axis(axis, x.ndim)
    if intermediate_dtype is None:
        intermediate_dtype = dtype
    split_every = _normalize_split_every(split_every, axis)
    result = partial_reduce(
        x, partial(combine_func, **(extra_func_kwargs or {})),
        initial_func=partial(func, axis=axis, keepdims=True, **(extra_func_kwargs or {})),
        split_every=split_every, dtype=intermediate_dtype)
    result = tree_reduce(result, partial(combine_func, **(extra_func_kwargs or {})), axis=axis,
                         dtype=intermediate_dtype, split_every=split_every)
    if aggegrate_func is not None:
        result = map_blocks(_map_program(aggegrate_func, result.ndim, result.dtype, dtype),
                            result, dtype=dtype)
    if not keepdims:
        axis_to_squeeze = tuple(i for i in axis if result.shape[i] == 1)
        if len(axis_to_squeeze) > 0:
            result = squeeze(result, axis_to_squeeze)
    from ..array_api import astype

    return astype(result, dtype, copy=False)


# ------------------------------------------------------------------ scans


class _scan_block_function:
    """Output block ``b`` of a scan with carry reads block ``b`` of the values
    and the one carry chunk that holds the carry planes of ``b``'s row of
    blocks along ``axis`` (coordinate 0 there)."""

    def __init__(self, x_name, carry_name, axis):
        self.x_name, self.carry_name, self.axis = x_name, carry_name, axis

    def __call__(self, out_key):
        coords = tuple(out_key[1:])
        carry = coords[:self.axis] + (0,) + coords[self.axis + 1:]
        return [(self.x_name,) + coords, (self.carry_name,) + carry]


def scan(x: "Array", axis: int) -> "Array":
    """Prefix sums of ``x`` along ``axis``, same shape, chunks and dtype.
    ``x.dtype`` is one of the scan value types (float32, float64, int64,
    uint64); floats accumulate in float64 (``ir.scan_acc_dtype``).

    One block along ``axis``: one scan op.  ``nb`` blocks: per-chunk totals
    (the first step of ``reduction``), merged so that the ``nb`` totals along
    ``axis`` form one chunk, their exclusive prefix -- the carry of every
    block -- and a scan of each chunk of ``x`` that starts from its carry
    plane.  Every task reads whole chunks only and none reads a whole axis of
    ``x``; the merged totals must fit ``allowed_mem``."""
    from ..chunkfuncs import NumpyReduction

    dtype = np.dtype(x.dtype)
    acc = ir.scan_acc_dtype(dtype)
    inds = tuple(range(x.ndim))
    nb = x.numblocks[axis]
    if nb == 1:
        return blockwise(ir.ScanProgram(axis=axis, dtype=dtype), inds, x, inds, dtype=dtype,
                         fusable=False)
    spec = x.spec
    totals_chunksize = tuple(1 if i == axis else c for i, c in enumerate(x.chunksize))
    merged_chunksize = tuple(nb if i == axis else c for i, c in enumerate(x.chunksize))
    merged_mem = chunk_memory(acc, merged_chunksize)
    x_mem = chunk_memory(dtype, x.chunksize)
    # the merge reads totals chunks into one merged chunk, the carry op reads
    # and writes a merged chunk, the last op reads one next to its two chunks
    # of x (a compressed and an uncompressed copy of each, as blockwise counts)
    need = spec.reserved_mem + builtins.max(
        2 * chunk_memory(acc, totals_chunksize) + 2 * merged_mem, 4 * merged_mem, 2 * merged_mem + 4 * x_mem)
    if need > spec.allowed_mem:
        raise ValueError(
            f"Not enough memory for cumulative_sum. Increase allowed_mem ({spec.allowed_mem}) "
            "or decrease chunk size")
    sums = blockwise(NumpyReduction("sum", "sum").program(x.ndim, dtype, (axis,), keepdims=True, dtype=acc),
                     inds, x, inds, dtype=acc, adjust_chunks={axis: (1,) * nb})
    merged = merge_chunks(sums, merged_chunksize)
    carry = blockwise(ir.ScanProgram(axis=axis, exclusive=True, dtype=acc), inds, merged, inds,
                      dtype=acc, fusable=False)
    # the carry chunk is an array argument, so the projected memory of the op
    # already holds its two copies: no extra_projected_mem on top
    return general_blockwise(ir.ScanProgram(axis=axis, carry=True, dtype=dtype, nargs=2),
                             _scan_block_function(x.name, carry.name, axis), x, carry,
                             shape=x.shape, dtype=dtype, chunks=x.chunks, extra_projected_mem=0,
                             fusable=False)


# ------------------------------------------------------------------ sorts


def sort_network(nb: int):
    """Rounds of (lower, upper) block pairs that sort ``nb`` sorted blocks by
    merge-splits: the normalised bitonic network over ``P = next_pow2(nb)``
    positions.  For k = 2, 4, .., P one flip round (block b with b ^ (k - 1)),
    then rounds j = k/4, .., 1 (b with b ^ j).  In a pair the lower block keeps
    the first ``len(lower)`` elements of the merge and the upper one the rest,
    so a ragged last block keeps its length.  Positions at or above ``nb``
    stand for empty blocks after every real one: their pairs are left out (the
    partner is copied), and so is a round without a real pair."""
    if nb < 1:
        raise ValueError("sort_network needs at least one block")
    P = 1
    while P < nb:
        P *= 2
    rounds = []

    def add(partner):
        pairs = [(b, partner(b)) for b in range(nb) if b < partner(b) < nb]
        if pairs:
            rounds.append(pairs)

    k = 2
    while k <= P:
        add(lambda b: b ^ (k - 1))
        j = k // 4
        while j >= 1:
            add(lambda b: b ^ j)
            j //= 2
        k *= 2
    return rounds


class _merge_block_function:
    """Output block ``b`` of one round of the block network reads its own
    chunk of the previous round and its partner's, the lower block of the pair
    first; a block without a partner reads only its own."""

    def __init__(self, name, axis, pairs):
        self.name, self.axis = name, axis
        self.partner = {}
        for lo, hi in pairs:
            self.partner[lo], self.partner[hi] = hi, lo

    def __call__(self, out_key):
        coords = tuple(out_key[1:])
        b = coords[self.axis]
        p = self.partner.get(b)
        if p is None:
            return [(self.name,) + coords]
        other = coords[:self.axis] + (p,) + coords[self.axis + 1:]
        lo, hi = (coords, other) if b < p else (other, coords)
        return [(self.name,) + lo, (self.name,) + hi]


def sort(x: "Array", axis: int, descending: bool = False, pairs: bool = False,
         return_pairs: bool = False) -> "Array":
    """``x`` sorted along ``axis`` (``pairs=False``, same dtype) or the int64
    indices that sort it (``pairs=True``), same shape and chunks.  ``x.dtype``
    is one of the sort key types (float32, float64, 32- and 64-bit integers).
    Stable: ties go to the smaller index along the axis in both directions.

    The kernels sort rows, so an axis with a longer dim after it is moved
    last by ``permute_dims`` and moved back afterwards (two extra passes; the
    first one materialises, a sort is never fused).  One block along the axis:
    one ``"chunk"`` op.  ``nb`` blocks: the chunk op, then one ``"merge"`` op
    of ``nb`` tasks per round of ``sort_network(nb)``.  No task reads more
    than two chunks; every op passes the ordinary projected-memory check.

    ``return_pairs`` (with ``pairs``, and an axis that needs no permute): the
    sorted ``ir.sort_pairs_dtype`` array ``{v, i}`` itself, keys next to their
    indices, instead of the indices alone."""
    from ..array_api.manipulation_functions import permute_dims
    from ..chunkfuncs import _arg_aggregate

    nd = x.ndim
    if return_pairs and not pairs:
        raise ValueError("sort: return_pairs needs pairs")
    if builtins.any(s > 1 for s in x.shape[axis + 1:]):
        if return_pairs:
            raise ValueError("sort: return_pairs along an axis that is not the last one with more than one element")
        order = [d for d in range(nd) if d != axis] + [axis]
        y = sort(permute_dims(x, tuple(order)), nd - 1, descending, pairs)
        return permute_dims(y, tuple(int(i) for i in np.argsort(order)))
    dtype = np.dtype(x.dtype)
    work_dtype = ir.sort_pairs_dtype(dtype) if pairs else dtype
    inds = tuple(range(nd))
    # the merge passes inside a chunk ping-pong with a scratch copy of it
    chunk_mem = chunk_memory(work_dtype, x.chunksize)
    cur = blockwise(ir.SortProgram(axis=axis, descending=descending, pairs=pairs, dtype=dtype),
                    inds, x, inds, dtype=work_dtype, extra_projected_mem=chunk_mem, fusable=False)
    for rnd in sort_network(x.numblocks[axis]):
        # the partner's chunk is a second chunk of the one array argument
        cur = general_blockwise(
            ir.SortProgram(axis=axis, descending=descending, pairs=pairs, dtype=dtype, kind="merge", nargs=2),
            _merge_block_function(cur.name, axis, rnd), cur, shape=cur.shape, dtype=work_dtype,
            chunks=cur.chunks, extra_projected_mem=2 * chunk_mem, fusable=False)
    if pairs and not return_pairs:
        cur = blockwise(_arg_aggregate.program(nd, work_dtype), inds, cur, inds, dtype=np.int64)
    return cur


# ------------------------------------------------------------------ searches


class _search_block_function:
    """Output block ``j`` of the search against block ``b`` of the sorted
    array reads chunk ``j`` of the values, chunk ``b`` of the sorted array and,
    after the first block, chunk ``j`` of the counts so far."""

    def __init__(self, values_name, sorted_name, b, counts_name=None):
        self.values_name, self.sorted_name, self.b, self.counts_name = values_name, sorted_name, b, counts_name

    def __call__(self, out_key):
        coords = tuple(out_key[1:])
        keys = [(self.values_name,) + coords, (self.sorted_name, self.b)]
        if self.counts_name is not None:
            keys.append((self.counts_name,) + coords)
        return keys


def searchsorted(x1: "Array", x2: "Array", right: bool = False) -> "Array":
    """For every element of ``x2`` the int64 number of elements of the sorted
    1-d ``x1`` that sort before it (before or tied with it: ``right``), with
    the shape and chunks of ``x2``.  Both have the same dtype, one of the sort
    key types, and neither is empty.

    The count over ``x1`` is the sum of the counts over its blocks, so with
    ``nb`` blocks of ``x1`` the plan is ``nb`` chained ops: op ``b`` adds the
    count against block ``b`` to the counts of op ``b - 1``.  A task reads one
    chunk of ``x2``, one chunk of ``x1`` and (after the first op) one chunk of
    counts, never more, and every op passes the ordinary projected-memory
    check.  The price is ``nb`` passes over ``x2``: one read of its values
    and one read and one write of the counts per block of ``x1``."""
    dtype = np.dtype(x1.dtype)
    counts = None
    for b in range(x1.numblocks[0]):
        args = (x2, x1) if counts is None else (x2, x1, counts)
        counts = general_blockwise(
            ir.SearchProgram(right=bool(right), dtype=dtype, nargs=len(args)),
            _search_block_function(x2.name, x1.name, b, None if counts is None else counts.name),
            *args, shape=x2.shape, dtype=np.int64, chunks=x2.chunks, extra_projected_mem=0, fusable=False)
    return counts


# ------------------------------------------------------------------ gathers (take_along_axis)


class _gather_block_function:
    """Output block ``c`` of the gather from block ``b`` of the axis reads
    chunk ``c`` of the indices, the chunk of ``x`` at ``c`` with the axis
    coordinate replaced by ``b`` and, after the first block, chunk ``c`` of the
    result so far."""

    def __init__(self, idx_name, x_name, axis, b, prev_name=None):
        self.idx_name, self.x_name, self.axis, self.b, self.prev_name = idx_name, x_name, axis, b, prev_name

    def __call__(self, out_key):
        coords = tuple(out_key[1:])
        keys = [(self.idx_name,) + coords,
                (self.x_name,) + coords[:self.axis] + (self.b,) + coords[self.axis + 1:]]
        if self.prev_name is not None:
            keys.append((self.prev_name,) + coords)
        return keys


def take_along_axis(x: "Array", idx: "Array", axis: int) -> "Array":
    """``np.take_along_axis(x, idx, axis)`` for an int64 ``idx`` of ``x``'s
    number of dimensions, extents and chunks off ``axis`` (``0 <= axis <
    ndim``), neither empty: the shape and chunks of ``idx``, the dtype of
    ``x`` (real, 1, 2, 4 or 8 bytes).  An index ``i`` in ``[-n, 0)`` means
    ``i + n``; one outside ``[-n, n)`` gives a zero element.

    An output chunk may need any block of ``x`` along the axis and no task may
    hold them all, so with ``nb`` blocks the plan is ``nb`` chained ops: op
    ``b`` writes the elements whose index falls in block ``b`` and keeps the
    result of op ``b - 1`` (zero in op 0) elsewhere.  A task reads one chunk
    of ``idx``, one chunk of ``x`` and (after the first op) one chunk of the
    result so far, never more, and every op passes the ordinary
    projected-memory check.  The price is ``nb`` passes over ``idx``: one read
    of the indices and one read and one write of the result per block."""
    dtype = np.dtype(x.dtype)
    out = None
    for b in range(x.numblocks[axis]):
        args = (idx, x) if out is None else (idx, x, out)
        out = general_blockwise(
            ir.GatherProgram(axis=int(axis), dtype=dtype, nargs=len(args)),
            _gather_block_function(idx.name, x.name, axis, b, None if out is None else out.name),
            *args, shape=idx.shape, dtype=dtype, chunks=idx.chunks, extra_projected_mem=0, fusable=False)
    return out


# ------------------------------------------------------------------ run heads (unique_*)


class _unique_block_function:
    """Output block ``b`` reads chunk ``b`` of the sorted array and, after
    block 0, chunk ``b - 1`` (for the predecessor of its first element)."""

    def __init__(self, name):
        self.name = name

    def __call__(self, out_key):
        b = out_key[1]
        return [(self.name, b)] if b == 0 else [(self.name, b), (self.name, b - 1)]


def _unique_op(s, program, shape, dtype, chunks):
    from ..lowering import unique_scratch_bytes
    from .._native import UNIQUE_TILE

    if s.ndim != 1 or s.size == 0:
        raise ValueError("unique: a sorted 1-d array that is not empty")
    # the chunk before is a second chunk of the one array argument; the tile
    # counts are the launch's scratch
    extra = s.chunkmem * 2 + unique_scratch_bytes(s.chunksize[0], UNIQUE_TILE)
    return general_blockwise(program, _unique_block_function(s.name), s, shape=shape, dtype=dtype,
                             chunks=chunks, extra_projected_mem=extra, fusable=False)


def _unique_key_dtype(s, pairs):
    dtype = np.dtype(s.dtype)
    if pairs:
        if dtype.names != ("v", "i"):
            raise TypeError(f"unique: a pairs array has the fields v and i, not {dtype}")
        dtype = dtype["v"]
    return dtype


def unique_count(s: "Array", pairs: bool = False) -> "Array":
    """The int64 number of run heads of every chunk of the sorted 1-d array
    ``s`` (plain keys, or with ``pairs`` the ``{v, i}`` array of
    ``sort(.., return_pairs=True)``): shape ``(nb,)`` in chunks of 1, one never
    fused ``ir.UniqueProgram`` op whose task ``b`` reads chunks ``b`` and
    ``b - 1`` of ``s``."""
    dtype = _unique_key_dtype(s, pairs)
    nb = s.numblocks[0]
    return _unique_op(s, ir.UniqueProgram(kind="count", pairs=bool(pairs), dtype=dtype, nargs=2),
                      (nb,), np.int64, ((1,) * nb,))


def unique_pack(s: "Array", pairs: bool = False, payload=None) -> "Array":
    """The run heads of every chunk of the sorted 1-d array ``s`` packed at
    the front of the chunk of the same number of an array of ``s``'s shape and
    chunks, zeros behind them; the same two reads as ``unique_count``.
    ``payload=None``: plain keys.  ``"position"``: ``{v, i}`` records, ``i`` the
    position of the head in ``s``.  ``"index"`` (``pairs`` only): ``{v, i}``
    records that keep the ``i`` of ``s``."""
    dtype = _unique_key_dtype(s, pairs)
    if payload not in (None, "position", "index") or (payload == "index" and not pairs):
        raise ValueError(f"unique_pack: payload {payload!r}" + ("" if pairs else " of plain keys"))
    out_dtype = dtype if payload is None else ir.sort_pairs_dtype(dtype)
    return _unique_op(s, ir.UniqueProgram(kind="pack", pairs=bool(pairs), payload=payload, dtype=dtype, nargs=2),
                      s.shape, out_dtype, s.chunks)


def unique_gather(packed: "Array", counts_host, field=None) -> "Array":
    """The first ``counts_host[b]`` elements of every chunk ``b`` of the 1-d
    array ``packed``, concatenated: shape ``(k,)`` with ``k = sum(counts_host)
    > 0`` in chunks of ``min(c, k)``, ``c`` the chunk length of ``packed``.
    ``field`` reads one field of a structured ``packed``.

    One op whatever the number of blocks: output block ``j`` copies the pieces
    ``packed[b * c + lo : b * c + hi]`` that fall into its range, which the
    host knows from the prefix sums of ``counts_host`` (``GatherRegions``,
    lowered like ``concat``).  The pieces of a task are one output chunk's
    worth of elements in all."""
    counts = [int(v) for v in np.asarray(counts_host).reshape(-1)]
    if packed.ndim != 1 or len(counts) != packed.numblocks[0]:
        raise ValueError(f"unique_gather: {len(counts)} counts for {packed.numblocks} blocks")
    if builtins.any(n < 0 or n > e for n, e in zip(counts, packed.chunks[0])):
        raise ValueError("unique_gather: a count outside its chunk")
    k = builtins.sum(counts)
    if k == 0:
        raise ValueError("unique_gather: nothing to gather")
    dtype = np.dtype(packed.dtype) if field is None else np.dtype(packed.dtype)[field]
    c = packed.chunksize[0]
    chunks = normalize_chunks((builtins.min(c, k),), shape=(k,), dtype=dtype)
    return map_direct(GatherRegions(chunks, packed.chunks[0], counts), packed, shape=(k,), dtype=dtype, chunks=chunks,
                      extra_projected_mem=chunk_memory(dtype, to_chunksize(chunks)), field=field)


# ------------------------------------------------------------------ selection (nonzero, x[mask])


class _select_block_function:
    """Output block ``b`` reads chunk ``b`` of every argument."""

    def __init__(self, names):
        self.names = tuple(names)

    def __call__(self, out_key):
        return [(name, out_key[1]) for name in self.names]


def _select_op(f, values, program, shape, dtype, chunks):
    from ..lowering import select_predicate, select_scratch_bytes
    from .._native import SELECT_TILE_BYTES

    if f.ndim != 1 or f.size == 0:
        raise ValueError("select: a 1-d array that is not empty")
    try:
        esize, _ = select_predicate(f.dtype)
    except Exception as e:
        raise TypeError(str(e)) from None
    args = (f,) if values is None else (f, values)
    # the input and output chunks are counted by general_blockwise; the tile counts are the launch's scratch
    extra = select_scratch_bytes(f.chunksize[0], esize, SELECT_TILE_BYTES)
    return general_blockwise(program, _select_block_function(a.name for a in args), *args, shape=shape,
                             dtype=dtype, chunks=chunks, extra_projected_mem=extra, fusable=False)


def select_count(f: "Array") -> "Array":
    """The int64 number of elements of every chunk of the 1-d array ``f`` that
    are not zero (bool, integers, float32, float64, bfloat16; -0.0 is zero, a
    NaN is not): shape ``(nb,)`` in chunks of 1, one never fused
    ``ir.SelectProgram`` op whose task ``b`` reads chunk ``b`` only."""
    nb = f.numblocks[0]
    return _select_op(f, None, ir.SelectProgram(kind="count", dtype=np.dtype(f.dtype), nargs=1),
                      (nb,), np.int64, ((1,) * nb,))


def select_pack(f: "Array", values=None) -> "Array":
    """An array of ``f``'s shape and chunks that holds, packed at the front of
    every chunk with zeros behind them, the global flat positions of the
    chunk's elements of ``f`` that are not zero (int64, ``values=None``), or
    the elements of ``values`` at those places (``values.dtype``; ``values`` is
    1-d with ``f``'s shape and chunks, and task ``b`` reads chunk ``b`` of
    both).  One never fused ``ir.SelectProgram`` op."""
    if values is None:
        return _select_op(f, None, ir.SelectProgram(kind="pack", dtype=np.dtype(f.dtype), nargs=1),
                          f.shape, np.int64, f.chunks)
    vdtype = np.dtype(values.dtype)
    if vdtype.names or vdtype.kind == "c" or vdtype.itemsize not in (1, 2, 4, 8):
        raise TypeError(f"select_pack: values of {vdtype}")
    if values.shape != f.shape or values.chunks != f.chunks:
        raise ValueError(f"select_pack: values of shape {values.shape} in chunks {values.chunks} for a mask of "
                         f"shape {f.shape} in chunks {f.chunks}")
    return _select_op(f, values, ir.SelectProgram(kind="pack", payload="values", dtype=np.dtype(f.dtype),
                                                  value_dtype=vdtype, nargs=2),
                      f.shape, vdtype, f.chunks)


def select_nonzero(f: "Array", values=None):
    """EAGER: runs ``select_count(f)`` and one ``select_pack(f, values)`` on
    ``f.spec.executor`` now and reads the per-chunk counts to the host.
    Returns the lazy 1-d array of the ``k`` packed elements, gathered from HBM
    (``unique_gather`` over ``from_device``), or None if ``k == 0``."""
    counts = select_count(f)
    packed = select_pack(f, values)
    compute(counts, packed, _return_in_memory_array=False)
    per_chunk = counts._read_stored()
    if int(per_chunk.sum()) == 0:
        return None
    return unique_gather(from_device(packed.zarray, f.spec), per_chunk)


def _is_bool_key(ind):
    return isinstance(ind, (CoreArray, np.ndarray)) and np.dtype(ind.dtype) == np.bool_


def _index_mask(x, mask):
    """``x[mask]`` for a bool ``mask`` of ``x``'s shape: the selected elements
    in C order, 1-d.  EAGER, like ``select_nonzero``."""
    from ..array_api.creation_functions import empty
    from ..array_api.manipulation_functions import _ravel

    if np.dtype(x.dtype).kind == "c":
        raise TypeError("boolean-mask indexing of a complex array is not supported")
    if tuple(mask.shape) != tuple(x.shape):
        if mask.ndim < x.ndim:
            raise NotImplementedError(
                f"a boolean mask of fewer dimensions ({mask.ndim}) than the array ({x.ndim}) is not supported: "
                "the mask must have the array's shape")
        raise IndexError(f"boolean index of shape {tuple(mask.shape)} did not match the indexed array of "
                         f"shape {tuple(x.shape)}")
    if x.ndim == 0:
        raise NotImplementedError("boolean-mask indexing of a 0-d array is not supported")
    if isinstance(mask, np.ndarray):
        mask = from_array(mask, chunks=x.chunks, spec=x.spec)
    elif mask.chunks != x.chunks:
        mask = rechunk(mask, x.chunksize)
    out = None
    if x.size:
        out = select_nonzero(_ravel(mask), _ravel(x))
    if out is None:
        out = empty((0,), dtype=x.dtype, chunks=(1,), spec=x.spec)
    return out


def from_device(target: DeviceArray, spec=None) -> "Array":
    """An array over a ``DeviceArray`` that an earlier compute has written:
    a source without an op, so a plan that starts from it computes nothing
    again.  The buffer stays alive as long as the arrays built on it, and the
    executor counts it among the plan's HBM-resident arrays."""
    if not isinstance(target, DeviceArray) or not target.written:
        raise ValueError("from_device: a DeviceArray that has been computed")
    if target.name is None:
        target.name = gensym()
    plan = Plan._new(target.name, "from_device", target)
    return _Array()(target.name, target, spec or _default_spec(), plan)


# ------------------------------------------------------------------ histograms


class _hist_block_function:
    """Output block ``(b..., 0)`` of the partial histograms reads chunk
    ``b...`` of the values and the one chunk of the edges."""

    def __init__(self, x_name, edges_name):
        self.x_name, self.edges_name = x_name, edges_name

    def __call__(self, out_key):
        return [(self.x_name,) + tuple(out_key[1:-1]), (self.edges_name, 0)]


def histogram(x: "Array", edges: "Array", nbins: int, uniform: bool) -> "Array":
    """The int64 counts, shape ``(nbins,)`` in one chunk, of the elements of
    ``x`` (any shape, not empty) in the bins of the 1-d one-chunk array
    ``edges`` of ``nbins + 1`` non-decreasing values (``ir.HistogramProgram``);
    ``uniform`` says that the edges are evenly spaced.

    ``x`` is converted to the edges' dtype first (float32 only for float32 ``x``
    with float32 edges, else float64), so the kernel has two key types; for
    non-float ``x`` that is one extra pass.  Then one op counts every chunk of
    ``x`` into its own row of a partials array of shape ``x.numblocks +
    (nbins,)`` -- a task reads one chunk of ``x`` and the edges and writes
    ``nbins`` counts, which the ordinary projected-memory check covers -- and
    the existing sum reduction adds the rows up."""
    from ..array_api import astype
    from ..array_api.statistical_functions import sum as _sum

    dtype = np.dtype(edges.dtype)
    if edges.ndim != 1 or edges.numblocks != (1,) or edges.shape[0] != nbins + 1 or nbins < 1:
        raise ValueError(f"histogram: {nbins} bins need one chunk of {nbins + 1} edges")
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"histogram: edges of dtype {dtype}")
    x = astype(x, dtype, copy=False)
    shape = tuple(x.numblocks) + (nbins,)
    chunks = tuple((1,) * n for n in x.numblocks) + ((nbins,),)
    partials = general_blockwise(
        ir.HistogramProgram(nbins=int(nbins), uniform=bool(uniform), dtype=dtype, nargs=2),
        _hist_block_function(x.name, edges.name),
        x, edges, shape=shape, dtype=np.int64, chunks=chunks, extra_projected_mem=0, fusable=False)
    if x.ndim == 0:
        return partials
    return _sum(partials, axis=tuple(range(x.ndim)), dtype=np.int64)


def _normalize_split_every(split_every, axis):
    split_every = split_every or 4
    if isinstance(split_every, dict):
        split_every = {k: split_every.get(k, 2) for k in axis}
    elif isinstance(split_every, Integral):
        n = builtins.max(int(split_every ** (1 / (len(axis) or 1))), 2)
        split_every = dict.fromkeys(axis, n)
    else:
        raise ValueError("split_every must be a int or a dict")
    return split_every


def tree_reduce(x, func, axis, dtype, split_every=None):
    """Apply a reduction function repeatedly across multiple axes."""
    if axis is None:
        axis = tuple(range(x.ndim))
    if isinstance(axis, Integral):
        axis = (axis,)
    axis = validate_axis(axis, x.ndim)
    split_every = _normalize_split_every(split_every, axis)
    depth = 0
    for i, n in enumerate(x.numblocks):
        if i in split_every and split_every[i] != 1:
            depth = int(builtins.max(depth, math.ceil(math.log(n, split_every[i]))))
    for _ in range(depth):
        x = partial_reduce(x, func, split_every=split_every, dtype=dtype)
    return x


def partial_reduce(x, func, initial_func=None, split_every=None, dtype=None):
    """Reduce groups of ``split_every`` blocks per axis into one block."""
    chunks = [(1,) * math.ceil(len(c) / split_every[i]) if i in split_every else c
              for (i, c) in enumerate(x.chunks)]
    shape = tuple(map(sum, chunks))
    axis = tuple(ax for ax in split_every.keys())

    def block_function(out_key):
        out_coords = out_key[1:]
        in_keys = [list(range(bi * split_every.get(i, 1),
                              min((bi + 1) * split_every.get(i, 1), x.numblocks[i])))
                   for i, bi in enumerate(out_coords)]
        return (iter([(x.name,) + tuple(p) for p in product(*in_keys)]),)

    extra_projected_mem = x.chunkmem
    # the task reduces the concatenation of its blocks: initial_func's
    # reduction over the merged view (fields compose, e.g. mean's n/total)
    r = as_chunk_reduction(initial_func if initial_func is not None else func)
    if r is None:
        prog = ir.OpaqueProgram(func=func, nargs=1)
    else:
        kw = {"dtype": dtype} if dtype is not None and not _has_bound_dtype(r) else {}
        prog = r.program(x.ndim, x.dtype, axis, keepdims=True, **kw)
    return general_blockwise(prog, block_function, x, shape=shape, dtype=dtype, chunks=chunks,
                             extra_projected_mem=extra_projected_mem)


def _has_bound_dtype(r) -> bool:
    kw = getattr(r, "kw", None)
    return bool(kw) and "dtype" in kw


def squeeze(x, /, axis):
    if not isinstance(axis, tuple):
        axis = (axis,)
    if any(x.shape[i] != 1 for i in axis):
        raise ValueError("cannot squeeze axis with size other than one")
    axis = validate_axis(axis, x.ndim)
    chunks = tuple(c for i, c in enumerate(x.chunks) if i not in axis)
    prog = ir.ExprProgram(ndim=x.ndim, nargs=1,
                          outputs=ir.Arg(0, x.dtype, tuple(range(x.ndim))) if not x.dtype.names else
                          tuple((f, ir.Arg(0, x.dtype[f], tuple(range(x.ndim)), field=f))
                                for f in x.dtype.names),
                          out_axes=tuple(d for d in range(x.ndim) if d not in axis), name="squeeze")
    return map_blocks(prog, x, dtype=x.dtype, chunks=chunks, drop_axis=axis)


def arg_reduction(x, /, arg_func, axis=None, *, keepdims=False):
    """argmax / argmin along one axis or over the whole array
    (core/ops.py:1093-1153).

    The reference's first map (_arg_map_func) turns each block into {i, v}
    with the block-offset index, then ``reduction`` combines the pairs with
    _arg_combine.  Here every ELEMENT is a {v, i} pair -- its value key and
    its global index (the flat C-order index when axis is None, which the
    reference gets from reshape) -- built inside the reduce kernel's program
    and reduced in one fused pass with the pair op argmax / argmin
    (chunkfuncs.ArgReduction): the first NaN wins, else the larger (smaller)
    value, ties to the smaller index, as numpy.  Value keys: floats as f64
    (exact), bool / ints as int64, uint64 with the sign bit flipped
    (order-preserving)."""
    from ..array_api import creation_functions as cf
    from ..array_api import manipulation_functions as mf
    from ..array_api import elementwise_functions as ef
    from ..chunkfuncs import ArgReduction, _arg_aggregate

    if x.ndim == 0:
        x = mf.expand_dims(x, axis=0)
        axis, keepdims = 0, False
    if axis is not None:
        axis = validate_axis(axis, x.ndim)
        if isinstance(axis, tuple):
            if len(axis) != 1:
                raise ValueError("argmax/argmin take a single axis")
            axis = axis[0]
    if (x.size if axis is None else x.shape[axis]) == 0:
        raise ValueError(f"attempt to get {arg_func} of an empty sequence")

    def index_along(d):
        """The index along dim d, broadcastable against x."""
        idx = cf.arange(x.shape[d], dtype=np.int64, chunks=(x.chunks[d],), spec=x.spec)
        for e in range(x.ndim):
            if e != d:
                idx = mf.expand_dims(idx, axis=e)
        return idx

    if axis is None and x.ndim > 1:
        idx = None
        for d in range(x.ndim):
            stride = int(np.prod(x.shape[d + 1:], dtype=np.int64))
            term = ef.multiply(index_along(d), cf.asarray(np.int64(stride), spec=x.spec))
            idx = term if idx is None else ef.add(idx, term)
        red_axis = None
    else:
        red_axis = 0 if axis is None else axis
        idx = index_along(red_axis)

    dt = np.dtype(x.dtype)
    n = x.ndim
    v = ir.Arg(0, dt, tuple(range(n)))
    if ir.is_float(dt):
        vdt = np.dtype(np.float64)
        key = ir.cast(v, vdt)
    else:
        vdt = np.dtype(np.int64)
        key = ir.cast(v, vdt)
        if dt == np.uint64:
            key = ir.Binary("bitwise_xor", key, ir.Const(np.int64(np.iinfo(np.int64).min), vdt), vdt)
    intermediate = [("v", vdt), ("i", np.int64)]
    prog = ir.ExprProgram(ndim=n, nargs=2,
                          outputs=(("v", key), ("i", ir.Arg(1, np.dtype(np.int64), tuple(range(n))))),
                          out_axes=tuple(range(n)), name=f"{arg_func}_pairs")
    inds = tuple(range(n))[::-1]
    pairs = blockwise(prog, inds, x, inds, idx, inds, dtype=intermediate)
    r = ArgReduction(arg_func)
    return reduction(pairs, r, combine_func=r, aggegrate_func=_arg_aggregate, axis=red_axis,
                     intermediate_dtype=intermediate, dtype=np.int64, keepdims=keepdims)


def unify_chunks(*args: "Array", **kwargs):
    if not args:
        return {}, []
    arginds = [(args[i], args[i + 1]) for i in range(0, len(args), 2)]
    arrays, inds = zip(*arginds)
    if all(ind is None for ind in inds):
        return {}, list(arrays)
    if all(ind == inds[0] for ind in inds) and all(a.chunks == arrays[0].chunks for a in arrays):
        return dict(zip(inds[0], arrays[0].chunks)), list(arrays)
    # broadcast dimensions: per index, the common refinement of the chunkings
    groups = {}
    for a, ind in arginds:
        if ind is None:
            continue
        for c, i in zip(a.chunks, ind):
            groups.setdefault(i, set()).add(c)
    chunkss = {}
    for i, cs in groups.items():
        cs2 = cs - {(1,)} if len(cs) > 1 else cs
        chunkss[i] = common_blockdim(cs2)
    out = []
    for a, ind in arginds:
        if ind is None:
            out.append(a)
            continue
        chunks = tuple(chunkss[j] if a.shape[n] > 1 else (a.shape[n],) for n, j in enumerate(ind))
        if chunks != a.chunks and all(a.chunks):
            out.append(rechunk(a, to_chunksize(chunks)))
        else:
            out.append(a)
    return chunkss, out


def validate_axis(axis, ndim):
    if isinstance(axis, (tuple, list)):
        return tuple(validate_axis(ax, ndim) for ax in axis)
    if not isinstance(axis, Integral):
        raise TypeError(f"Axis value must be an integer, got {axis}")
    if axis < -ndim or axis >= ndim:
        raise np.exceptions.AxisError(axis, ndim) if hasattr(np, "exceptions") else ValueError(axis)
    if axis < 0:
        axis += ndim
    return axis
