from .array import CoreArray, compute, gensym, measure_reserved_mem, visualize
from .ops import (
    blockwise,
    elemwise,
    from_array,
    from_device,
    from_zarr,
    histogram,
    map_blocks,
    map_direct,
    merge_chunks,
    partial_reduce,
    rechunk,
    reduction,
    scan,
    searchsorted,
    select_count,
    select_pack,
    sort,
    sort_network,
    squeeze,
    store,
    take_along_axis,
    to_zarr,
    tree_reduce,
    unify_chunks,
    unique_count,
    unique_gather,
    unique_pack,
)
from .plan import Plan

__all__ = [
    "CoreArray", "Plan", "blockwise", "compute", "elemwise", "from_array", "from_device", "from_zarr",
    "gensym", "histogram", "map_blocks", "map_direct", "measure_reserved_mem", "merge_chunks",
    "partial_reduce", "rechunk", "reduction", "scan", "searchsorted", "select_count", "select_pack", "sort", "sort_network", "squeeze", "store", "take_along_axis", "to_zarr", "tree_reduce",
    "unify_chunks", "unique_count", "unique_gather", "unique_pack", "visualize",
]
