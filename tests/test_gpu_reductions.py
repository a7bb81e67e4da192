"""Reduction conformance on the GPU: every reduction of the fused kernels
(vm.h acc_init / acc_add / acc_combine, kernels.h, stream_impl.h) x every
dtype it accepts x every kernel form, against a plain high-precision
reference of the same operation on the same host array.

The kernel forms are the rows of vm_model.REDUCE_FORMS (the same table
test_reduce_plan.py checks on a lower-only dry run): each test asserts,
through the spy on lowering.FusedLaunch, that every reduction it computed
reached the form it names -- mode bits, tasks, kept and reduced extents, the
split workspace, the number of rounds -- so a geometry that quietly stops
reaching its kernel fails.

Inputs (vm_model.reduce_inputs): every kept element tells one designed
story (NaNs of either sign, infinities, zeros of either sign, dtype extremes,
wrapping sums and products, ...), its special values in different chunks,
splits and the first and last reduced row.  Equality (vm_model.
check_reduction): integer and bool results bit-exact, sums and products
wrapped; float max / min value-equal with NaN in the same places; float sums,
products and means within the bound of float64 accumulation in any order plus
the final rounding(s), NaN and +-inf equal in place and sign.  Nothing is
masked but the sign of a zero max / min and of a zero sum."""
import numpy as np
import pytest

import vm_model as M
from cubed_amd import lowering as L
from gpu_fixtures import build_cell, interp, jit, run_cell, spy  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ interpreter
@pytest.mark.parametrize("dtype", M.REDUCE_DTYPES)
@pytest.mark.parametrize("form", list(M.REDUCE_FORMS))
def test_interpreter_matrix(interp, spy, form, dtype):
    """Every reduction ``dtype`` takes, default and explicit result dtypes,
    on one kernel form of the ahead-of-time interpreter."""
    lazy, checks, leaves = build_cell(interp, form, dtype)
    run_cell(lazy, checks)
    M.assert_form_ran(spy, form, leaves, jit=False)


# ------------------------------------------------------------------ JIT
JIT_FORMS = ("scalar-axis0", "stream-split", "b-split", "lifted")
JIT_DTYPES = ("float32", "float64", "int64", "int8")  # one per register type, and a narrow one


JIT_PARTS = 4


def jit_cases(dtype, part):
    """Every reduction of ``dtype`` runs on every form of the slice; a test
    takes every fourth of them (at most three), since each specialised
    program is a hipRTC compile of a second or two (measured: 5.5 s for the
    three of lifted-float32, 5.0 s for the two of stream-split-float32 and
    their folds)."""
    return M.reduce_cases(dtype)[part::JIT_PARTS]


@pytest.mark.parametrize("part", range(JIT_PARTS))
@pytest.mark.parametrize("dtype", JIT_DTYPES)
@pytest.mark.parametrize("form", JIT_FORMS)
def test_jit_slice(jit, spy, form, dtype, part):
    """The hipRTC-specialised kernels: every reduction of float32, float64,
    int64 and int8 on the scalar, split streaming, split reduced-dims-last
    and lifted forms."""
    cases = jit_cases(dtype, part)
    assert 1 <= len(cases) <= 3
    lazy, checks, leaves = build_cell(jit, form, dtype, cases)
    run_cell(lazy, checks)
    M.assert_form_ran(spy, form, leaves, jit=True)


def test_jit_slice_is_the_full_cross_product():
    for dtype in JIT_DTYPES:
        dealt = [c for part in range(JIT_PARTS) for c in jit_cases(dtype, part)]
        assert sorted(dealt, key=str) == sorted(M.reduce_cases(dtype), key=str)


@pytest.mark.parametrize("w", [1, 2, 4])
def test_stream_groups_per_thread(jit, spy, monkeypatch, w):
    """max, nansum and mean of float32 on the ragged streaming form with W
    kept groups per thread forced: a wave owns 256 W kept elements, so the
    1028 are four full waves and a partial one at W = 1, two and a partial
    one at W = 2, one and a partial one at W = 4.  (The W = 2 programs take
    hipRTC some 20 s each to compile, as those of test_gpu_parity.py's test
    of the same name do: the case is slow, and it is a case the kernels have.)"""
    monkeypatch.setattr(L, "FORCE_STREAM_W", w)
    cases = [("max", None), ("nansum", None), ("mean", None)]
    lazy, checks, leaves = build_cell(jit, "stream-ragged", "float32", cases)
    run_cell(lazy, checks)
    M.assert_form_ran(spy, "stream-ragged", leaves, jit=True)
    bits = {1: 0, 2: L.MODE_STREAM_W2, 4: L.MODE_STREAM_W4}[w]
    first = [s for s in spy if M.launch_signature(s) == M.form_signature("stream-ragged", "float32")]
    assert len(first) == len(lazy)
    assert all(s.mode & (L.MODE_STREAM_W2 | L.MODE_STREAM_W4) == bits for s in spy if s.mode & L.MODE_STREAM)
