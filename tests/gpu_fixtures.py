"""Fixtures and helpers shared by the GPU conformance suites
(test_gpu_elementwise.py, test_gpu_reductions.py).  Not a conftest: the test
modules import the names they use."""
import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
import vm_model as M
from cubed_amd import lowering as L


class Seen(tuple):
    """(vtype, mode, has JIT handle) of one FusedLaunch, with the launch's
    geometry as attributes: ``nfields`` (0: a map), ``ntasks``, ``max_kept``,
    ``max_red``, ``ws`` (cubed_fused_workspace_bytes(...) of the launch) and
    ``split`` -- a workspace on a launch that writes no partials: the reduced
    extent is split across workgroups and folded."""

    def __new__(cls, launch):
        prog = launch.prog
        self = super().__new__(cls, (int(prog.vtype), int(prog.mode), launch.handle is not None))
        self.nfields = int(prog.nfields)
        self.ntasks, self.max_kept, self.max_red = int(launch.ntasks), int(launch.max_kept), int(launch.max_red)
        self.ws = int(launch.ws_bytes)
        self.split = self.ws > 0 and not prog.mode & L.MODE_PARTIALS
        return self

    vtype = property(lambda self: self[0])
    mode = property(lambda self: self[1])
    jit = property(lambda self: self[2])


def record_launches(monkeypatch):
    seen = []

    class Recording(L.FusedLaunch):
        def __init__(self, prog, *a, **k):
            super().__init__(prog, *a, **k)
            seen.append(Seen(self))

    monkeypatch.setattr(L, "FusedLaunch", Recording)
    return seen


@pytest.fixture
def spy(monkeypatch):
    """[(vtype, mode, has JIT handle)] of every FusedLaunch built (Seen)."""
    return record_launches(monkeypatch)


def make_spec(ex, allowed_mem="2GB", reserved_mem="100MB"):
    return cubed.Spec(allowed_mem=allowed_mem, reserved_mem=reserved_mem, executor=ex)


@pytest.fixture
def interp(monkeypatch, gpu_executor):
    """A fresh executor running the ahead-of-time interpreter kernels."""
    from cubed_amd.runtime.executors.gpu import GpuDagExecutor

    monkeypatch.setenv("CUBED_AMD_JIT", "0")
    return make_spec(GpuDagExecutor("cuda:0"))


@pytest.fixture
def jit(monkeypatch, gpu_executor):
    from cubed_amd.runtime.executors.gpu import GpuDagExecutor

    monkeypatch.setenv("CUBED_AMD_JIT", "1")
    return make_spec(GpuDagExecutor("cuda:0"))


def arr(x, chunks, spec):
    return cubed.from_array(x, chunks=chunks, spec=spec)


# ------------------------------------------------------------------ reduction cells
def reduction(fn):
    return getattr(cubed, fn) if fn.startswith("nan") else getattr(xp, fn)


def device_array(x, dtype, chunks, spec):
    if dtype == "bfloat16":  # x: float32 values bfloat16 holds exactly
        return xp.astype(arr(x, chunks, spec), xp.bfloat16)
    return arr(x, chunks, spec)


def leaf_dtype(dtype, consumers):
    """The dtype the reduction kernel reads.  A bfloat16 input is an astype
    of a float32 array: with one consumer the cast fuses into the reduction,
    which then reads float32 leaves and rounds them to bfloat16 in registers;
    with several the bfloat16 array is written out and read back."""
    return "float32" if dtype == "bfloat16" and consumers == 1 else dtype


def build_cell(spec, form, dtype, cases=None):
    """Lazy results, their checks and the dtype each one's kernel reads, of
    ``cases`` (default: every reduction ``dtype`` takes) on the inputs of
    ``form``: as many input variants as it takes for every story to be
    reduced."""
    f = M.REDUCE_FORMS[form]
    if f["mem"]:
        spec = make_spec(spec.executor, f["mem"], 0)
    in_dtype = M.reduce_dtype(dtype)
    lazy, checks, leaves = [], [], []
    cases = cases or M.reduce_cases(dtype)
    for v in range(M.reduce_variants(dtype, f["shape"], f["axis"])):
        dev = {}
        for fn, explicit in cases:
            kind = "prod" if fn == "prod" else "sum"
            if kind not in dev:
                x, stories = M.reduce_inputs(kind, dtype, f["shape"], f["axis"], variant=v)
                dev[kind] = x, stories, device_array(x, dtype, f["chunks"], spec)
            x, stories, X = dev[kind]
            kw = dict(axis=f["axis"], keepdims=f["keepdims"])
            if explicit is not None:
                kw["dtype"] = np.dtype(explicit)
            y = reduction(fn)(X, **kw)
            assert y.dtype == M.reduce_result_dtype(fn, in_dtype, explicit), (fn, dtype, explicit, y.dtype)
            lazy.append(y)
            leaves.append(leaf_dtype(dtype, sum((c[0] == "prod") == (fn == "prod") for c in cases)))
            what = f"{fn}({dtype}{', dtype=' + explicit if explicit else ''}) {form} variant {v}"
            checks.append(dict(fn=fn, x=x, axis=f["axis"], in_dtype=in_dtype, dtype=explicit,
                               keepdims=f["keepdims"], stories=stories, what=what))
    return lazy, checks, leaves


def run_cell(lazy, checks):
    got = cubed.compute(*lazy)
    failures = []
    for g, c in zip(got, checks):
        try:
            M.check_reduction(got=np.asarray(g), **c)
        except AssertionError as e:
            failures.append(str(e)[:400])
    assert not failures, "\n".join(failures)
