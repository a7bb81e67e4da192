"""The reduction conformance suite on CPU: the kernel forms its geometry
table names (vm_model.REDUCE_FORMS) checked on a lower-only dry run -- nothing
is launched --, the designed inputs checked against the conditions the
tolerances rest on, and the comparison helpers fed deliberately wrong results.

The values themselves are checked on the GPU (tests/test_gpu_reductions.py),
which reads the same table."""

import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
import vm_model as M
from cubed_amd import ir
from cubed_amd import lowering as L
from cubed_amd.core.plan import arrays_to_plan
from dryrun import DryExecutor
from gpu_fixtures import build_cell, make_spec, record_launches

FORMS = list(M.REDUCE_FORMS)


@pytest.fixture
def lowered(built, monkeypatch):
    """lower(*lazy) -> the recorded launches (gpu_fixtures.Seen) of their
    plan on the interpreter path, and the spec to build the arrays with."""
    monkeypatch.setenv("CUBED_AMD_JIT", "0")
    seen = record_launches(monkeypatch)
    ex = DryExecutor()

    def lower(*lazy):
        del seen[:]
        arrays_to_plan(*lazy).execute(executor=ex, array_names=[y.name for y in lazy])
        return list(seen)

    return lower, make_spec(ex)


def _zeros(form, dtype, spec):
    f = M.REDUCE_FORMS[form]
    if f["mem"]:
        spec = make_spec(spec.executor, f["mem"], 0)
    return cubed.from_array(np.zeros(f["shape"], dtype=M.reduce_dtype(dtype)), chunks=f["chunks"], spec=spec)


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("dtype", M.REDUCE_DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_form_table(lowered, form, dtype):
    """Every row at every input dtype (bfloat16 as a stored leaf): the mode
    bits, tasks and extents of the first launch, its fields, the rounds, and
    whether the reduced extent is split."""
    lower, spec = lowered
    f = M.REDUCE_FORMS[form]
    x = _zeros(form, dtype, spec)
    want = M.form_signature(form, dtype)
    fns = [("any", 1)] if dtype == "bool" else [("sum", 1), ("max", 1)]
    if dtype in ("float32", "float64", "bfloat16"):
        fns += [("mean", 2)]
    for fn, nfields in fns:
        y = getattr(xp, fn)(x, axis=f["axis"], keepdims=f["keepdims"])
        red = [s for s in lower(y) if s.nfields > 0]
        assert M.launch_signature(red[0]) == want, (fn, M.launch_signature(red[0]), want)
        assert [s.nfields for s in red] == [nfields] * f["rounds"], fn
        assert (red[0].ws > 0) == (f["split"] or bool(want[1] & L.MODE_PARTIALS)), fn
        assert not any(s.jit for s in red)
        assert y.shape == np.empty(f["shape"], dtype=bool).sum(axis=f["axis"], keepdims=f["keepdims"]).shape
        M.assert_form_ran(red, form, [dtype], jit=False)


def test_forms_differ_where_the_table_says():
    """The rows the streaming kernels take and their narrow twins, the split
    rows and the lifted ones are told apart by the signature alone."""
    sig = M.form_signature
    for form, f in M.REDUCE_FORMS.items():
        stream, narrow = f["modes"]
        assert (sig(form, "float64")[1], sig(form, "uint64")[1], sig(form, "bfloat16")[1]) == (stream, narrow, narrow)
        assert bool(stream & L.MODE_STREAM) == (stream != narrow)
        assert not narrow & L.MODE_STREAM
    modes = {form: f["modes"] for form, f in M.REDUCE_FORMS.items()}
    assert modes["scalar-axis0"] == (0, 0) and modes["vec4-unsplit"] == (12, 4) and modes["b-vec4"] == (5, 5)
    assert modes["b-scalar"] == (1, 1) and modes["lifted"] == (12 | L.MODE_PARTIALS, 4 | L.MODE_PARTIALS)
    assert {form for form, f in M.REDUCE_FORMS.items() if f["split"]} == \
        {"stream-split", "vec4-split", "b-split", "full-b-split", "merge-rounds"}


@pytest.mark.parametrize("form", FORMS)
def test_gpu_cells_lower_to_their_form(lowered, form):
    """The cells of the GPU suite -- the designed inputs, every reduction and
    variant of a dtype in one plan -- reach the form, a fused and a stored
    bfloat16 astype included."""
    lower, spec = lowered
    turn = FORMS.index(form)
    for dtype in (("float32", "uint8"), ("float64", "bfloat16"), ("int64", "int8"))[turn % 3]:
        lazy, checks, leaves = build_cell(spec, form, dtype)
        assert len(lazy) == len(checks) == len(leaves) == \
            len(M.reduce_cases(dtype)) * M.reduce_variants(dtype, *[M.REDUCE_FORMS[form][k] for k in ("shape", "axis")])
        M.assert_form_ran(lower(*lazy), form, leaves, jit=False)
        if dtype == "bfloat16":
            assert sorted(set(leaves)) == ["bfloat16", "float32"]


@pytest.mark.parametrize("fn", ["sum", "prod", "nansum"])
@pytest.mark.parametrize("dtype, out", [("float32", "float32"), ("bfloat16", None), ("float64", "float32")])
def test_narrow_float_results_keep_float64_partials(lowered, fn, dtype, out):
    """A float32 / bfloat16 sum, nansum or product of several rounds keeps its
    partials in float64 and is rounded once at the end (regression: partials
    in the result dtype put sum(float32, dtype=float32) over (7, 13) in
    (3, 5) chunks two spacings off)."""
    lower, spec = lowered
    x = _zeros("scalar-axis0", dtype, spec)
    f = getattr(cubed, fn) if fn == "nansum" else getattr(xp, fn)
    y = f(x, axis=0) if out is None else f(x, axis=0, dtype=np.dtype(out))
    assert y.dtype == M.reduce_dtype(out or dtype)
    red = [s for s in lower(y) if s.nfields > 0]
    assert len(red) == 2 and red[1].vtype == L.V_F64  # the combine round reads float64 partials
    for node, d in y.plan.dag.nodes(data=True):
        p = d.get("pipeline")
        prog = getattr(getattr(p, "config", None), "function", None)
        if isinstance(prog, ir.ExprProgram) and prog.reduce is not None:
            assert [np.dtype(fl.dtype) for fl in prog.reduce.fields] == [np.dtype(np.float64)], node


def test_integer_and_float64_partials_are_unchanged(lowered):
    lower, spec = lowered
    for dtype, out, want in (("int8", "int8", np.int8), ("uint8", None, np.uint64), ("float64", None, np.float64),
                             ("float32", None, np.float64)):
        y = xp.sum(_zeros("scalar-axis0", dtype, spec), axis=0, **({} if out is None else dict(dtype=np.dtype(out))))
        progs = [d["pipeline"].config.function for _, d in y.plan.dag.nodes(data=True)
                 if isinstance(getattr(getattr(d.get("pipeline"), "config", None), "function", None), ir.ExprProgram)]
        fields = [fl.dtype for p in progs if p.reduce is not None for fl in p.reduce.fields]
        assert len(fields) == 2 and all(np.dtype(t) == np.dtype(want) for t in fields), dtype


@pytest.mark.parametrize("fn", ["nansum", "nanmean"])
def test_nan_reductions_combine_with_plain_sums(lowered, fn):
    """Only the per-chunk round skips NaNs.  A partial that is NaN because
    +inf and -inf met in one chunk is a value of the result (numpy:
    np.nansum([np.inf, -np.inf]) is nan); a NaN-skipping combine round dropped
    it (regression: nansum / nanmean of the both_inf story on the scalar-all
    and full-b-split forms gave a finite result)."""
    lower, spec = lowered
    y = getattr(cubed, fn)(_zeros("scalar-all", "float64", spec))
    progs = [d["pipeline"].config.function for _, d in y.plan.dag.nodes(data=True)
             if isinstance(getattr(getattr(d.get("pipeline"), "config", None), "function", None), ir.ExprProgram)]
    rops = [[fl.rop for fl in p.reduce.fields] for p in progs if p.reduce is not None]
    first = ["nansum"] if fn == "nansum" else ["count_nonnan", "nansum"]
    assert rops == [first, ["sum"] * len(first)]
    assert len([s for s in lower(y) if s.nfields > 0]) == 2


def test_bf16_readback_keeps_a_0d_shape():
    bits = ir.numpy_to_bf16(np.array([1.5, -2.0], dtype=np.float32))
    assert ir.bf16_to_numpy(bits).shape == (2,)
    assert ir.bf16_to_numpy(bits[0]).shape == () and float(ir.bf16_to_numpy(bits[0])) == 1.5
    assert ir.bf16_to_numpy(bits.reshape(1, 2, 1)).shape == (1, 2, 1)


def test_a_geometry_that_misses_its_form_fails(lowered):
    lower, spec = lowered
    f = M.REDUCE_FORMS["stream-split"]
    x = cubed.from_array(np.zeros((64, 1024)), chunks=(16, 1020), spec=spec)  # ragged inner chunks: no stream
    seen = lower(xp.sum(x, axis=0))
    with pytest.raises(AssertionError):
        M.assert_form_ran(seen, "stream-split", ["float64"], jit=False)
    seen = lower(xp.sum(_zeros("stream-split", "float64", spec), axis=f["axis"]))
    M.assert_form_ran(seen, "stream-split", ["float64"], jit=False)
    with pytest.raises(AssertionError):
        M.assert_form_ran(seen, "stream-split", ["float64"], jit=True)
    with pytest.raises(AssertionError):
        M.assert_form_ran(seen, "stream-split", ["float64", "float64"], jit=False)
    with pytest.raises(AssertionError):
        M.assert_form_ran(seen, "vec4-unsplit", ["float64"], jit=False)


# ------------------------------------------------------------------ the inputs
def _inputs(form, dtype, kind):
    f = M.REDUCE_FORMS[form]
    for v in range(M.reduce_variants(dtype, f["shape"], f["axis"])):
        yield (f,) + M.reduce_inputs(kind, dtype, f["shape"], f["axis"], variant=v)


@pytest.mark.parametrize("dtype", ["float32", "float64", "bfloat16"])
@pytest.mark.parametrize("form", FORMS)
def test_float_inputs_keep_the_magnitude_conditions(form, dtype):
    """float_reduce_bounds asserts them on the reference: sum|v| < max / 2 of
    the narrowest result dtype, every subset of a product's factors normal in
    float64 and the product normal in the result dtype."""
    out = M.reduce_dtype(dtype)
    told = set()
    for f, x, stories in _inputs(form, dtype, "sum"):
        told |= set(stories.ravel())
        assert x.dtype == (np.float32 if dtype == "bfloat16" else out)
        if dtype == "bfloat16":
            assert np.array_equal(ir.bf16_to_numpy(ir.numpy_to_bf16(x)).reshape(x.shape), x, equal_nan=True)
        for fn in ("sum", "nanmean"):
            ref, tol, finite = M.float_reduce_bounds(fn, x, f["axis"], out)
            assert np.all(tol[finite] > 0) and np.array_equal(finite, np.isfinite(ref))
    assert told == set(M.FLOAT_STORIES)
    for f, x, stories in _inputs(form, dtype, "prod"):
        ref, tol, finite = M.float_reduce_bounds("prod", x, f["axis"], out)
        plain = np.isin(stories, ["ordinary", "all_equal", "negative", "positive"])
        assert np.all(finite[plain]) and np.all(ref[plain] != 0)
        if dtype != "bfloat16":  # (bfloat16 rounds most of such factors to 1)
            r = M.reduce_counts(f["shape"], f["axis"])[0]
            factors = x[np.isfinite(x) & (x != 0)]
            assert np.all(np.abs(np.log2(np.abs(factors))) <= M.prod_exponent_bound(r) * 1.001)


def test_float_stories_are_what_they_say():
    f = M.REDUCE_FORMS["stream-split"]
    x, stories = M.reduce_inputs("sum", "float32", f["shape"], f["axis"])
    r = f["shape"][0]
    col = {s: x[:, stories == s] for s in M.FLOAT_STORIES}
    assert all(c.shape[1] >= 4 for c in col.values())  # every placement of the special values
    assert np.isfinite(col["ordinary"]).all() and (col["ordinary"] != 0).all()
    for s in ("one_nan", "neg_nan", "pos_inf", "one_neg_zero"):
        special = {"one_nan": np.isnan, "neg_nan": lambda v: np.isnan(v) & np.signbit(v), "pos_inf": np.isposinf,
                   "one_neg_zero": lambda v: (v == 0) & np.signbit(v)}[s](col[s])
        assert (special.sum(axis=0) == 1).all(), s
        # first row, last row, the middle, a third of the way: different chunks and splits
        assert set(np.argwhere(special)[:, 0]) == {0, r - 1, r // 2, r // 3}, s
    assert not np.signbit(col["one_nan"][np.isnan(col["one_nan"])]).any()
    last = np.isnan(col["nan_last_row"])
    assert last[-1].all() and not last[:-1].any()
    assert np.isnan(col["all_nan"]).all() and np.signbit(col["all_nan"]).any() and not np.signbit(col["all_nan"]).all()
    both = col["both_inf"]
    assert (np.isposinf(both).sum(axis=0) == 1).all() and (np.isneginf(both).sum(axis=0) == 1).all()
    assert {0, r - 1} <= set(np.argwhere(np.isinf(both))[:, 0])
    assert (col["all_neg_zero"] == 0).all() and np.signbit(col["all_neg_zero"]).all()
    mixed = col["mixed_zero"]
    assert (mixed == 0).all() and np.signbit(mixed).any(axis=0).all() and (~np.signbit(mixed)).any(axis=0).all()
    assert (col["all_equal"] == col["all_equal"][0]).all()
    assert (col["negative"] < 0).all() and (col["positive"] > 0).all()


@pytest.mark.parametrize("form", ["scalar-all", "b-split", "lifted", "full-b-split", "3d-axes02"])
def test_special_values_move_between_the_variants(form):
    """Forms with fewer kept elements than stories: the variants put a
    story's special value in the first and last reduced row and in the
    middle too, not at one spot."""
    f = M.REDUCE_FORMS[form]
    r, k = M.reduce_counts(f["shape"], f["axis"])
    assert k < len(M.FLOAT_STORIES)
    red = M.reduce_axes(f["axis"], len(f["shape"]))
    kept = tuple(a for a in range(len(f["shape"])) if a not in red)
    where = {}
    for _, x, stories in _inputs(form, "float64", "sum"):
        cols = x.transpose(red + kept).reshape(r, k)
        for j, s in enumerate(stories.ravel()):
            if s in ("one_nan", "neg_nan", "pos_inf", "both_inf"):
                where.setdefault(s, set()).update(np.flatnonzero(~np.isfinite(cols[:, j])).tolist())
    spots = set().union(*where.values())
    assert set(where) == {"one_nan", "neg_nan", "pos_inf", "both_inf"}
    assert {0, r - 1} <= spots and spots & {r // 2, r // 3}, spots
    assert len({tuple(sorted(v)) for v in where.values()}) >= 2  # the stories do not all share one spot


@pytest.mark.parametrize("dtype", [d for d in M.REDUCE_DTYPES if M.reduce_dtype(d).kind in "iu"])
def test_integer_stories_are_what_they_say(dtype):
    f = M.REDUCE_FORMS["vec4-split"]  # 200 reduced rows
    dt = np.dtype(dtype)
    ii = np.iinfo(dt)
    x, stories = M.reduce_inputs("sum", dtype, f["shape"], f["axis"])
    assert x.dtype == dt and set(stories) == set(M.INT_STORIES)
    col = {s: x[:, stories == s] for s in M.INT_STORIES}
    both = col["min_and_max"]
    assert ((both == ii.min).sum(axis=0) == 1).all() and ((both == ii.max).sum(axis=0) == 1).all()
    assert (col["all_min"] == ii.min).all() and (col["all_max"] == ii.max).all() and (col["all_zero"] == 0).all()
    assert ((col["single_nonzero"] != 0).sum(axis=0) == 1).all()
    exact = [sum(int(v) for v in c) for c in col["wrap_sum"].T]
    assert all(not ii.min <= s <= ii.max for s in exact)  # the sum of the dtype's own width wraps
    if dt.itemsize == 8:
        top = 2 ** 62 if dt.kind == "i" else 2 ** 63
        assert (np.abs(col["wrap_sum"].astype(np.longdouble) - top) < 8).all()
    if dt.kind == "u":
        half = ii.max // 2 + 1  # uint64: values on both sides of 2^63
        for s in ("wrap_sum", "ordinary"):
            assert (col[s] >= half).any() and (col[s] < half).any(), s
        assert (col["single_nonzero"].max(axis=0) == half + 1).all()
    p, _ = M.reduce_inputs("prod", dtype, f["shape"], f["axis"])
    for s in ("prod_wrap", "prod_zero"):
        c = p[:, stories == s]
        assert np.isin(c, [0, 2, 3]).all() and ((c == 0).sum(axis=0) == (s == "prod_zero")).all()
        assert ((c == 2).sum(axis=0) > 0).all() and ((c == 3).sum(axis=0) > 100).all()  # 3^100 > 2^64
    with np.errstate(all="ignore"):
        wrapped = np.prod(p[:, stories == "prod_wrap"], axis=0, dtype=np.uint64)
    assert (wrapped != 0).all()
    assert (p[:, stories == "ordinary"] % 2 == 1).all()  # odd factors: the wrapped product is not zero


def test_bool_stories():
    f = M.REDUCE_FORMS["scalar-axis1"]
    told = set()
    for _, x, stories in _inputs("scalar-axis1", "bool", "sum"):
        assert x.dtype == np.bool_
        told |= set(stories)
        assert np.array_equal(np.any(x, axis=f["axis"])[stories == "all_zero"], [False] * (stories == "all_zero").sum())
        assert not np.all(x, axis=f["axis"])[stories == "prod_zero"].any()
        assert np.any(x, axis=f["axis"])[stories == "single_nonzero"].all()
    assert told == set(M.BOOL_STORIES)


@pytest.mark.parametrize("form", FORMS)
def test_every_story_is_reduced_in_every_cell(form):
    f = M.REDUCE_FORMS[form]
    for dtype in ("bool", "uint8", "float64"):
        told = set()
        for _, x, stories in _inputs(form, dtype, "sum"):
            assert x.shape == f["shape"]
            assert stories.shape == np.empty(f["shape"], dtype=bool).sum(axis=f["axis"]).shape
            told |= set(stories.ravel())
        assert told == set(M.stories_for(dtype))


def test_reduce_cases():
    for dtype in M.REDUCE_DTYPES:
        cases = M.reduce_cases(dtype)
        assert len(set(cases)) == len(cases)
        assert {fn for fn, _ in cases} >= {"any", "all"}
    assert {("sum", "float32"), ("prod", "float32"), ("nansum", "float32")} <= set(M.reduce_cases("float32"))
    assert {("sum", "int8"), ("prod", "int8"), ("nansum", "int8")} <= set(M.reduce_cases("int8"))
    assert {("sum", "uint64"), ("prod", "uint64"), ("nansum", "uint64")} <= set(M.reduce_cases("uint8"))
    assert {fn for fn, _ in M.reduce_cases("bfloat16")} == set(M.FLOAT_REDUCTIONS)
    assert {fn for fn, _ in M.reduce_cases("uint64")} == set(M.INT_REDUCTIONS)
    assert M.reduce_cases("bool") == [("any", None), ("all", None)]
    # the array API's result dtypes, as the functions themselves give them
    spec = cubed.Spec(allowed_mem="2GB")
    for dtype in M.REDUCE_DTYPES:
        x = cubed.from_array(np.zeros((4, 4), dtype=M.reduce_dtype(dtype)), chunks=(2, 2), spec=spec)
        for fn, explicit in M.reduce_cases(dtype):
            kw = {} if explicit is None else dict(dtype=np.dtype(explicit))
            f = getattr(cubed, fn) if fn.startswith("nan") else getattr(xp, fn)
            assert f(x, **kw).dtype == M.reduce_result_dtype(fn, M.reduce_dtype(dtype), explicit), (fn, dtype)


# ------------------------------------------------------------------ the checker
def _right(fn, x, axis, dtype=None, keepdims=False):
    """A correct result computed the plain way."""
    with np.errstate(all="ignore"):
        out = M.reduce_result_dtype(fn, x.dtype, dtype)
        if fn in ("any", "all", "max", "min"):
            return np.asarray(getattr(np, fn)(x, axis=axis, keepdims=keepdims))
        if x.dtype.kind != "f":
            return np.asarray(getattr(np, fn)(x, axis=axis, keepdims=keepdims, dtype=out))
        return np.asarray(getattr(np, fn)(x.astype(np.float64), axis=axis, keepdims=keepdims)).astype(out)


def _check(fn, x, got, stories, axis=0, dtype=None, keepdims=False):
    M.check_reduction(fn, x, got, axis, x.dtype, dtype=dtype, keepdims=keepdims, stories=stories, what=fn)


def _rejects(fn, x, got, stories, story, **kw):
    with pytest.raises(AssertionError) as e:
        _check(fn, x, got, stories, **kw)
    assert story in str(e.value), str(e.value)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_checker_accepts_right_results_and_rejects_wrong_ones():
    f = M.REDUCE_FORMS["vec4-split"]
    x, stories = M.reduce_inputs("sum", "float32", f["shape"], 0)
    at = {s: int(np.argmax(stories == s)) for s in M.FLOAT_STORIES}
    for fn in M.FLOAT_REDUCTIONS:
        _check(fn, x, _right(fn, x, 0), stories)
    # a NaN dropped from a max (the NaN-ignoring maximum), of either sign, first row or last
    for s in ("one_nan", "nan_last_row", "neg_nan"):
        got = _right("max", x, 0)
        got[at[s]] = np.nanmax(x[:, at[s]])
        _rejects("max", x, got, stories, s)
    got = _right("min", x, 0)
    got[:] = np.nanmin(x, axis=0, initial=np.inf)  # all of them dropped
    _rejects("min", x, got, stories, "all_nan")
    # a NaN added where none belongs
    for fn in ("max", "sum", "mean", "nansum", "nanmean"):
        got = _right(fn, x, 0)
        got[at["ordinary"]] = np.nan
        _rejects(fn, x, got, stories, "ordinary")
    got = _right("nansum", x, 0)
    got[at["all_nan"]] = np.nan  # numpy's nansum of NaNs is 0
    _rejects("nansum", x, got, stories, "all_nan")
    got = _right("nanmean", x, 0)
    got[at["all_nan"]] = 0.0  # ... and the nanmean of nothing is NaN
    _rejects("nanmean", x, got, stories, "all_nan")
    # inf with the wrong sign; a NaN sum of +inf and -inf turned into an inf
    for fn in ("sum", "mean", "max", "nansum"):
        got = _right(fn, x, 0)
        got[at["pos_inf"]] = -np.inf
        _rejects(fn, x, got, stories, "pos_inf")
    got = _right("sum", x, 0)
    got[at["both_inf"]] = np.inf
    _rejects("sum", x, got, stories, "both_inf")
    # the sign of a NaN, of a zero sum and of a zero max is nobody's business
    for fn in ("sum", "max"):
        got = _right(fn, x, 0)
        got[at["one_nan"]] = M.NEG_NAN
        got[at["all_neg_zero"]] = 0.0
        got[at["mixed_zero"]] = -0.0
        _check(fn, x, got, stories)
    # a float sum off by twice the tolerance, by half of it
    for fn, out in (("sum", np.float64), ("sum", np.float32), ("nansum", np.float64), ("mean", np.float32),
                    ("nanmean", np.float32)):
        dtype = out if fn in ("sum", "nansum") else None
        ref, tol, finite = M.float_reduce_bounds(fn, x, 0, out)
        k = at["negative"]
        assert finite[k]
        got = _right(fn, x, 0, dtype)
        got[k] = (ref[k] + 2 * tol[k]).astype(out)
        _rejects(fn, x, got, stories, "negative", dtype=dtype)
        got[k] = (ref[k] - tol[k] / 2).astype(out)
        _check(fn, x, got, stories, dtype=dtype)
    # a float32 sum accumulated in float32: 200 roundings where one is allowed
    with np.errstate(all="ignore"):
        got = np.zeros(x.shape[1], dtype=np.float32)
        for row in x[::-1]:
            got = (got + row).astype(np.float32)
    with pytest.raises(AssertionError):
        _check("sum", x, got, stories, dtype=np.float32)
    # the right values in the wrong dtype; a keepdims shape lost
    with pytest.raises(AssertionError, match="dtype"):
        _check("sum", x, _right("sum", x, 0).astype(np.float32), stories)
    with pytest.raises(AssertionError, match="dtype"):
        _check("mean", x, _right("mean", x, 0).astype(np.float64), stories)
    with pytest.raises(AssertionError, match="shape"):
        _check("max", x, _right("max", x, 0), stories, keepdims=True)
    _check("max", x, _right("max", x, 0, keepdims=True), stories, keepdims=True)
    with pytest.raises(AssertionError, match="shape"):
        _check("max", x, _right("max", x, 0, keepdims=True), stories)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_checker_products():
    f = M.REDUCE_FORMS["vec4-split"]
    x, stories = M.reduce_inputs("prod", "float32", f["shape"], 0)
    at = {s: int(np.argmax(stories == s)) for s in M.FLOAT_STORIES}
    for dtype in (None, np.float32):
        _check("prod", x, _right("prod", x, 0, dtype), stories, dtype=dtype)
    got = _right("prod", x, 0)
    got[at["positive"]] *= 1 + 400 * 2.0 ** -53  # twice the bound of 200 factors
    _rejects("prod", x, got, stories, "positive")
    got = _right("prod", x, 0)
    got[at["one_neg_zero"]] = 1e-300  # a zero factor lost
    _rejects("prod", x, got, stories, "one_neg_zero")
    got = _right("prod", x, 0)
    got[at["both_inf"]] *= -1
    _rejects("prod", x, got, stories, "both_inf")
    with pytest.raises(AssertionError, match="normal"):  # factors the bound does not hold for
        M.float_reduce_bounds("prod", np.full((400, 2), 1.5), 0, np.float32)
    with pytest.raises(AssertionError, match="overflow"):
        M.float_reduce_bounds("sum", np.full((4, 2), 1e38, dtype=np.float32), 0, np.float32)


def test_checker_integers():
    f = M.REDUCE_FORMS["vec4-split"]
    x, stories = M.reduce_inputs("sum", "int64", f["shape"], 0)
    at = {s: int(np.argmax(stories == s)) for s in M.INT_STORIES}
    for fn in M.INT_REDUCTIONS:
        _check(fn, x, _right(fn, x, 0), stories)
    # an int64 sum saturated instead of wrapped
    exact = sum(int(v) for v in x[:, at["wrap_sum"]])
    assert exact > 2 ** 63
    got = _right("sum", x, 0)
    assert got[at["wrap_sum"]] == ((exact + 2 ** 63) % 2 ** 64) - 2 ** 63
    got[at["wrap_sum"]] = np.iinfo(np.int64).max
    _rejects("sum", x, got, stories, "wrap_sum")
    # a uint64 max computed as signed: 2^63 + 1 loses to everything below 2^63
    u, ustories = M.reduce_inputs("sum", "uint64", f["shape"], 0)
    for fn in ("max", "min"):
        signed = getattr(np, fn)(u.view(np.int64), axis=0).view(np.uint64)
        _check(fn, u, _right(fn, u, 0), ustories)
        with pytest.raises(AssertionError) as e:
            _check(fn, u, signed, ustories)
        assert "min_and_max" in str(e.value) and "ordinary" in str(e.value)
    # the right values in the wrong dtype; an explicit narrow dtype wraps at its own width
    with pytest.raises(AssertionError, match="dtype"):
        _check("max", u, _right("max", u, 0).astype(np.int64), ustories)
    b, bstories = M.reduce_inputs("sum", "int8", f["shape"], 0)
    _check("sum", b, _right("sum", b, 0, np.int8), bstories, dtype=np.int8)
    with pytest.raises(AssertionError, match="dtype"):
        _check("sum", b, _right("sum", b, 0), bstories, dtype=np.int8)
    got = np.clip(_right("sum", b, 0), -128, 127).astype(np.int8)
    _rejects("sum", b, got, bstories, "wrap_sum", dtype=np.int8)
    # any / all of floats: NaN is true, -0.0 is false
    x, stories = M.reduce_inputs("sum", "float64", f["shape"], 0)
    k, z = int(np.argmax(stories == "all_nan")), int(np.argmax(stories == "all_neg_zero"))
    got = _right("any", x, 0)
    assert got[k] and not got[z]
    got[k] = False
    _rejects("any", x, got, stories, "all_nan")
    got = _right("any", x, 0)
    got[z] = True
    _rejects("any", x, got, stories, "all_neg_zero")
    with pytest.raises(AssertionError, match="shape"):
        _check("all", x, _right("all", x, 0), stories, keepdims=True)


def test_bfloat16_spacing():
    v = np.array([1.0, 1.5, 255.0, 2.0 ** -126, 0.0], dtype=np.float32)
    assert np.array_equal(M.spacing_in(v, ir.bfloat16).astype(np.float64),
                          [2.0 ** -7, 2.0 ** -7, 1.0, 2.0 ** -133, 2.0 ** -133])
    assert np.array_equal(M.spacing_in(v, np.float32).astype(np.float32), np.spacing(v))
