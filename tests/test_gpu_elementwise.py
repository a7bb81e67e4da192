"""Elementwise conformance on the GPU: every op of the per-element VM
(cubed_amd/csrc/vm.h) against numpy applied to the same host arrays, on each
kernel family -- the ahead-of-time interpreter (CUBED_AMD_JIT=0), the
hipRTC-specialised kernels (the default) and the streaming kernels.  A spy on
lowering.FusedLaunch records the register type, the mode bits and whether a
JIT handle exists, so each test knows which kernel form ran.

Inputs (vm_model.py): per dtype an edge vector, the Cartesian product of the
edge vectors for binary ops, then seeded random fill.  Nothing is masked:
what numpy leaves undefined (negative shift counts, negative integer
exponents, float -> int casts of NaN / inf / out-of-range values) is kept out
of the inputs by construction.

Equality (bit-exact unless stated): maximum / minimum are value-equal with
NaN in the same places (numpy's own sign of a zero result differs between
its scalar and SIMD loops); transcendentals, float pow, hypot, atan2 and
logaddexp are within ULP_BASELINE[...] + 4 ulps of a higher-precision numpy
reference (float64 for f16 / f32 results, longdouble for f64), with NaN / inf
positions and signs equal."""
import math
import operator

import numpy as np
import pytest

import cubed_amd as cubed
import cubed_amd.array_api as xp
import vm_model as M
from cubed_amd import ir
from cubed_amd import lowering as L
from gpu_fixtures import arr, interp, jit, spy  # noqa: F401  (the fixtures are used by name)

pytestmark = pytest.mark.gpu

GEOMS = {"vec4": ((24, 32), (8, 16)),   # inner chunk extent a multiple of 4: VEC = 4
         "ragged": ((7, 13), (3, 5))}   # ragged: VEC = 1
MODE_VEC4, MODE_STREAM = 4, 8
DTYPES = [d.name for d in M.REAL_DTYPES]
# the array-API functions take no float16 (array_api/dtypes.py): it is cast
# to and from here, and its ops are covered on the host model (test_codegen.py)
OP_DTYPES = [d for d in DTYPES if d != "float16"]

# numpy's own same-dtype error against the higher-precision reference, in
# ulps rounded up, measured on the CPU over exactly the inputs used below
# (vm_model.unary_inputs / binary_inputs at n = 91, 768 and 65536, seed 0).
# The kernels are allowed this + 4 ulps: the device math library is of
# OpenCL accuracy class (a few ulps) where numpy's SIMD routines are <= 1.
# Each entry: numpy's baseline rounded up, with the measured f32, f64 values
# beside it.  The logaddexp entries are numpy's own cancellation in
# x + log1p(exp(y - x)) near a zero result.
ULP_BASELINE = {
    ("acos", "float32"): 2, ("acos", "float64"): 1,        # 1.228, 0.731
    ("acosh", "float32"): 1, ("acosh", "float64"): 1,      # 0.560, 0.499
    ("asin", "float32"): 3, ("asin", "float64"): 1,        # 2.109, 0.699
    ("asinh", "float32"): 1, ("asinh", "float64"): 1,      # 0.579, 0.543
    ("atan", "float32"): 1, ("atan", "float64"): 1,        # 0.957, 0.511
    ("atan2", "float32"): 3, ("atan2", "float64"): 1,      # 2.080, 0.625
    ("atanh", "float32"): 1, ("atanh", "float64"): 1,      # 0.826, 0.553
    ("cos", "float32"): 1, ("cos", "float64"): 1,          # 0.985, 0.499
    ("cosh", "float32"): 2, ("cosh", "float64"): 1,        # 1.636, 0.723
    ("exp", "float32"): 3, ("exp", "float64"): 1,          # 2.190, 0.601
    ("expm1", "float32"): 2, ("expm1", "float64"): 1,      # 1.646, 0.500
    ("hypot", "float32"): 1, ("hypot", "float64"): 1,      # 0.499, 0.501
    ("log", "float32"): 2, ("log", "float64"): 1,          # 1.584, 0.522
    ("log10", "float32"): 2, ("log10", "float64"): 1,      # 1.459, 0.525
    ("log1p", "float32"): 2, ("log1p", "float64"): 1,      # 1.181, 0.556
    ("log2", "float32"): 2, ("log2", "float64"): 1,        # 1.187, 0.500
    ("logaddexp", "float32"): 6, ("logaddexp", "float64"): 11,  # 5.315, 10.594
    ("pow", "float32"): 1, ("pow", "float64"): 1,          # 0.939, 0.625
    ("sin", "float32"): 1, ("sin", "float64"): 1,          # 0.948, 0.514
    ("sinh", "float32"): 1, ("sinh", "float64"): 1,        # 0.931, 0.775
    ("tan", "float32"): 3, ("tan", "float64"): 1,          # 2.265, 0.503
    ("tanh", "float32"): 2, ("tanh", "float64"): 1,        # 1.271, 0.903
}
ULP_SLACK = 4


# ------------------------------------------------------------------ comparison
def high_precision(op, xs):
    dt = xs[0].dtype
    hp = np.float64 if dt.itemsize < 8 else np.longdouble
    with np.errstate(all="ignore"):
        return M.np_op(op, *[x.astype(hp) for x in xs])


def compare(op, xs, got, what):
    """``got`` against numpy's op(*xs) under the rule of the op's class."""
    dt = xs[0].dtype
    with np.errstate(all="ignore"):
        exp = M.np_op(op, *xs)
    name = op
    if M.is_ulp(name, dt):
        if dt.itemsize == 8 and np.finfo(np.longdouble).nmant < 63:
            pytest.skip("no float type wider than float64 for the reference")
        assert got.dtype == exp.dtype and got.shape == exp.shape, what
        ref = high_precision(name, np.broadcast_arrays(*xs))
        err = M.ulp_error(got, ref, dt)
        bound = ULP_BASELINE[(name, dt.name)] + ULP_SLACK
        worst = np.unravel_index(np.argmax(err), err.shape)
        print(f"ulp {name} {dt.name}: max {err.max():.2f} (bound {bound})")
        assert err.max() <= bound, (what, float(err.max()), bound,
                                    [np.broadcast_arrays(*xs)[i][worst] for i in range(len(xs))], got[worst])
    elif name in M.ZERO_SIGN_FREE:
        M.assert_value_equal(got, exp, what)
    else:
        M.assert_bit_equal(got, exp, what)


OPERATORS = {"add": operator.add, "subtract": operator.sub, "multiply": operator.mul, "divide": operator.truediv,
             "floor_divide": operator.floordiv, "remainder": operator.mod, "pow": operator.pow,
             "less": operator.lt, "less_equal": operator.le, "greater": operator.gt, "greater_equal": operator.ge,
             "equal": operator.eq, "not_equal": operator.ne, "bitwise_and": operator.and_,
             "bitwise_or": operator.or_, "bitwise_xor": operator.xor, "bitwise_left_shift": operator.lshift,
             "bitwise_right_shift": operator.rshift}


def python_scalar(dtype):
    k = np.dtype(dtype).kind
    return True if k == "b" else (3 if k in "iu" else 2.5)


def build_matrix(spec, dtype, geom, ops=None, variants=True):
    """Lazy arrays and their checks for every op valid at ``dtype``: array
    operands, plus (binary ops) a broadcast row operand at the vec4 geometry
    and a Python scalar at the ragged one."""
    shape, chunks = GEOMS[geom]
    n = shape[0] * shape[1]
    un, bi = M.ops_for(dtype, extra=False)
    lazy, checks = [], []
    for op in un:
        if ops is not None and op not in ops:
            continue
        x = M.unary_inputs(op, dtype, n).reshape(shape)
        lazy.append(getattr(xp, op)(arr(x, chunks, spec)))
        checks.append((op, [x], f"{op}({dtype}) {geom}"))
    for op in bi:
        if ops is not None and op not in ops:
            continue
        a, b = [v.reshape(shape) for v in M.binary_inputs(op, dtype, n)]
        A = arr(a, chunks, spec)
        lazy.append(getattr(xp, op)(A, arr(b, chunks, spec)))
        checks.append((op, [a, b], f"{op}({dtype}, {dtype}) {geom}"))
        if not variants:
            continue
        if geom == "vec4":
            row = np.resize(M._second_operand(op, dtype), shape[1])
            lazy.append(getattr(xp, op)(A, arr(row, (chunks[1],), spec)))
            checks.append((op, [a, row], f"{op}({dtype}, row) {geom}"))
        elif op in OPERATORS:
            s = python_scalar(dtype)
            lazy.append(OPERATORS[op](A, s))
            checks.append((op, [a, np.asarray(s, dtype=dtype)], f"{op}({dtype}, {s!r}) {geom}"))
    return lazy, checks


def run_matrix(lazy, checks):
    got = cubed.compute(*lazy)
    failures = []
    for g, (op, xs, what) in zip(got, checks):
        try:
            compare(op, xs, np.asarray(g), what)
        except AssertionError as e:
            failures.append(f"{what}: {str(e)[:300]}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ interpreter
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("dtype", OP_DTYPES)
def test_interpreter_matrix(interp, spy, dtype, geom):
    """Every op valid at ``dtype`` on the ahead-of-time interpreter."""
    lazy, checks = build_matrix(interp, dtype, geom)
    run_matrix(lazy, checks)
    assert spy and not any(h for _, _, h in spy), "the interpreter kernels must have run"
    # (contiguous maps over leaves of the register type's own dtype -- int64,
    # float32, float64 at the vec4 geometry -- run on the streaming kernels)
    want = {"b": {L.V_I64}, "i": {L.V_I64}, "u": {L.V_I64},
            "f": {L.V_F32} if np.dtype(dtype).itemsize < 8 else {L.V_F64}}[np.dtype(dtype).kind]
    assert {v for v, _, _ in spy} == want
    if geom == "ragged":
        assert not any(m & MODE_VEC4 for _, m, _ in spy)
    else:
        assert any(m & MODE_VEC4 for _, m, _ in spy)


# ------------------------------------------------------------------ JIT
def _home(op):
    """Home dtype of an op under the JIT: f32 for float ops, uint64 for the
    ordered, division and shift ops, i32 for the other integer ops."""
    cat = dict(M.UNARY_API, **M.BINARY_API)[op]
    if op in L._UNSIGNED_OPS:
        return "uint64"
    if op.startswith("logical"):
        return "bool"
    if op.startswith("bitwise") or op in ("equal", "not_equal"):
        return "int32"
    return "float32" if "f" in cat else "int32"


_JIT_OPS = sorted(set(M.UNARY_API) | set(M.BINARY_API))
_JIT_GROUPS = [_JIT_OPS[i:i + 2] for i in range(0, len(_JIT_OPS), 2)]


@pytest.mark.parametrize("group", _JIT_GROUPS, ids=["-".join(g) for g in _JIT_GROUPS])
def test_jit_ops(jit, spy, group):
    """Each op once at its home dtype on the hipRTC-specialised kernels
    (one compile of about two seconds per op: two ops per test)."""
    lazy, checks = [], []
    for op in group:
        lz, ck = build_matrix(jit, _home(op), "vec4", ops={op}, variants=False)
        lazy += lz
        checks += ck
    run_matrix(lazy, checks)
    # (positive is a plain copy: no fused program)
    assert len(spy) >= len([op for op in group if op != "positive"]) and all(h for _, _, h in spy), \
        "the specialised kernels must have run"


def _mixed_cases(spec):
    """(lazy array, numpy reference) of the fused programs that were wrong
    while integer nodes ran in float registers / uint64 as signed."""
    shape, chunks = GEOMS["vec4"]
    n = shape[0] * shape[1]
    out = []

    def two(op, dt):
        a, b = [v.reshape(shape) for v in M.binary_inputs(op, dt, n)]
        return a, b, arr(a, chunks, spec), arr(b, chunks, spec)

    with np.errstate(all="ignore"):
        a, b, A, B = two("bitwise_left_shift", "int32")
        out.append(("astype(i32 << i32, f64)", xp.astype(A << B, xp.float64), (a << b).astype("f8")))
        a, b, A, B = two("multiply", "int16")
        out.append(("astype(i16 * i16, f32)", xp.astype(A * B, xp.float32), (a * b).astype("f4")))
        a, b, A, B = two("floor_divide", "int64")
        out.append(("astype(i64 // i64, f64)", xp.astype(A // B, xp.float64), (a // b).astype("f8")))
        out.append(("astype(i64 * i64, f64)", xp.astype(A * B, xp.float64), (a * b).astype("f8")))
        f = np.random.default_rng(4).standard_normal(shape)
        F = arr(f, chunks, spec)
        out.append(("where(f64 > 0, i64 < i64, ..)", xp.where(F > 0, A < B, A > B), np.where(f > 0, a < b, a > b)))
        out.append(("where(f64 > 0, i64, i64)", xp.where(F > 0, A, B), np.where(f > 0, a, b)))
        a, b, A, B = two("pow", "int64")
        out.append(("astype(i64 ** i64, f64)", xp.astype(A ** B, xp.float64), (a ** b).astype("f8")))
        a, b, A, B = two("bitwise_right_shift", "uint64")
        out.append(("astype(u64 >> u64, f64)", xp.astype(A >> B, xp.float64), (a >> b).astype("f8")))
        a, b, A, B = two("remainder", "uint64")
        out.append(("where(f64 > 0, u64 % u64, u64 // u64)", xp.where(F > 0, A % B, A // B),
                    np.where(f > 0, a % b, a // b)))
        out.append(("abs(u64)", xp.abs(A), np.abs(a)))
        out.append(("sign(u64)", xp.sign(A), np.sign(a)))
        big = np.resize(np.array([2.0 ** 63, 2.0 ** 63 + 2048, 2.0 ** 64 - 2048, 1.5, 0.0, 2.0 ** 53 + 2]), shape)
        out.append(("astype(f64 >= 2^63, u64)", xp.astype(arr(big, chunks, spec), xp.uint64), big.astype("u8")))
        out.append(("astype(f64 * 1, u64)", xp.astype(arr(big, chunks, spec) * 1.0, xp.uint64), big.astype("u8")))
        t = np.resize(np.array([1 + 2.0 ** -11 + 2.0 ** -30, -(1 + 2.0 ** -11 + 2.0 ** -30), 0.1, 65519.9]), shape)
        out.append(("astype(f64, f16)", xp.astype(arr(t, chunks, spec), np.float16), t.astype("f2")))
    return out


@pytest.mark.parametrize("part", range(7))
def test_jit_mixed_programs(jit, spy, part):
    cases = _mixed_cases(jit)[part::7]
    got = cubed.compute(*[c[1] for c in cases])
    for g, (what, _, exp) in zip(got, cases):
        M.assert_bit_equal(np.asarray(g), exp, what)
    assert spy and all(h for _, _, h in spy)


def test_jit_signed_and_float_forms(jit, spy):
    """The ops whose JIT home dtype is uint64, once more in their signed and
    float forms (npy_max, ifloordiv, imod, the arithmetic right shift)."""
    lazy, checks = [], []
    for op, dt in [("maximum", "float32"), ("bitwise_right_shift", "int64"), ("floor_divide", "int64"),
                   ("remainder", "int64")]:
        lz, ck = build_matrix(jit, dt, "vec4", ops={op}, variants=False)
        lazy += lz
        checks += ck
    run_matrix(lazy, checks)
    assert len(spy) >= 4 and all(h for _, _, h in spy)


def test_interpreter_mixed_programs(interp, spy):
    cases = _mixed_cases(interp)
    got = cubed.compute(*[c[1] for c in cases])
    for g, (what, _, exp) in zip(got, cases):
        M.assert_bit_equal(np.asarray(g), exp, what)
    assert spy and not any(h for _, _, h in spy)


@pytest.mark.parametrize("path", ["jit", "interpreter"])
def test_f32_divide_sqrt_correctly_rounded(request, spy, path):
    """f32 / and sqrt are bit-exact against numpy at 4096 random operand
    pairs on both paths (both builds pass
    -fhip-fp32-correctly-rounded-divide-sqrt)."""
    spec = request.getfixturevalue("jit" if path == "jit" else "interp")
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(4096) * np.exp(rng.uniform(-40, 40, 4096))).astype("f4")
    b = (rng.standard_normal(4096) * np.exp(rng.uniform(-40, 40, 4096))).astype("f4")
    A, B = arr(a, (1024,), spec), arr(b, (1024,), spec)
    q, r = cubed.compute(xp.divide(A, B), xp.sqrt(xp.abs(A)))
    with np.errstate(all="ignore"):
        M.assert_bit_equal(np.asarray(q), a / b, "f32 divide")
        M.assert_bit_equal(np.asarray(r), np.sqrt(np.abs(a)), "f32 sqrt")
    assert spy and all(h == (path == "jit") for _, _, h in spy)
    assert {v for v, _, _ in spy} == {L.V_F32}


# ------------------------------------------------------------------ streaming
STREAM_SHAPE, STREAM_CHUNKS = (64, 1024), (16, 1024)
STREAM_OPS = {
    "float32": ["add", "subtract", "multiply", "maximum", "minimum", "floor_divide", "remainder", "where", "exp"],
    "float64": ["add", "subtract", "multiply", "maximum", "minimum", "floor_divide", "remainder", "where", "sin"],
    "int64": ["add", "subtract", "multiply", "maximum", "minimum", "floor_divide", "remainder", "where",
              "bitwise_xor"],
}


def stream_inputs(op, dtype):
    """Two operands of STREAM_SHAPE.  Floats leave +-max out: a column's sum
    of +max and -max terms overflows or not with the order of the additions,
    in numpy's pairwise sum as much as in the kernel's."""
    n = STREAM_SHAPE[0] * STREAM_SHAPE[1]
    a, b = M.binary_inputs("add" if op in ("where", "exp", "sin") else op, dtype, n)
    if np.dtype(dtype).kind == "f":
        big = np.finfo(dtype).max
        a = np.where(np.abs(a) == big, a.dtype.type(7.5), a)
        b = np.where(np.abs(b) == big, b.dtype.type(-3.25), b)
    rng = np.random.default_rng(11)
    return rng.permutation(a).reshape(STREAM_SHAPE), rng.permutation(b).reshape(STREAM_SHAPE)


@pytest.mark.parametrize("dtype", list(STREAM_OPS))
@pytest.mark.parametrize("which", [0, 1, 2])
def test_stream_sum_of_op(interp, spy, dtype, which):
    """xp.sum(op(a, b), axis=0) on the ahead-of-time streaming kernels (the
    same stream_impl.h the specialised ones instantiate; no compile cost).  int64 sums wrap and
    are exact.  Float columns are accumulated in f64 by the kernel: allowed
    64 * 2^-53 * sum|v| for the 64 additions plus one ulp of the float64 result
    for the final rounding, against the sum in longdouble."""
    ops = STREAM_OPS[dtype][which::3]
    lazy, refs = [], []
    for op in ops:
        a, b = stream_inputs(op, dtype)
        A, B = arr(a, STREAM_CHUNKS, interp), arr(b, STREAM_CHUNKS, interp)
        with np.errstate(all="ignore"):
            if op == "where":
                lazy.append(xp.sum(xp.where(A > B, A, B), axis=0))
                v = np.where(a > b, a, b)
            elif op in ("exp", "sin"):
                lazy.append(xp.sum(getattr(xp, op)(A), axis=0))
                v = getattr(np, op)(a)
            else:
                lazy.append(xp.sum(getattr(xp, op)(A, B), axis=0))
                v = M.np_op(op, a, b)
        refs.append((op, v))
    got = cubed.compute(*lazy)
    for g, (op, v) in zip(got, refs):
        g = np.asarray(g)
        # (the array API's sum of a float32 array is float64, as the reference's)
        assert g.dtype == (np.int64 if v.dtype.kind == "i" else np.float64), op
        if v.dtype.kind == "i":
            with np.errstate(all="ignore"):
                M.assert_bit_equal(g, np.sum(v, axis=0), f"sum({op}) {dtype}")
            continue
        with np.errstate(all="ignore"):
            ref = np.sum(v.astype(np.longdouble), axis=0)
            mag = np.sum(np.abs(v).astype(np.longdouble), axis=0)
            ref_dt = ref.astype(g.dtype)
        assert np.array_equal(np.isnan(g), np.isnan(ref_dt)), op
        fin = np.isfinite(ref_dt)
        assert np.array_equal(g[~fin], ref_dt[~fin], equal_nan=True), op
        tol = 64 * 2.0 ** -53 * mag[fin] + np.spacing(np.abs(ref_dt[fin])).astype(np.longdouble)
        if op in ("exp", "sin"):  # the device routine's own error, per term
            tol = tol + (M_ULP(op, dtype) * np.finfo(dtype).eps) * mag[fin]
        err = np.abs(g[fin].astype(np.longdouble) - ref[fin])
        print(f"stream sum({op}) {dtype}: max err/tol {float(np.max(err / tol)):.3f}")
        assert np.all(err <= tol), (op, float(np.max(err / tol)))
    assert len(spy) == len(ops) and all(m & MODE_STREAM for _, m, _ in spy), "the streaming kernels must have run"
    want = {"float32": L.V_F32, "float64": L.V_F64, "int64": L.V_I64}[dtype]
    assert all(v == want and not h for v, _, h in spy)


def test_stream_sum_specialised(jit, spy):
    """One streaming reduction on the hipRTC-specialised stream kernel."""
    a, b = stream_inputs("maximum", "int64")
    got = xp.sum(xp.maximum(arr(a, STREAM_CHUNKS, jit), arr(b, STREAM_CHUNKS, jit)), axis=0).compute()
    M.assert_bit_equal(np.asarray(got), np.sum(np.maximum(a, b), axis=0), "sum(maximum) int64")
    assert spy and all(m & MODE_STREAM and h for _, m, h in spy)


def M_ULP(op, dtype):
    return ULP_BASELINE[(op, np.dtype(dtype).name)] + ULP_SLACK


# ------------------------------------------------------------------ casts
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("src", DTYPES)
def test_cast_matrix(interp, spy, src, geom):
    """astype from ``src`` to each of the 12 real dtypes (ldv / stv / st1 at
    VEC = 4 and VEC = 1), bit-exact against numpy's astype."""
    shape, chunks = GEOMS[geom]
    n = shape[0] * shape[1]
    lazy, exps = [], []
    for dst in DTYPES:
        x = M.cast_source(src, dst, n).reshape(shape)
        lazy.append(xp.astype(arr(x, chunks, interp), np.dtype(dst)))
        with np.errstate(all="ignore"):
            exps.append((f"astype({src} -> {dst}) {geom}", x.astype(dst)))
    got = cubed.compute(*lazy)
    failures = []
    for g, (what, exp) in zip(got, exps):
        try:
            M.assert_bit_equal(np.asarray(g), exp, what)
        except AssertionError as e:
            failures.append(f"{what}: {str(e)[:300]}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_cast_bf16(interp, geom):
    shape, chunks = GEOMS[geom]
    x = M.unary_inputs("abs", "float32", shape[0] * shape[1]).reshape(shape)
    bits = ir.numpy_to_bf16(x).reshape(shape)
    down, up = cubed.compute(xp.astype(arr(x, chunks, interp), xp.bfloat16),
                             xp.astype(arr(bits, chunks, interp), xp.float32))
    M.assert_bit_equal(np.asarray(down, dtype=np.float32), ir.bf16_to_numpy(bits).reshape(shape), "f32 -> bf16")
    M.assert_bit_equal(np.asarray(up), ir.bf16_to_numpy(bits).reshape(shape), "bf16 -> f32")


# ------------------------------------------------------------------ reductions
def _u64_both_sides():
    rng = np.random.default_rng(13)
    x = rng.integers(0, 2 ** 64, (45, 39), dtype=np.uint64, endpoint=False)
    x[::3] >>= np.uint64(1)  # a third below 2^63
    x[0, 0], x[44, 38], x[7, 10], x[8, 11] = 2 ** 63 + 1, 5, 2 ** 63 - 1, 2 ** 63
    return x


@pytest.mark.parametrize("fn, axis", [("max", 0), ("min", 1), ("max", None)])
def test_uint64_max_min_reduction(jit, fn, axis):
    x = _u64_both_sides()
    got = np.asarray(getattr(xp, fn)(arr(x, (7, 10), jit), axis=axis).compute())
    M.assert_bit_equal(got, np.asarray(getattr(np, fn)(x, axis=axis)), f"{fn}(u64, axis={axis})")


def test_uint64_max_min_reduction_interpreter(interp, spy):
    x = _u64_both_sides()
    X = arr(x, (7, 10), interp)
    two = arr(np.array([2 ** 63 + 1, 5], dtype=np.uint64), (2,), interp)
    cases = [(fn, axis) for fn in ("max", "min") for axis in (0, 1, None)]
    got = cubed.compute(*[getattr(xp, fn)(X, axis=axis) for fn, axis in cases], xp.max(two), xp.min(two))
    for g, (fn, axis) in zip(got, cases):
        M.assert_bit_equal(np.asarray(g), np.asarray(getattr(np, fn)(x, axis=axis)), f"{fn}(u64, axis={axis})")
    assert int(got[-2]) == 2 ** 63 + 1 and int(got[-1]) == 5
    assert spy and not any(h for _, _, h in spy)


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).nmant >= 63
    assert math.isfinite(float(np.longdouble(1) + np.finfo(np.longdouble).eps))
