"""A host model of the per-element VM (cubed_amd/csrc/vm.h) and the shared
inputs / numpy references of the elementwise conformance tests.

``run_code`` interprets a ``lowering.Codegen`` instruction list with numpy:
registers are arrays of the program's register type (float32, float64 or
int64), every opcode does what ``unary()`` / ``binary()`` / ``cast_val`` do
there, leaves are loaded as ``ld1`` and results stored as ``st1`` would.  An
opcode the model does not know -- or one vm.h has no case for in that register
type, such as a shift in float registers -- raises ``UnknownOpcode``.

``model_eval`` lowers an expression program exactly as
``lowering.program_fits`` does and, where the program does not fit one fused
launch, splits it as the executor would (``split.split_program``: parts are
stored at their node dtype and read back as leaves).

``np_eval`` is the reference: numpy evaluating the expression tree directly,
with the casts at every node.  Not a conftest; plain helpers."""
import numpy as np

from cubed_amd import ir
from cubed_amd import lowering as L

VTYPE_DTYPE = {L.V_F32: np.dtype("f4"), L.V_F64: np.dtype("f8"), L.V_I64: np.dtype("i8")}
UNARY_BY_CODE = {v: k for k, v in ir.UNARY_OPS.items() if v is not None}
BINARY_BY_CODE = {v: k for k, v in ir.BINARY_OPS.items()}
# include/cubed_amd.h CUBED_OP_UFLOORDIV .. CUBED_OP_USHR
UNSIGNED_BY_CODE = {94: "floor_divide", 95: "remainder", 96: "maximum", 97: "minimum", 98: "less",
                    99: "less_equal", 100: "greater", 101: "greater_equal", 102: "bitwise_right_shift"}
I64_MIN = np.iinfo(np.int64).min
TWO63 = 9223372036854775808.0


class UnknownOpcode(Exception):
    pass


# ------------------------------------------------------------------ scalar I/O
def f2i64(x):
    """common.h f2i64: truncate; NaN / out of range give INT64_MIN."""
    x = np.asarray(x, dtype=np.float64)
    ok = (x >= -TWO63) & (x < TWO63)
    return np.where(ok, np.trunc(np.where(ok, x, 0)).astype(np.int64), I64_MIN)


def to_u64bits(x):
    x = np.asarray(x, dtype=np.float64)
    big = x >= TWO63
    hi = np.where(big, x, TWO63).astype(np.uint64).view(np.int64)
    return np.where(big, hi, f2i64(np.where(big, 0, x)))


def _wrap(i, dt):
    """int64 values -> integer dtype dt, wrapping (a C conversion)."""
    return np.asarray(i, dtype=np.int64).astype(dt)


def load(a, V):
    """ld1: one element of a's dtype converted to V."""
    a = np.asarray(a)
    if a.dtype == ir.bfloat16:
        a = ir.bf16_to_numpy(a)
    if V.kind == "i" and a.dtype.kind == "f":
        return f2i64(a)  # never generated: float leaves make a float program
    return a.astype(V)


def store(v, dt):
    """st1: V converted to dtype dt."""
    dt = np.dtype(dt)
    if dt == ir.bfloat16:
        return ir.numpy_to_bf16(v.astype(np.float32))
    if dt.kind == "b":
        return v != 0
    if dt.kind == "f":
        return v.astype(dt)
    if v.dtype.kind == "i":
        return _wrap(v, dt)
    if dt == np.uint64:
        return to_u64bits(v).view(np.uint64)
    return _wrap(f2i64(v), dt)


def cast_val(x, t, V):
    """vm.h cast_val: round the register value to dtype t, keeping it in V."""
    t = np.dtype(t)
    if t.kind == "b":
        return (x != 0).astype(V)
    if V.kind == "i":
        return x if t.itemsize == 8 else _wrap(x, t).astype(V)
    if t == ir.bfloat16:
        return ir.bf16_to_numpy(ir.numpy_to_bf16(x.astype(np.float32))).astype(V)
    if t.kind == "f":
        return x.astype(t).astype(V)
    if t == np.uint64:
        return to_u64bits(x).view(np.uint64).astype(V)
    return _wrap(f2i64(x), t).astype(V)


# ------------------------------------------------------------------ ops
def _u(x):
    return x.view(np.uint64)


def _ipow(b, e):
    r = np.ones_like(b, dtype=np.uint64)
    x = _u(b).copy()
    ee = e.copy()
    for _ in range(63):
        r = np.where((ee & 1) != 0, r * x, r)
        x = x * x
        ee = ee >> 1
    return np.where(e < 0, 0, r.view(np.int64))


def _ifloordiv(a, b):
    safe = np.where((b == 0) | (b == -1), 1, b)
    q = np.floor_divide(a, safe)
    q = np.where(b == -1, (np.uint64(0) - _u(a)).view(np.int64), q)
    return np.where(b == 0, 0, q)


def _imod(a, b):
    safe = np.where((b == 0) | (b == -1), 1, b)
    return np.where((b == 0) | (b == -1), 0, np.remainder(a, safe))


def _bool(x):
    return x != 0


INT_UNARY = {
    "negative": lambda x: (np.uint64(0) - _u(x)).view(np.int64),
    "abs": lambda x: np.where(x < 0, (np.uint64(0) - _u(x)).view(np.int64), x),
    "logical_not": lambda x: (x == 0).astype(np.int64),
    "bitwise_invert": lambda x: ~x,
    "sign": lambda x: (x > 0).astype(np.int64) - (x < 0).astype(np.int64),
    "square": lambda x: (_u(x) * _u(x)).view(np.int64),
    "isnan": lambda x: np.zeros_like(x),
    "isinf": lambda x: np.zeros_like(x),
    "signbit": lambda x: (x < 0).astype(np.int64),
    "isfinite": lambda x: np.ones_like(x),
}
# vm.h `default: break` in int64 registers: identities of integers
INT_IDENTITY = {"floor", "ceil", "trunc", "round"}

FLOAT_UNARY = {
    "negative": np.negative, "abs": np.abs, "sqrt": np.sqrt, "exp": np.exp, "log": np.log, "sin": np.sin,
    "cos": np.cos, "tan": np.tan, "tanh": np.tanh, "floor": np.floor, "ceil": np.ceil, "trunc": np.trunc,
    "round": np.rint, "isnan": np.isnan, "isinf": np.isinf, "isfinite": np.isfinite,
    "logical_not": lambda x: x == 0, "bitwise_invert": lambda x: ~f2i64(x), "sign": np.sign,
    "square": np.square, "reciprocal": lambda x: x.dtype.type(1) / x, "log1p": np.log1p, "expm1": np.expm1,
    "log2": np.log2, "log10": np.log10, "sinh": np.sinh, "cosh": np.cosh, "asin": np.arcsin, "acos": np.arccos,
    "atan": np.arctan, "asinh": np.arcsinh, "acosh": np.arccosh, "atanh": np.arctanh, "exp2": np.exp2,
    "signbit": np.signbit,
}

INT_BINARY = {
    "add": lambda x, y: (_u(x) + _u(y)).view(np.int64),
    "subtract": lambda x, y: (_u(x) - _u(y)).view(np.int64),
    "multiply": lambda x, y: (_u(x) * _u(y)).view(np.int64),
    "floor_divide": _ifloordiv, "remainder": _imod, "pow": _ipow,
    "maximum": np.maximum, "minimum": np.minimum, "fmax": np.maximum, "fmin": np.minimum,
    "equal": np.equal, "not_equal": np.not_equal, "less": np.less, "less_equal": np.less_equal,
    "greater": np.greater, "greater_equal": np.greater_equal,
    "logical_and": lambda x, y: _bool(x) & _bool(y), "logical_or": lambda x, y: _bool(x) | _bool(y),
    "logical_xor": lambda x, y: _bool(x) ^ _bool(y),
    "bitwise_and": np.bitwise_and, "bitwise_or": np.bitwise_or, "bitwise_xor": np.bitwise_xor,
    "bitwise_left_shift": lambda x, y: np.where((y < 0) | (y > 63), 0,
                                                (_u(x) << _u(np.clip(y, 0, 63))).view(np.int64)),
    "bitwise_right_shift": lambda x, y: np.where((y < 0) | (y > 63), np.where(x < 0, -1, 0),
                                                 x >> np.clip(y, 0, 63)),
}
UINT_BINARY = {
    "floor_divide": lambda x, y: np.where(y == 0, 0, (_u(x) // np.where(y == 0, 1, _u(y))).view(np.int64)),
    "remainder": lambda x, y: np.where(y == 0, 0, (_u(x) % np.where(y == 0, 1, _u(y))).view(np.int64)),
    "maximum": lambda x, y: np.maximum(_u(x), _u(y)).view(np.int64),
    "minimum": lambda x, y: np.minimum(_u(x), _u(y)).view(np.int64),
    "less": lambda x, y: _u(x) < _u(y), "less_equal": lambda x, y: _u(x) <= _u(y),
    "greater": lambda x, y: _u(x) > _u(y), "greater_equal": lambda x, y: _u(x) >= _u(y),
    "bitwise_right_shift": lambda x, y: np.where(_u(y) > 63, 0, (_u(x) >> np.minimum(_u(y), 63)).view(np.int64)),
}
# (no shifts: vm.h has no float case for them)
FLOAT_BINARY = {
    "add": np.add, "subtract": np.subtract, "multiply": np.multiply, "divide": np.divide,
    "floor_divide": np.floor_divide, "remainder": np.remainder, "pow": np.power,
    "maximum": np.maximum, "minimum": np.minimum, "fmax": np.fmax, "fmin": np.fmin,
    "equal": np.equal, "not_equal": np.not_equal, "less": np.less, "less_equal": np.less_equal,
    "greater": np.greater, "greater_equal": np.greater_equal,
    "logical_and": lambda x, y: _bool(x) & _bool(y), "logical_or": lambda x, y: _bool(x) | _bool(y),
    "logical_xor": lambda x, y: _bool(x) ^ _bool(y),
    "bitwise_and": lambda x, y: f2i64(x) & f2i64(y), "bitwise_or": lambda x, y: f2i64(x) | f2i64(y),
    "bitwise_xor": lambda x, y: f2i64(x) ^ f2i64(y),
    "atan2": np.arctan2, "hypot": np.hypot, "copysign": np.copysign, "logaddexp": np.logaddexp,
    "logaddexp2": np.logaddexp2,
}


def run_code(code, consts, vtype, regs):
    """vm.h run_vm over ``regs`` (register index -> array of the V dtype)."""
    V = VTYPE_DTYPE[vtype]
    isint = V.kind == "i"
    n = len(next(iter(regs.values())))
    with np.errstate(all="ignore"):
        for op, a, b, c, t, imm in code:
            if op == L._OPCODES["CONST"]:
                kind, v = consts[imm]
                assert kind == ("i" if isint else "f")
                regs[a] = np.full(n, v, dtype=np.int64 if isint else np.float64).astype(V)
            elif op == L._OPCODES["MOV"]:
                regs[a] = regs[b].copy()
            elif op == L._OPCODES["CAST"]:
                regs[a] = cast_val(regs[a], ir.CODE_DTYPES[t], V)
            elif op == L._OPCODES["WHERE"]:
                regs[a] = np.where(regs[c] != 0, regs[a], regs[b])
            elif op in UNARY_BY_CODE:
                name = UNARY_BY_CODE[op]
                table = INT_UNARY if isint else FLOAT_UNARY
                if name in table:
                    regs[a] = np.asarray(table[name](regs[a])).astype(V)
                elif not (isint and name in INT_IDENTITY):
                    raise UnknownOpcode(f"unary {name} ({op}) in {V} registers")
            elif op in BINARY_BY_CODE or op in UNSIGNED_BY_CODE:
                if op in UNSIGNED_BY_CODE:
                    name, table = UNSIGNED_BY_CODE[op], (UINT_BINARY if isint else {})
                else:
                    name, table = BINARY_BY_CODE[op], (INT_BINARY if isint else FLOAT_BINARY)
                if name not in table:
                    raise UnknownOpcode(f"binary {name} ({op}) in {V} registers")
                regs[a] = np.asarray(table[name](regs[a], regs[b])).astype(V)
            else:
                raise UnknownOpcode(f"opcode {op}")
            assert regs[a].dtype == V
    return regs


# ------------------------------------------------------------------ programs
def lower(p):
    """(vtype, Codegen, leaves, output register) of a map program, lowered as
    lowering.program_fits / lower_expr_pipeline do."""
    outs, _ = L.program_exprs(p)
    pre = L.dedupe_leaves(outs)
    leaves = L.collect_leaves(pre)
    by_key = {L._leaf_key(l): i for i, l in enumerate(leaves)}
    leaf_regs = {}
    for e in pre:
        for lf in ir.leaves(e):
            if not isinstance(lf, (ir.Const, ir.Field)):
                leaf_regs[id(lf)] = by_key[L._leaf_key(lf)]
    vtype = L.choose_vtype(pre, leaves)
    cg = L.Codegen(vtype, leaf_regs)
    cg.count_uses(pre)
    r, _ = cg.gen(pre[0])
    return vtype, cg, leaves, r, pre[0]


def run_one(p, arrays):
    vtype, cg, leaves, r, e = lower(p)
    V = VTYPE_DTYPE[vtype]
    regs = {i: load(arrays[lf.index], V) for i, lf in enumerate(leaves)}
    n = len(arrays[0])
    for i in range(len(leaves), 6):
        regs[i] = np.zeros(n, dtype=V)
    run_code(cg.code, cg.consts, vtype, regs)
    return store(regs[r], e.dtype)


def model_eval(p, arrays):
    """What the kernels compute for map program ``p`` over 1-d ``arrays``:
    one fused launch where the program fits, else the executor's split."""
    if L.program_fits(p):
        return run_one(p, arrays), [lower(p)[0]]
    from cubed_amd.split import split_program

    parts, rest = split_program(p)
    arrays = list(arrays)
    vtypes = []
    for sub, dt in parts:
        assert L.program_fits(sub)
        vtypes.append(lower(sub)[0])
        arrays.append(run_one(sub, arrays))
        assert arrays[-1].dtype == np.dtype(dt)
    vtypes.append(lower(rest)[0])
    return run_one(rest, arrays), vtypes


NP_NAMES = {"pow": "power", "bitwise_invert": "invert", "asin": "arcsin", "acos": "arccos", "atan": "arctan",
            "asinh": "arcsinh", "acosh": "arccosh", "atanh": "arctanh", "atan2": "arctan2",
            "bitwise_left_shift": "left_shift", "bitwise_right_shift": "right_shift", "abs": "absolute"}


def np_op(op, *xs):
    """numpy's own result of elementwise ``op`` (array-API name)."""
    if op in ("floor", "ceil", "trunc", "round", "positive") and xs[0].dtype.kind in "iub":
        return xs[0].copy()
    return getattr(np, NP_NAMES.get(op, op))(*xs)


def np_eval(e, arrays):
    """numpy evaluating the expression tree, with the casts at every node."""
    with np.errstate(all="ignore"):
        if isinstance(e, ir.Arg):
            return arrays[e.index]
        if isinstance(e, ir.Const):
            return np.array(e.value).astype(e.dtype)
        if isinstance(e, ir.Cast):
            return np_eval(e.x, arrays).astype(e.dtype)
        if isinstance(e, ir.Where):
            r = np.where(np_eval(e.c, arrays), np_eval(e.a, arrays), np_eval(e.b, arrays))
        else:
            r = np_op(e.op, *[np_eval(c, arrays) for c in e.children()])
        assert r.dtype == np.dtype(e.dtype), (e, r.dtype)
        return r


# ------------------------------------------------------------------ the op table
# array-API function -> the dtype kinds it accepts ("b" bool, "i" signed,
# "u" unsigned, "f" real floating), as array_api/elementwise_functions.py
_F, _N, _I, _IB, _ALL = "f", "iuf", "iu", "biu", "biuf"
UNARY_API = {
    "abs": _N, "negative": _N, "positive": _N, "sign": _N, "square": _N, "round": _N,
    "floor": _N, "ceil": _N, "trunc": _N, "isfinite": _N, "isinf": _N, "isnan": _N,
    "bitwise_invert": _IB, "logical_not": "b",
    "sqrt": _F, "exp": _F, "expm1": _F, "log": _F, "log1p": _F, "log2": _F, "log10": _F, "sin": _F, "cos": _F,
    "tan": _F, "sinh": _F, "cosh": _F, "tanh": _F, "asin": _F, "acos": _F, "atan": _F, "asinh": _F,
    "acosh": _F, "atanh": _F,
}
BINARY_API = {
    "add": _N, "subtract": _N, "multiply": _N, "pow": _N, "floor_divide": _N, "remainder": _N,
    "maximum": _N, "minimum": _N, "divide": _F,
    "equal": _ALL, "not_equal": _ALL, "less": _ALL, "less_equal": _ALL, "greater": _ALL, "greater_equal": _ALL,
    "logical_and": "b", "logical_or": "b", "logical_xor": "b",
    "bitwise_and": _IB, "bitwise_or": _IB, "bitwise_xor": _IB,
    "bitwise_left_shift": _I, "bitwise_right_shift": _I,
    "atan2": _F, "hypot": _F, "logaddexp": _F, "copysign": _F,
}
# ops of ir.UNARY_OPS / ir.BINARY_OPS that have no array-API function here
# (reached through numpy ufuncs in map_blocks): float operands
UNARY_EXTRA = {"signbit": _F, "reciprocal": _F, "exp2": _F}
BINARY_EXTRA = {"fmax": _F, "fmin": _F, "logaddexp2": _F}
BOOL_RESULT = ir.COMPARISONS | ir.UNARY_BOOL_RESULT

# results compared within a bound in ulps; everything else is bit-exact
ULP_OPS = {"exp", "expm1", "log", "log1p", "log2", "log10", "sin", "cos", "tan", "sinh", "cosh", "tanh", "asin",
           "acos", "atan", "asinh", "acosh", "atanh", "exp2", "pow", "atan2", "hypot", "logaddexp", "logaddexp2"}
# value-equal, the sign of a zero result not asserted
ZERO_SIGN_FREE = {"maximum", "minimum", "fmax", "fmin"}

REAL_DTYPES = [np.dtype(d) for d in ("bool", "i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8", "f2", "f4", "f8")]


def ops_for(dtype, extra=True):
    k = np.dtype(dtype).kind
    un = dict(UNARY_API, **(UNARY_EXTRA if extra else {}))
    bi = dict(BINARY_API, **(BINARY_EXTRA if extra else {}))
    return [o for o, c in un.items() if k in c], [o for o, c in bi.items() if k in c]


def result_dtype(op, dtype):
    return np.dtype(bool) if op in BOOL_RESULT else np.dtype(dtype)


def is_ulp(op, dtype):
    return op in ULP_OPS and np.dtype(dtype).kind == "f"


# ------------------------------------------------------------------ inputs
def edge_vector(dtype):
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return np.array([False, True])
    if dt.kind == "f":
        fi = np.finfo(dt)
        big = {2: 1e4, 4: 1e6, 8: 1e15}[dt.itemsize]
        v = [0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny, -fi.tiny, 1.0, -1.0, 0.5, 1.5,
             2.5, -2.5, fi.max, -fi.max, np.inf, -np.inf, np.nan, big, -big * 0.37, 3.0, -7.25, 0.1]
        return np.array(v, dtype=dt)
    ii = np.iinfo(dt)
    v = [ii.min, ii.min + 1, 0, 1, 2, 3, ii.max - 1, ii.max]
    if dt.kind == "i":
        v += [-1, -2, -3]
    else:
        h = 1 << (dt.itemsize * 8 - 1)  # around the sign bit of the signed type
        v += [h - 1, h, h + 1]
    if dt.itemsize == 8:
        v += [(1 << 53) + 1, (1 << 53) + 3, (1 << 62) + 5]
        if dt.kind == "i":
            v += [-(1 << 53) - 1]
    return np.array(sorted(set(v)), dtype=dt)


def random_fill(dtype, n, seed):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dt.kind == "b":
        return rng.random(n) < 0.5
    if dt.kind == "f":
        x = rng.standard_normal(n) * np.exp(rng.uniform(-3, 3, n))
        return x.astype(dt)
    ii = np.iinfo(dt)
    wide = rng.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)
    small = rng.integers(max(ii.min, -20), min(ii.max, 20), n, dtype=dt, endpoint=True)
    return np.where(rng.random(n) < 0.5, wide, small).astype(dt)


def _second_operand(op, dtype):
    """The second operand's edge vector: shift counts 0 .. width + 1 and
    non-negative integer exponents up to ones that overflow (negative counts
    and exponents are left out by construction)."""
    dt = np.dtype(dtype)
    if dt.kind in "iu" and op in ("bitwise_left_shift", "bitwise_right_shift"):
        return np.arange(0, dt.itemsize * 8 + 2).astype(dt)
    if dt.kind in "iu" and op == "pow":
        return np.array([e for e in (0, 1, 2, 3, 5, 7, 13, 31, 63, 65) if e <= np.iinfo(dt).max], dtype=dt)
    return edge_vector(dt)


def unary_inputs(op, dtype, n, seed=0):
    ev = edge_vector(dtype)
    x = np.concatenate([ev, random_fill(dtype, max(n - len(ev), 0), seed)])
    return x[:n] if len(x) > n else np.resize(x, n)


def binary_inputs(op, dtype, n, seed=0):
    """The Cartesian product of the edge vectors, then seeded random fill; a
    shape smaller than the product takes a seeded sample of it."""
    a0, b0 = edge_vector(dtype), _second_operand(op, dtype)
    A, B = [m.ravel() for m in np.meshgrid(a0, b0, indexing="ij")]
    rng = np.random.default_rng(seed + 1)
    if len(A) > n:
        pick = rng.permutation(len(A))[:n]
        return A[pick], B[pick]
    fa = random_fill(dtype, n - len(A), seed + 2)
    fb = b0[rng.integers(0, len(b0), n - len(A))] if len(b0) != len(a0) or np.dtype(dtype).kind != "f" \
        else random_fill(dtype, n - len(A), seed + 3)
    if np.dtype(dtype).kind in "iu" and op not in ("bitwise_left_shift", "bitwise_right_shift", "pow"):
        fb = np.where(rng.random(n - len(A)) < 0.5, fb, random_fill(dtype, n - len(A), seed + 3))
    return np.concatenate([A, fa]), np.concatenate([B, fb.astype(dtype)])


# ------------------------------------------------------------------ comparison
def assert_bit_equal(got, exp, what=""):
    assert got.dtype == exp.dtype, (what, got.dtype, exp.dtype)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if exp.dtype.kind == "f":
        nan = np.isnan(exp)
        assert np.array_equal(np.isnan(got), nan), (what, "NaN positions")
        u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[exp.dtype.itemsize]
        bad = (got.view(u) != exp.view(u)) & ~nan
    else:
        bad = got != exp
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(), got[bad][:3], exp[bad][:3])


def assert_value_equal(got, exp, what=""):
    """Equal values, NaN in the same places; the sign of zero not compared."""
    assert got.dtype == exp.dtype, (what, got.dtype, exp.dtype)
    assert np.array_equal(got, exp, equal_nan=exp.dtype.kind == "f"), what


def ulp_error(got, ref, dtype):
    """|got - ref| in ulps of ``dtype`` at ref (ref in higher precision);
    positions where ref is NaN / inf / rounds to inf must match exactly."""
    dt = np.dtype(dtype)
    with np.errstate(all="ignore"):
        ref_dt = ref.astype(dt)
        special = ~np.isfinite(ref_dt)
        assert np.array_equal(np.isnan(got), np.isnan(ref_dt)), "NaN positions"
        assert np.array_equal(got[special & ~np.isnan(ref_dt)], ref_dt[special & ~np.isnan(ref_dt)]), "inf positions"
        ok = ~special & np.isfinite(got)
        err = np.zeros(got.shape, dtype=np.float64)
        err[~special & ~np.isfinite(got)] = np.inf  # overflowed where the reference is finite
        spacing = np.spacing(np.maximum(np.abs(ref_dt[ok]), np.finfo(dt).tiny)).astype(ref.dtype)
        err[ok] = np.abs((got[ok].astype(ref.dtype) - ref[ok]) / spacing).astype(np.float64)
    return err


# ------------------------------------------------------------------ casts
def cast_source(src, dst, n):
    """n values of dtype src whose cast to dst numpy defines: float -> int
    sources lie inside dst's range (negative fractions and, for uint64, f64
    values in [2^63, 2^64) included)."""
    src, dst = np.dtype(src), np.dtype(dst)
    if not (src.kind == "f" and dst.kind in "iu"):
        return unary_inputs("abs", src, n)
    ii = np.iinfo(dst)
    edge = [ii.min, ii.min + 1, -3, -2, -1, 0, 1, 2, 3, ii.max - 1, ii.max, ii.max // 2, 2 ** 63, 2 ** 63 + 2048,
            2 ** 64 - 2048, 2 ** 53 + 2]
    frac = [-2.5, -1.5, -0.75, -0.5, -0.0, 0.5, 0.75, 1.5, 2.5, 126.5, 254.9, 32766.5, 65534.5]
    rng = np.random.default_rng(5)
    with np.errstate(all="ignore"):
        rnd = rng.uniform(max(float(ii.min), -1e18), min(float(ii.max), 1e19), 4 * n)
        v = np.concatenate([np.array(edge, dtype="f8"), np.array(frac), rnd, rng.uniform(-200, 200, n)]).astype(src)
        t = np.trunc(v.astype(np.longdouble))
    v = v[np.isfinite(v) & (t >= ii.min) & (t <= ii.max)]
    return np.resize(v, n)
