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


# ------------------------------------------------------------------ reductions: kernel forms
# The geometry table of the reduction conformance tests, in one place:
# test_reduce_plan.py asserts it on a lower-only dry run, test_gpu_reductions.py
# on the launches that ran.  Per form: the array, its chunks, the reduced
# axes, and what the first reduction launch of the plan looks like -- the
# kernel-form bits of its mode for float32 / float64 / int64 inputs (which
# may stream) and for every other dtype ("narrow": the narrow and unsigned
# integers and bool), its tasks, largest kept and reduced extents, whether
# the reduced extent is split (a workspace on a launch without MODE_PARTIALS)
# and how many reduction launches the plan has in all.  Mode bits: 1 kernel B
# (reduced dims last), 4 VEC = 4, 8 streaming, 16 partials (here: lifted).
FORM_BITS = 1 | 2 | 4 | L.MODE_STREAM | L.MODE_PARTIALS


def _form(shape, chunks, axis, modes, ntasks, kept, red, split=False, rounds=1, keepdims=False, mem=None):
    return dict(shape=shape, chunks=chunks, axis=axis, modes=modes, ntasks=ntasks, kept=kept, red=red,
                split=split, rounds=rounds, keepdims=keepdims, mem=mem)


REDUCE_FORMS = {
    # kernel A, VEC = 1, a combine round behind it
    "scalar-axis0": _form((7, 13), (3, 5), 0, (0, 0), 9, 5, 3, rounds=2),
    "scalar-axis1": _form((7, 13), (3, 5), 1, (0, 0), 9, 3, 5, rounds=2),
    "scalar-all": _form((7, 13), (3, 5), None, (0, 0), 9, 1, 15, rounds=2),
    # the streaming kernel unsplit; narrow dtypes: kernel A with VEC = 4
    "vec4-unsplit": _form((24, 32), (8, 16), 0, (12, 4), 2, 16, 24),
    # a kept extent (1028) that is no multiple of a wave's 256, two rounds
    "stream-ragged": _form((70, 1028), (16, 1028), 0, (12, 4), 5, 1028, 16, rounds=2),
    # the reduced extent split across workgroups, folded by the last to arrive
    "stream-split": _form((64, 1024), (16, 1024), 0, (12, 4), 1, 1024, 64, split=True),
    "vec4-split": _form((200, 36), (50, 36), 0, (12, 4), 1, 36, 200, split=True),
    # kernel B: the reduced dim last
    "b-vec4": _form((5, 1000), (5, 1000), 1, (5, 5), 1, 5, 1000),
    "b-scalar": _form((5, 1001), (5, 1001), 1, (1, 1), 1, 5, 1001),
    "b-split": _form((3, 20000), (3, 10000), 1, (5, 5), 1, 3, 20000, split=True),
    # a full reduction lifted: the inner dim walked as a kept dim, per-element
    # partials, then the grouped fold
    "lifted": _form((64, 4096), (32, 4096), None, (28, 20), 1, 4096, 64),
    # a full reduction that does not lift (2.2 rows per chunk on average): kernel B, split
    "full-b-split": _form((70, 4100), (32, 4100), None, (5, 5), 3, 1, 131200, split=True, rounds=2),
    # 80 chunks along the reduced axis under a small allowed_mem: the merge +
    # combine rounds fold into one split pass
    "merge-rounds": _form((400, 64), (5, 64), 0, (12, 4), 1, 64, 400, split=True, mem=120_000),
    "3d-axes02": _form((9, 10, 11), (4, 5, 6), (0, 2), (0, 0), 12, 5, 24, rounds=2),
    "3d-axis1-keepdims": _form((9, 10, 11), (4, 5, 6), 1, (0, 0), 6, 24, 10, keepdims=True),
}
STREAM_CLASS = ("float32", "float64", "int64")


def form_signature(form, leaf):
    """(vtype, form bits, tasks, kept, red, split) of the first reduction
    launch of ``form`` over leaves of dtype ``leaf`` (a name of REDUCE_DTYPES)."""
    f = REDUCE_FORMS[form]
    vtype = {"float32": L.V_F32, "bfloat16": L.V_F32, "float64": L.V_F64}.get(leaf, L.V_I64)
    return (vtype, f["modes"][0 if leaf in STREAM_CLASS else 1], f["ntasks"], f["kept"], f["red"], f["split"])


def launch_signature(s):
    """The same of one recorded launch (gpu_fixtures.Seen)."""
    return (s.vtype, s.mode & FORM_BITS, s.ntasks, s.max_kept, s.max_red, s.split)


def assert_form_ran(seen, form, leaves, jit):
    """``seen`` holds the launches of len(leaves) reductions of ``form``,
    ``leaves`` naming the dtype each one reads: each reached the form's
    kernel, with the form's rounds, on the interpreter or the specialised
    kernels throughout."""
    red = [s for s in seen if s.nfields > 0]
    ran = sorted(launch_signature(s) for s in red)
    wanted = [form_signature(form, leaf) for leaf in leaves]
    for want in sorted(set(wanted)):
        assert ran.count(want) == wanted.count(want), (form, want, wanted.count(want), sorted(set(ran)))
        if want[1] & L.MODE_PARTIALS:
            assert all(s.ws > 0 for s in red if launch_signature(s) == want)
    assert len(red) == len(leaves) * REDUCE_FORMS[form]["rounds"], (form, len(red), len(leaves))
    assert seen and all(s.jit == jit for s in seen), (form, "jit", jit)


# ------------------------------------------------------------------ reductions: inputs
# Every kept element (an output column) of a reduction input tells one
# story; the stories cycle over the kept elements, and an input with fewer
# kept elements than stories comes in several variants so that each story is
# reduced at least once.  A story's special values sit in the first reduced
# row, the last, the middle or a third of the way in, by the column's turn
# and the variant, so that they meet different chunks and different splits
# on the forms with a single kept element too.
FLOAT_STORIES = ("ordinary", "one_nan", "nan_last_row", "neg_nan", "all_nan", "pos_inf", "both_inf",
                 "all_neg_zero", "mixed_zero", "all_equal", "negative", "positive", "one_neg_zero")
INT_STORIES = ("min_and_max", "all_min", "all_max", "all_zero", "single_nonzero", "wrap_sum", "prod_wrap",
               "prod_zero", "ordinary")
BOOL_STORIES = ("min_and_max", "all_zero", "all_max", "single_nonzero", "prod_zero", "ordinary")
REDUCE_DTYPES = ("bool", "int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32",
                 "float64", "bfloat16")
NEG_NAN = np.copysign(np.nan, -1.0)


def reduce_dtype(name):
    return ir.bfloat16 if name == "bfloat16" else np.dtype(name)


def stories_for(dtype):
    dt = reduce_dtype(dtype) if isinstance(dtype, str) else np.dtype(dtype)
    if dt == ir.bfloat16 or dt.kind == "f":
        return FLOAT_STORIES
    return BOOL_STORIES if dt.kind == "b" else INT_STORIES


def reduce_axes(axis, ndim):
    if axis is None:
        return tuple(range(ndim))
    if isinstance(axis, (int, np.integer)):
        return (int(axis) % ndim,)
    return tuple(sorted(int(a) % ndim for a in axis))


def reduce_counts(shape, axis):
    """(reduced count, kept count) of a reduction of ``shape`` over ``axis``."""
    red = reduce_axes(axis, len(shape))
    r = int(np.prod([shape[a] for a in red], dtype=np.int64))
    return r, int(np.prod(shape, dtype=np.int64)) // r


def reduce_variants(dtype, shape, axis):
    """How many inputs it takes for every story to own a kept element."""
    return -(-len(stories_for(dtype)) // reduce_counts(shape, axis)[1])


def prod_exponent_bound(r):
    """Ordinary factors of a product over ``r`` elements have magnitudes
    2^u, |u| <= this: the product of any subset then lies within 2^+-100,
    normal in float64 and in float32 / bfloat16."""
    return min(0.25, 100.0 / r)


def _float_column(story, kind, r, turn, rng):
    """One kept element's ``r`` reduced values, as float64."""
    spots = [0, r - 1, r // 2, r // 3]
    p, q = spots[turn % 4], spots[(turn + 1) % 4]
    if kind == "prod":
        b = prod_exponent_bound(r)
        col = np.exp2(rng.uniform(-b, b, r)) * np.where(rng.random(r) < 0.5, -1.0, 1.0)
        same = -np.exp2(b)
    else:
        col = rng.standard_normal(r) * np.exp(rng.uniform(-3, 3, r))
        same = 1.5
    if story == "one_nan":
        col[p] = np.nan
    elif story == "nan_last_row":
        col[r - 1] = np.nan
    elif story == "neg_nan":
        col[p] = NEG_NAN
    elif story == "all_nan":
        col[:] = np.nan
        col[q] = NEG_NAN
    elif story == "pos_inf":
        col[p] = np.inf
    elif story == "both_inf":
        col[p], col[q] = np.inf, -np.inf
    elif story == "all_neg_zero":
        col[:] = -0.0
    elif story == "mixed_zero":
        col = np.where(rng.random(r) < 0.5, 0.0, -0.0)
        col[p], col[q] = 0.0, -0.0
    elif story == "all_equal":
        col[:] = same
    elif story == "negative":
        col = -np.abs(col)
    elif story == "positive":
        col = np.abs(col)
    elif story == "one_neg_zero":
        col[p] = -0.0
    else:
        assert story == "ordinary", story
    return col


def _int_column(story, kind, dt, r, turn, rng):
    spots = [0, r - 1, r // 2, r // 3]
    p, q = spots[turn % 4], spots[(turn + 1) % 4]
    if dt.kind == "b":
        lo, hi, bits = 0, 1, 1
    else:
        lo, hi, bits = int(np.iinfo(dt).min), int(np.iinfo(dt).max), dt.itemsize * 8
    wide = np.uint64 if dt.kind != "i" else np.int64

    def small():
        return rng.integers(max(lo, -3) + (dt.kind == "u"), min(hi, 3), r, endpoint=True).astype(wide)

    if story == "ordinary":
        col = random_fill(dt, r, int(rng.integers(1 << 30))).astype(wide)
        if kind == "prod" and dt.kind != "b":
            col |= wide(1)  # odd factors: the wrapped product never collapses to zero
    elif story == "min_and_max":
        col = small()
        col[p], col[q] = lo, hi
    elif story in ("all_min", "all_max", "all_zero"):
        col = np.full(r, {"all_min": lo, "all_max": hi, "all_zero": 0}[story], dtype=wide)
    elif story == "single_nonzero":
        col = np.zeros(r, dtype=wide)
        # unsigned: just above the signed type's sign bit (uint64: 2^63 + 1)
        col[p] = 1 if dt.kind == "b" else -3 if dt.kind == "i" else (1 << (bits - 1)) + 1
    elif story == "wrap_sum":
        # near 2^(bits - 2) (signed) / 2^(bits - 1) (unsigned): four of them wrap
        # a sum of the dtype's own width -- int64 near 2^62, uint64 near 2^63
        base = 1 << (bits - 2 if dt.kind == "i" else bits - 1)
        col = (base - 1 + rng.integers(0, 3, r)).astype(wide)
        if dt.kind == "u":
            col[q] = base - 1 - (r % 5)  # and one below the sign bit of the signed type
    else:
        assert story in ("prod_wrap", "prod_zero"), story
        # factors of 3 and a few of 2 (2^64 divides a product of 64 of them)
        col = np.full(r, 3, dtype=wide)
        twos = min(r // 2, 5 if bits == 8 else 40)
        col[rng.permutation(r)[:twos]] = 2
        if story == "prod_zero":
            col[p] = 0
    return col.astype(dt)


def reduce_inputs(kind, dtype, shape, axis, variant=0, seed=0):
    """(x, stories): the designed input of a reduction of ``shape`` over
    ``axis`` and the story of each kept element (an object array of the
    result's shape without keepdims).  ``kind`` is "prod" for products --
    ordinary factors within prod_exponent_bound -- and "sum" for every other
    reduction.  bfloat16 inputs come as float32 values that bfloat16 holds
    exactly."""
    dt = reduce_dtype(dtype) if isinstance(dtype, str) else np.dtype(dtype)
    isfloat = dt == ir.bfloat16 or dt.kind == "f"
    host = np.dtype("f4") if dt == ir.bfloat16 else dt
    stories = stories_for(dt)
    red = reduce_axes(axis, len(shape))
    kept = tuple(a for a in range(len(shape)) if a not in red)
    r, k = reduce_counts(shape, axis)
    rng = np.random.default_rng([seed, variant, kind == "prod", REDUCE_DTYPES.index(
        "bfloat16" if dt == ir.bfloat16 else dt.name)])
    cols = np.empty((r, k), dtype=host)
    names = np.empty(k, dtype=object)
    for j in range(k):
        turn, s = divmod(j + variant * k, len(stories))
        names[j] = stories[s]
        if isfloat:
            col = _float_column(stories[s], kind, r, turn + variant + variant // 4, rng)
            if dt == ir.bfloat16:
                col = ir.bf16_to_numpy(ir.numpy_to_bf16(col.astype("f4")))
            cols[:, j] = col.astype(host)
        else:
            cols[:, j] = _int_column(stories[s], kind, dt, r, turn + variant + variant // 4, rng)
    x = cols.reshape([shape[a] for a in red + kept]).transpose(np.argsort(red + kept))
    return np.ascontiguousarray(x), names.reshape([shape[a] for a in kept])


# ------------------------------------------------------------------ reductions: references
FLOAT_REDUCTIONS = ("sum", "prod", "max", "min", "mean", "any", "all", "nansum", "nanmean")
INT_REDUCTIONS = ("sum", "prod", "max", "min", "any", "all", "nansum")
# sum / prod / nansum also run with these explicit result dtypes
EXPLICIT_DTYPES = {"float32": "float32", "int8": "int8", "int16": "int16", "uint8": "uint64", "uint32": "uint32"}


def reduce_cases(dtype):
    """[(reduction, explicit dtype or None)] a dtype takes.  nanmean, like
    mean, takes the real floating dtypes only."""
    dt = reduce_dtype(dtype)
    if dt.kind == "b":
        return [("any", None), ("all", None)]
    fns = FLOAT_REDUCTIONS if dt == ir.bfloat16 or dt.kind == "f" else INT_REDUCTIONS
    out = [(fn, None) for fn in fns]
    if dtype in EXPLICIT_DTYPES:
        out += [(fn, EXPLICIT_DTYPES[dtype]) for fn in ("sum", "prod", "nansum")]
    return out


def reduce_result_dtype(fn, in_dtype, dtype=None):
    """The array API's result dtype (array_api/statistical_functions.py)."""
    dt = np.dtype(in_dtype)
    if fn in ("any", "all"):
        return np.dtype(bool)
    if fn in ("sum", "prod", "nansum"):
        if dtype is not None:
            return np.dtype(dtype)
        if dt.kind in "iu":
            return np.dtype("i8" if dt.kind == "i" else "u8")
        return np.dtype("f8") if dt == np.dtype("f4") else dt
    return dt


def spacing_in(v, dtype):
    """np.spacing(|v|) in ``dtype`` (bfloat16: 2^16 float32 spacings at the
    value cut to bfloat16's bits), as longdouble."""
    v = np.abs(np.asarray(v))
    with np.errstate(all="ignore"):
        if np.dtype(dtype) == ir.bfloat16:
            cut = (v.astype("f4").view(np.uint32) & np.uint32(0xFFFF0000)).view("f4")
            return np.spacing(cut).astype(np.longdouble) * 65536
        return np.spacing(v.astype(dtype)).astype(np.longdouble)


def _round_to(ref, dtype):
    """A longdouble reference rounded to ``dtype``, bfloat16 as float32 values."""
    with np.errstate(all="ignore"):
        if np.dtype(dtype) == ir.bfloat16:
            return ir.bf16_to_numpy(ir.numpy_to_bf16(ref.astype("f4"))).reshape(ref.shape)
        return ref.astype(dtype)


def float_reduce_bounds(fn, x, axis, out_dtype, keepdims=False):
    """(ref, tol, finite) of a float sum / nansum / prod / mean / nanmean of
    host values ``x``: the longdouble reference, the allowed error where the
    reference rounded to the result dtype is finite, and that mask.

    The kernels accumulate float sums in float64 in an order of their own and
    round once to the result dtype: n additions lose at most n * 2^-53 *
    sum|v|, the rounding one spacing of the result.  A mean divides that by
    the count and may lose two spacings (the division, the final rounding).
    A product of n factors loses at most n * 2^-53 * |prod| and one spacing.
    Asserted here on the way: sum|v| < max / 2 of the result dtype, so no order
    of the additions overflows; every subset of a product's finite factors
    stays normal in float64 and the product normal in the result dtype."""
    n = reduce_counts(x.shape, axis)[0]
    kw = dict(axis=axis, keepdims=keepdims)
    X = x.astype(np.longdouble)
    host = np.dtype("f4") if np.dtype(out_dtype) == ir.bfloat16 else np.dtype(out_dtype)
    fi = np.finfo(host)
    u = np.longdouble(2.0) ** -53
    with np.errstate(all="ignore"):
        nan = np.isnan(X)
        if fn == "prod":
            ref = np.prod(X, **kw)
            ok = np.isfinite(X) & (X != 0)
            log = np.sum(np.abs(np.log2(np.abs(np.where(ok, X, 1)))), **kw)
            assert np.all(log < 1000), "a subset of the factors could leave float64's normal range"
            whole = np.isfinite(ref) & (ref != 0)
            assert np.all((np.abs(ref[whole]) >= fi.tiny) & (np.abs(ref[whole]) <= fi.max / 2)), \
                "a product is not normal in the result dtype"
            finite = np.isfinite(_round_to(ref, out_dtype))
            tol = n * u * np.abs(ref) + spacing_in(_round_to(ref, out_dtype), out_dtype)
            return ref, tol, finite
        skip = nan if fn in ("nansum", "nanmean") else np.zeros_like(nan)
        ref = np.sum(np.where(skip, 0, X), **kw)
        mag = np.sum(np.where(np.isfinite(X), np.abs(X), 0), **kw)
        assert np.all(mag < np.longdouble(fi.max) / 2), "the additions could overflow in some order"
        scale = np.longdouble(1)
        if fn in ("mean", "nanmean"):
            count = np.sum(~skip, **kw).astype(np.longdouble)
            ref = ref / count  # an all-NaN nanmean: 0 / 0
            scale = np.where(count > 0, count, 1)
        finite = np.isfinite(_round_to(ref, out_dtype))
        sp = spacing_in(np.where(finite, _round_to(ref, out_dtype), 0), out_dtype)
        tol = n * u * mag / scale + (2 if fn in ("mean", "nanmean") else 1) * sp
    return ref, tol, finite


def check_reduction(fn, x, got, axis, in_dtype, dtype=None, keepdims=False, stories=None, what=""):
    """``got`` (compute()'s numpy result) against the reference of reduction
    ``fn`` over ``axis`` of host values ``x`` of dtype ``in_dtype``
    (bfloat16: ``x`` and ``got`` are its values widened to float32).

    Integer and bool results (any / all included) are bit-exact against
    numpy with the same ``dtype=``: sums and products wrap.  Float max / min:
    NaN in the same places whatever its sign, else equal values.  Float sum /
    nansum / prod / mean / nanmean: float_reduce_bounds; NaN and +-inf equal
    in place and sign.  Two signs of zero are not compared: that of a zero
    max / min (numpy's own differs between its scalar and SIMD loops) and that
    of a zero sum -- the kernels' identity is -0.0, so their sum of -0.0s is
    -0.0, where numpy's own answer has differed between versions (numpy
    2.2.6 gives +0.0 for np.sum(np.full(n, -0.0)) at every n).  Nothing else
    is masked; a
    failure names the stories of the kept elements that differ."""
    in_dtype = np.dtype(in_dtype)
    got = np.asarray(got)
    out_dtype = reduce_result_dtype(fn, in_dtype, dtype)
    host = np.dtype("f4") if out_dtype == ir.bfloat16 else out_dtype
    shape = np.empty(x.shape, dtype=bool).sum(axis=axis, keepdims=keepdims).shape
    assert got.dtype == host, (what, "dtype", got.dtype, host)
    assert got.shape == shape, (what, "shape", got.shape, shape)
    kw = dict(axis=axis, keepdims=keepdims)
    isfloat = in_dtype == ir.bfloat16 or in_dtype.kind == "f"
    with np.errstate(all="ignore"):
        if fn in ("any", "all") or not isfloat:
            npfn = getattr(np, fn)
            exp = npfn(x, **kw) if fn in ("any", "all", "max", "min") else npfn(x, dtype=out_dtype, **kw)
            exp = np.asarray(exp)
            assert exp.dtype == out_dtype, (what, exp.dtype)
            bad = got != exp
        elif fn in ("max", "min"):
            exp = np.asarray(getattr(np, fn)(x, **kw))
            bad = ~((got == exp) | (np.isnan(got) & np.isnan(exp)))
        else:
            ref, tol, finite = float_reduce_bounds(fn, x, axis, out_dtype, keepdims)
            exp = _round_to(ref, out_dtype)
            g = got.astype(np.longdouble)
            bad = np.where(finite, ~(np.abs(g - ref) <= tol),
                           ~((got == exp) | (np.isnan(got) & np.isnan(exp))))
            if fn == "prod":  # a zero product's sign is that of its factors'
                bad |= (exp == 0) & ((got != 0) | (np.signbit(got) != np.signbit(exp)))
    if np.any(bad):
        where = np.argwhere(bad)
        told = sorted(set(np.asarray(stories).reshape(shape)[bad])) if stories is not None else "?"
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ, stories {told}; first at "
                             f"{where[0].tolist()}: got {got[bad][:3]!r}, expected {np.asarray(exp)[bad][:3]!r}")
