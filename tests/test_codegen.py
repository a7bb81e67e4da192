"""The fused-program code generator (lowering.Codegen) against a direct
numpy evaluation: random expression DAGs over 3 leaves (shared
subexpressions, WHERE, one or two outputs) are compiled to two-address VM
code, the code is interpreted on the host with numpy ops in place of the
kernels' register ops, and every output register must hold the expression's
value.  Guards the register handover (a leaf or common subexpression at its
last use is computed in place) against clobbering an operand that is still
pending or an output already produced.  CPU only; no kernel runs."""
import random

import numpy as np

from cubed_amd import ir
from cubed_amd.lowering import _OPCODES, V_F64, Codegen, LoweringError

UNARY_BY_CODE = {v: k for k, v in ir.UNARY_OPS.items() if v is not None}
BINARY_BY_CODE = {v: k for k, v in ir.BINARY_OPS.items()}
NP_UNARY = {"negative": np.negative, "abs": np.abs, "exp": np.exp}
NP_BINARY = {"add": np.add, "subtract": np.subtract, "multiply": np.multiply,
             "maximum": np.maximum, "less": np.less}
F8 = np.dtype("f8")


def rand_expr(leaves, depth, rng):
    """A random expression DAG (leaves are shared objects: CSE and reuse)."""
    if depth == 0 or rng.random() < 0.25:
        return rng.choice(leaves)
    k = rng.random()
    if k < 0.25:
        return ir.Unary(rng.choice(list(NP_UNARY)), rand_expr(leaves, depth - 1, rng), F8)
    if k < 0.8:
        op = rng.choice(["add", "subtract", "multiply", "maximum"])
        return ir.Binary(op, rand_expr(leaves, depth - 1, rng), rand_expr(leaves, depth - 1, rng), F8)
    c = ir.Binary("less", rand_expr(leaves, depth - 1, rng), rand_expr(leaves, depth - 1, rng),
                  np.dtype("bool"))
    return ir.Where(c, rand_expr(leaves, depth - 1, rng), rand_expr(leaves, depth - 1, rng), F8)


def evaluate(e, vals):
    if isinstance(e, ir.Arg):
        return vals[e.index]
    if isinstance(e, ir.Unary):
        return NP_UNARY[e.op](evaluate(e.x, vals))
    if isinstance(e, ir.Binary):
        return NP_BINARY[e.op](evaluate(e.a, vals), evaluate(e.b, vals)).astype(float)
    return np.where(evaluate(e.c, vals) != 0, evaluate(e.a, vals), evaluate(e.b, vals))


def run(code, regs):
    """Interpret two-address VM code (vm.h run_vm) with numpy ops."""
    for op, a, b, c, _t, _imm in code:
        if op == _OPCODES["MOV"]:
            regs[a] = regs[b].copy()
        elif op == _OPCODES["WHERE"]:
            regs[a] = np.where(regs[c] != 0, regs[a], regs[b])
        elif op == _OPCODES["CAST"]:
            pass  # f64 values in f64 registers
        elif op in BINARY_BY_CODE:
            regs[a] = NP_BINARY[BINARY_BY_CODE[op]](regs[a], regs[b]).astype(float)
        else:
            regs[a] = NP_UNARY[UNARY_BY_CODE[op]](regs[a])


def test_codegen_matches_numpy_on_random_programs():
    rng = random.Random(5)
    tried = 0
    with np.errstate(all="ignore"):
        for trial in range(1500):
            leaves = [ir.Arg(i, np.dtype("f8"), (0,)) for i in range(3)]
            outs = [rand_expr(leaves, 4, rng) for _ in range(rng.choice([1, 2]))]
            lr = {}
            for e in outs:
                for lf in ir.leaves(e):
                    lr[id(lf)] = lf.index
            cg = Codegen(V_F64, lr)
            cg.count_uses(outs)
            try:
                regs_out = []
                for e in outs:
                    r, _ = cg.gen(e)
                    cg.pin(r)
                    regs_out.append(r)
            except LoweringError:
                continue  # needs more than the VM's registers: split.py's case
            tried += 1
            vals = [np.random.default_rng(trial).standard_normal(8) for _ in range(3)]
            regs = {i: vals[i].copy() for i in range(3)}
            for i in range(3, 6):
                regs[i] = np.full(8, np.nan)
            run(cg.code, regs)
            for e, r in zip(outs, regs_out):
                assert np.array_equal(regs[r], evaluate(e, vals), equal_nan=True), (trial, e)
    assert tried > 500


def test_common_subexpression_handed_over_at_last_use():
    """t = exp(x0) is used twice: first as the left operand of t * x1 (it
    stays cached, so that use copies it), last as the left operand of
    t - x2: handed over in place, no second MOV."""
    x = [ir.Arg(i, F8, (0,)) for i in range(3)]
    t = ir.Unary("exp", x[0], F8)
    out = ir.Binary("add", ir.Binary("multiply", t, x[1], F8), ir.Binary("subtract", t, x[2], F8), F8)
    cg = Codegen(V_F64, {id(a): a.index for a in x})
    cg.count_uses([out])
    r, _ = cg.gen(out)
    movs = [c for c in cg.code if c[0] == _OPCODES["MOV"]]
    assert len(movs) == 1, cg.code
    vals = [np.linspace(-1, 1, 8) * (i + 1) for i in range(3)]
    regs = {i: vals[i].copy() for i in range(3)}
    for i in range(3, 6):
        regs[i] = np.full(8, np.nan)
    run(cg.code, regs)
    assert np.array_equal(regs[r], np.exp(vals[0]) * vals[1] + (np.exp(vals[0]) - vals[2]))


# --------------------------------------------------------------------------
# Elementwise conformance on the host: every op x dtype x fused form is
# lowered as the executor lowers it, run on the model of the VM (vm_model.py)
# and compared with numpy evaluating the same expression tree.
import pytest

import vm_model as M
from cubed_amd import lowering as L

N = 800  # elements per case: the edge product (at most 24 x 24) + random fill
FORMS = ["alone", "astype_f32", "astype_f64", "where"]


def op_program(op, dtype):
    dt = np.dtype(dtype)
    nargs = 1 if op in ir.UNARY_OPS else 2
    return ir.elementwise_program(op, [dt] * nargs, [1] * nargs, M.result_dtype(op, dt)), nargs


def form_program(op, dtype, form):
    """(program, number of array args) of ``op`` alone / followed by astype /
    feeding where(signbit(f32), op(..), y)."""
    p, nargs = op_program(op, dtype)
    rdt = M.result_dtype(op, dtype)
    if form == "alone":
        return p, nargs, 0
    if form.startswith("astype"):
        to = np.dtype("f4") if form.endswith("f32") else np.dtype("f8")
        c = ir.elementwise_program("astype", [rdt], [1], to)
        return ir.fuse_programs(c, [p], [nargs]), nargs, 0
    cond = ir.elementwise_program("signbit", [np.dtype("f4")], [1], np.bool_)
    w = ir.elementwise_program("where", [np.dtype(bool), rdt, rdt], [1, 1, 1], rdt)
    # args: cond's f32, the op's, then y (4 leaves at most: one fused program)
    return ir.fuse_programs(w, [cond, p, None], [1, nargs, 1]), nargs, 1


def form_arrays(op, dtype, form, nargs, n=N):
    xs = list(M.binary_inputs(op, dtype, n)) if nargs == 2 else [M.unary_inputs(op, dtype, n)]
    if form != "where":
        return xs
    rng = np.random.default_rng(3)
    c0 = rng.standard_normal(n).astype("f4")
    rdt = M.result_dtype(op, dtype)
    y = M.random_fill(rdt, n, 9)
    return [c0] + xs + [y]


def check(op, dtype, got, exp, what):
    if M.is_ulp(op, dtype):
        # the model runs numpy's routine in the register type: equal up to
        # the routine's own rounding (the GPU tests bound the device's error)
        ok = np.isfinite(exp)
        assert np.array_equal(np.isnan(got), np.isnan(exp)), what
        assert np.array_equal(got[~ok], exp[~ok], equal_nan=True), what
        g, e = got[ok].astype("f8"), exp[ok].astype("f8")
        fi = np.finfo(dtype)  # 2 ulps of the op's own dtype
        # (logaddexp = max + log1p(..) in [max, max + 0.7]: a result near 0
        # still carries the rounding of a sum of operands of size <= 0.7)
        floor = 1.0 if op.startswith("logaddexp") else fi.tiny
        tol = 2 * np.spacing(np.maximum(np.abs(exp[ok]), floor).astype(fi.dtype)).astype("f8")
        assert np.all(np.abs(g - e) <= tol), (what, np.abs(g - e).max())
    elif op in M.ZERO_SIGN_FREE:
        M.assert_value_equal(got, exp, what)
    else:
        M.assert_bit_equal(got, exp, what)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", [d.name for d in M.REAL_DTYPES])
def test_model_matches_numpy(dtype, form):
    """Every op valid at ``dtype``, in one fused form.  Pins the host half of
    the lowering: the register type, the CAST placement, the uint64 opcodes,
    and which integer nodes may run in float registers."""
    un, bi = M.ops_for(dtype)
    failures = []
    for op in un + bi:
        p, nargs, off = form_program(op, dtype, form)
        arrays = form_arrays(op, dtype, form, nargs)
        exp = M.np_eval(p.outputs, arrays)
        try:
            got, vtypes = M.model_eval(p, arrays)
            check(op, dtype, got, exp, (op, dtype, form, vtypes))
        except (AssertionError, M.UnknownOpcode) as e:
            failures.append(f"{op}: {type(e).__name__} {str(e)[:200]}")
    assert not failures, "\n".join(failures)


def test_model_refuses_unknown_opcodes():
    with pytest.raises(M.UnknownOpcode):
        M.run_code([(15, 0, 0, 0, 0, 0)], [], L.V_F64, {0: np.zeros(2)})
    with pytest.raises(M.UnknownOpcode):  # vm.h has no float case for shifts
        M.run_code([(ir.BINARY_OPS["bitwise_left_shift"], 0, 1, 0, 0, 0)], [], L.V_F64,
                   {0: np.ones(2), 1: np.ones(2)})


def test_model_covers_every_opcode():
    """Each name of ir.UNARY_OPS / ir.BINARY_OPS is run by the matrix above
    at some dtype, and the model has it in both register kinds it can reach."""
    un, bi = set(), set()
    for d in M.REAL_DTYPES:
        u, b = M.ops_for(d)
        un |= set(u)
        bi |= set(b)
    assert un == set(ir.UNARY_OPS) and bi == set(ir.BINARY_OPS)
    assert set(M.FLOAT_UNARY) == set(ir.UNARY_OPS) - {"positive"}
    assert set(M.FLOAT_BINARY) == set(ir.BINARY_OPS) - {"bitwise_left_shift", "bitwise_right_shift"}


def test_integer_shift_never_runs_in_float_registers():
    """astype(i32 << i32, f64): the shift is its own int64 program."""
    p, nargs, _ = form_program("bitwise_left_shift", "i4", "astype_f64")
    assert not L.program_fits(p)
    from cubed_amd.split import split_program

    parts, rest = split_program(p)
    assert [M.lower(s)[0] for s, _ in parts] == [L.V_I64] and parts[0][1] == np.dtype("i4")
    assert M.lower(rest)[0] == L.V_F64


def test_exact_integer_fusions_stay_fused():
    """int8 / int16 add in f32 registers and where() between int32 leaves in
    f64 registers are exact there: one program, as before."""
    for op, dt, form in [("add", "i1", "astype_f32"), ("subtract", "i2", "astype_f32"),
                         ("add", "u1", "where"), ("maximum", "i4", "astype_f64"), ("less", "i4", "where")]:
        p, _, _ = form_program(op, dt, form)
        assert L.program_fits(p), (op, dt, form)


def test_uint64_uses_unsigned_opcodes():
    for op, code in L._UNSIGNED_OPS.items():
        p, _ = op_program(op, "u8")
        vtype, cg, _, _, _ = M.lower(p)
        assert vtype == L.V_I64 and code in [c[0] for c in cg.code], op
        p, _ = op_program(op, "i8")
        assert code not in [c[0] for c in M.lower(p)[1].code], op


@pytest.mark.parametrize("src", [d.name for d in M.REAL_DTYPES])
def test_model_cast_matrix(src):
    """astype from ``src`` to each real dtype on the model, against numpy's
    astype: the register type must keep the source's value (an f64 leaf cast
    to bool or an integer does not go through an f32 register)."""
    for dst in M.REAL_DTYPES:
        x = M.cast_source(src, dst, 400)
        p = ir.elementwise_program("astype", [np.dtype(src)], [1], dst)
        with np.errstate(all="ignore"):
            exp = x.astype(dst)
        got, _ = M.model_eval(p, [x]) if np.dtype(src) != dst else (x, None)
        M.assert_bit_equal(got, exp, (src, dst.name))


def test_f64_to_f16_rounds_once():
    """astype(f64, f16) must not round through an f32 register: 1 + 2^-11 +
    2^-30 rounds up to 1 + 2^-10, through f32 it would tie down to 1."""
    p = ir.elementwise_program("astype", [np.dtype("f8")], [1], np.dtype("f2"))
    x = np.array([1 + 2.0 ** -11 + 2.0 ** -30, -(1 + 2.0 ** -11 + 2.0 ** -30), 0.1])
    got, vtypes = M.model_eval(p, [x])
    assert vtypes == [L.V_F64]
    M.assert_bit_equal(got, x.astype("f2"))


def test_headline_programs_lower_as_before():
    """mean((x + 1) * 2) in f32, mean(u * v) in f64 and the vorticity chain
    a * x + b * y keep their register type and instruction list."""
    f4, f8 = np.dtype("f4"), np.dtype("f8")
    x = ir.Arg(0, f4, (0, 1))
    e1 = ir.Binary("multiply", ir.Binary("add", x, ir.Const(1.0, f4), f4), ir.Const(2.0, f4), f4)
    u, v = ir.Arg(0, f8, (0, 1)), ir.Arg(1, f8, (0, 1))
    e2 = ir.Binary("multiply", u, v, f8)
    a, xx, b, y = (ir.Arg(i, f8, (0, 1)) for i in range(4))
    e3 = ir.Binary("add", ir.Binary("multiply", a, xx, f8), ir.Binary("multiply", b, y, f8), f8)
    ADD, MUL, CONST = ir.BINARY_OPS["add"], ir.BINARY_OPS["multiply"], L._OPCODES["CONST"]
    expect = [
        (e1, 1, L.V_F32, [(CONST, 1, 0, 0, 0, 0), (ADD, 0, 1, 0, 0, 0), (CONST, 1, 0, 0, 0, 1), (MUL, 0, 1, 0, 0, 0)]),
        (e2, 2, L.V_F64, [(MUL, 0, 1, 0, 0, 0)]),
        (e3, 4, L.V_F64, [(MUL, 0, 1, 0, 0, 0), (MUL, 2, 3, 0, 0, 0), (ADD, 0, 2, 0, 0, 0)]),
    ]
    for e, nargs, vt, code in expect:
        p = ir.reduce_program(2, e.dtype, (0,), [("n", "count", np.int64), ("total", "sum", np.float64)],
                              structured=True, value=e)
        assert L.program_fits(p)
        pre = L.dedupe_leaves([f.expr for f in p.reduce.fields])
        leaves = L.collect_leaves(pre)
        assert L.choose_vtype(pre, leaves) == vt
        assert L.float_exact(pre, vt)
        cg = L.Codegen(vt, {id(lf): i for i, lf in enumerate(leaves)})
        cg.count_uses(pre[:1])
        cg.gen(pre[0])
        assert cg.code == code, cg.code
