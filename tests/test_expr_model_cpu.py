"""The exact expression model (tests/expr_model.py) checked three ways, none of which needs a GPU: against numbers pinned by
hand, against Arrow C++ where it is known to agree with arrow-rs (int -> int, int -> float and float -> float casts, wrapping
integer + - * through numpy, integer comparisons; never decimals), and against the CPU oracle for every
vector set and error case of tests/expr_cases.py — the sets tests/test_gpu_expr_semantics.py runs through the kernels.
The host-side literal folding (csrc/expr.cpp fold_literal_cast) is checked here too, through the plan-only entry points."""
from __future__ import annotations

import math

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import qurious_amd as q
from qurious_amd import Operator as Op
from qurious_amd import planning

from . import expr_cases as C
from . import expr_model as M
from .expr_cases import BOOL, D32, D64, F32, F64, I8, I16, I32, I64, U8, U16, U32, U64, b, cast, col, dec, lit

V = M.Value


def ev(expr, *cols):
    return M.evaluate(expr, list(cols))


def cast1(frm, to, v):
    """the model's cast of one value: the value, or the error kind"""
    r = ev(cast(col("x", 0), to), V(frm, [v]))
    return r if isinstance(r, str) else r.values[0]


# ------------------------------------------------------------------------------------------------------- pinned by hand
def test_cast_multiplies_that_would_wrap_are_errors():
    # Int64 10^18 -> Decimal128(38, 30): the i128 product wraps to a value that passes |v| < 10^38
    wrapped = (10 ** 48 + (1 << 127)) % (1 << 128) - (1 << 127)
    assert wrapped == 18960114910927365649471927446130393088 and abs(wrapped) < 10 ** 38
    assert cast1(I64, dec(38, 30), 10 ** 18) == M.CAST_OVERFLOW
    # Decimal128(38, 0) 10^30 -> Decimal128(38, 9)
    wrapped = (10 ** 39 + (1 << 127)) % (1 << 128) - (1 << 127)
    assert wrapped == -20847100762815390390123822295304634368 and abs(wrapped) < 10 ** 38
    assert cast1(dec(38, 0), dec(38, 9), 10 ** 30) == M.CAST_OVERFLOW
    # the check is |value| < 10^(precision - k); value == 0 when precision < k
    assert cast1(I64, dec(38, 30), 10 ** 8 - 1) == (10 ** 8 - 1) * 10 ** 30 and cast1(I64, dec(38, 30), 10 ** 8) == M.CAST_OVERFLOW
    assert cast1(I64, dec(38, 30), 1 - 10 ** 8) == (1 - 10 ** 8) * 10 ** 30 and cast1(I64, dec(38, 30), -10 ** 8) == M.CAST_OVERFLOW
    assert cast1(dec(38, 0), dec(38, 9), 10 ** 29 - 1) == (10 ** 29 - 1) * 10 ** 9 and cast1(dec(38, 0), dec(38, 9), 10 ** 29) == M.CAST_OVERFLOW
    assert cast1(I32, dec(2, 5), 0) == 0 and cast1(I32, dec(2, 5), 1) == M.CAST_OVERFLOW and cast1(I32, dec(5, 5), -1) == M.CAST_OVERFLOW


def test_float_to_int_bounds_are_those_of_num_cast():
    p63, p64, p31 = float(1 << 63), float(1 << 64), float(1 << 31)
    assert float((1 << 63) - 1) == p63            # (double)INT64_MAX is 2^63: `<=` against it lets 2^63 through
    assert cast1(F64, I64, p63) == M.CAST_OVERFLOW and cast1(F64, I64, C.below(p63)) == (1 << 63) - 1024
    assert cast1(F64, I64, -p63) == -(1 << 63) and cast1(F64, I64, C.below(-p63)) == M.CAST_OVERFLOW
    assert cast1(F64, U64, p64) == M.CAST_OVERFLOW and cast1(F64, U64, C.below(p64)) == (1 << 64) - 2048
    assert cast1(F64, U64, -0.5) == 0 and cast1(F64, U64, -0.0) == 0 and cast1(F64, U64, -1.0) == M.CAST_OVERFLOW
    assert cast1(F64, I32, p31) == M.CAST_OVERFLOW and cast1(F64, I32, C.below(p31)) == (1 << 31) - 1
    assert cast1(F64, I32, C.below(-p31)) == -(1 << 31)       # truncation comes first
    assert cast1(F64, I32, -p31 - 1.0) == M.CAST_OVERFLOW
    assert cast1(F32, I32, p31) == M.CAST_OVERFLOW and cast1(F32, I32, C.f32_below(p31)) == 2147483520
    assert cast1(F64, I8, 127.9) == 127 and cast1(F64, I8, -128.9) == -128 and cast1(F64, I8, 128.0) == M.CAST_OVERFLOW
    assert cast1(F64, I64, 2.5) == 2 and cast1(F64, I64, -2.5) == -2 and cast1(F64, I64, -0.5) == 0
    for bad in (math.nan, math.inf, -math.inf):
        assert cast1(F64, I64, bad) == M.CAST_OVERFLOW and cast1(F64, U8, bad) == M.CAST_OVERFLOW


def test_float_to_decimal_checks_the_precision_on_the_integer():
    assert int(float(10 ** 23)) == 99999999999999991611392 < 10 ** 23
    for p in (23, 24, 38):   # the double nearest to 10^p lies below it: a legal value
        assert int(float(10 ** p)) < 10 ** p
        assert cast1(F64, dec(p, 0), float(10 ** p)) == int(float(10 ** p))
        assert cast1(F64, dec(p, 0), -float(10 ** p)) == -int(float(10 ** p))
        assert cast1(F64, dec(p, 0), C.above(float(10 ** p))) == M.CAST_OVERFLOW
    assert int(float(10 ** 22)) == 10 ** 22 and cast1(F64, dec(22, 0), 1e22) == M.CAST_OVERFLOW
    assert cast1(F64, dec(10, 2), 0.125) == 13 and cast1(F64, dec(10, 2), -0.125) == -13     # 12.5 rounds away from zero
    assert cast1(F64, dec(10, 0), 0.5) == 1 and cast1(F64, dec(10, 0), 2.5) == 3 and cast1(F64, dec(10, 0), -2.5) == -3 and cast1(F64, dec(10, 0), -0.0) == 0
    for bad in (math.nan, math.inf, -math.inf, 1e300):
        assert cast1(F64, dec(38, 0), bad) == M.CAST_OVERFLOW


def test_int64_to_float32_is_rounded_once():
    v = (1 << 60) + (1 << 36) + 1
    assert M.int_to_f32(v) == float((1 << 60) + (1 << 37))     # one rounding
    assert M.f32(float(v)) == float(1 << 60)                    # two roundings: through Float64 first
    assert cast1(I64, F32, v) == float((1 << 60) + (1 << 37)) and cast1(U64, F32, v) == float((1 << 60) + (1 << 37))
    assert cast1(I64, F32, (1 << 24) + 1) == float(1 << 24) and cast1(I64, F32, (1 << 24) + 3) == float((1 << 24) + 4)   # ties to even
    assert cast1(I64, F32, -((1 << 24) + 3)) == -float((1 << 24) + 4)
    assert cast1(I64, F64, (1 << 53) + 1) == float(1 << 53) and cast1(I64, F64, (1 << 53) + 3) == float((1 << 53) + 4)
    assert cast1(U64, F32, (1 << 64) - 1) == float(1 << 64) and cast1(I64, F32, -(1 << 63)) == -float(1 << 63)


def test_one_row_per_cast_branch():
    assert cast1(I64, I8, 127) == 127 and cast1(I64, I8, 128) == M.CAST_OVERFLOW and cast1(I64, I8, -129) == M.CAST_OVERFLOW
    assert cast1(I8, U8, -1) == M.CAST_OVERFLOW and cast1(U64, I64, 1 << 63) == M.CAST_OVERFLOW and cast1(U8, I8, 127) == 127
    assert cast1(D32, D64, -3) == -3 * 86_400_000 and cast1(D64, D32, 86_399_999) == 0 and cast1(D64, D32, -86_400_001) == -1    # truncating
    assert cast1(D32, I32, 9000) == 9000 and cast1(I32, D32, -1) == -1
    assert cast1(F64, F32, float((1 << 24) + 1)) == float(1 << 24) and cast1(F64, F32, 1e300) == math.inf and cast1(F32, F64, 0.5) == 0.5
    assert cast1(dec(9, 2), dec(9, 0), 50) == 1 and cast1(dec(9, 2), dec(9, 0), 49) == 0 and cast1(dec(9, 2), dec(9, 0), -50) == -1 and cast1(dec(9, 2), dec(9, 0), -149) == -1
    assert cast1(dec(9, 2), dec(7, 0), 999999949) == 9999999 and cast1(dec(9, 2), dec(7, 0), 999999950) == M.CAST_OVERFLOW   # rounds to 10^7
    assert cast1(dec(18, 4), I32, 21474836479999) == (1 << 31) - 1 and cast1(dec(18, 4), I32, 21474836480000) == M.CAST_OVERFLOW
    assert cast1(dec(18, 4), I32, -21474836489999) == -(1 << 31) and cast1(dec(18, 4), I32, -9999) == 0                  # truncating
    assert cast1(dec(9, 2), F64, 12345) == 123.45 and cast1(dec(9, 2), F32, 12345) == M.f32(123.45) and cast1(dec(38, 10), F64, 1 << 100) == float(1 << 100) / 1e10
    assert cast1(BOOL, I32, True) == 1 and cast1(BOOL, U8, False) == 0
    assert cast1(I64, I8, None) is None


def test_one_row_per_arithmetic_branch():
    one = lambda t, op, x, y: ev(b(col("x", 0), op, col("y", 1)), V(t, [x]), V(t, [y]))   # noqa: E731
    val = lambda *a: one(*a).values[0]   # noqa: E731
    assert val(I8, Op.Add, 127, 1) == -128 and val(U8, Op.Sub, 0, 1) == 255 and val(I16, Op.Mul, 256, 128) == -32768
    assert val(I32, Op.Add, (1 << 31) - 1, 1) == -(1 << 31) and val(U32, Op.Mul, 1 << 31, 2) == 0
    assert val(I64, Op.Mul, 1 << 62, 2) == -(1 << 63) and val(U64, Op.Add, (1 << 64) - 1, 2) == 1
    assert val(I64, Op.Div, -7, 2) == -3 and val(I64, Op.Mod, -7, 2) == -1 and val(I64, Op.Mod, 7, -2) == 1      # C semantics
    assert one(I64, Op.Div, 1, 0) == M.DIVIDE_BY_ZERO and one(U8, Op.Mod, 1, 0) == M.DIVIDE_BY_ZERO
    assert one(I64, Op.Div, -(1 << 63), -1) == M.ARITH_OVERFLOW and one(I8, Op.Div, -128, -1) == M.ARITH_OVERFLOW
    assert val(I64, Op.Mod, -(1 << 63), -1) == 0      # today's answer; see the doubt in expr_model.py
    assert val(I64, Op.Div, None, 0) is None and val(I64, Op.Div, 1, None) is None     # valid rows only
    neg = lambda t, x: ev(q.Negative(col("x", 0)), V(t, [x])).values[0]   # noqa: E731
    assert neg(I8, -128) == -128 and neg(I64, 5) == -5 and neg(dec(9, 2), 5) == -5 and math.copysign(1.0, neg(F64, 0.0)) == -1.0
    # decimals: the result types of binary.rs and the rescaling
    r = ev(b(col("x", 0), Op.Add, col("y", 1)), V(dec(9, 2), [150]), V(dec(18, 4), [1]))
    assert r == V(dec(19, 4), [15001])
    r = ev(b(col("x", 0), Op.Sub, col("y", 1)), V(dec(18, 4), [1]), V(dec(9, 2), [150]))
    assert r == V(dec(19, 4), [-14999])
    r = ev(b(col("x", 0), Op.Mul, col("y", 1)), V(dec(9, 2), [-150]), V(dec(18, 4), [3]))
    assert r == V(dec(28, 6), [-450])
    r = ev(b(col("x", 0), Op.Div, col("y", 1)), V(dec(9, 2), [150]), V(dec(9, 2), [-300]))
    assert r == V(F64, [-0.5])
    # floats
    assert val(F32, Op.Add, 16777216.0, 1.0) == 16777216.0 and val(F64, Op.Mod, -7.5, 2.0) == -1.5 and val(F64, Op.Div, 1.0, -0.0) == -math.inf
    cmp = lambda op, x, y: one(F64, op, x, y).values[0]   # noqa: E731
    assert cmp(Op.Lt, -0.0, 0.0) and not cmp(Op.Eq, -0.0, 0.0) and cmp(Op.Eq, math.nan, math.nan) and cmp(Op.Gt, math.nan, math.inf)
    assert cmp(Op.Lt, -math.nan, -math.inf)   # (a negative NaN is below everything)
    # Kleene logic, IS NULL, IF
    tf = V(BOOL, [True, True, True, False, False, False, None, None, None])
    ft = V(BOOL, [True, False, None, True, False, None, True, False, None])
    assert ev(b(col("x", 0), Op.And, col("y", 1)), tf, ft).values == [True, False, None, False, False, False, None, False, None]
    assert ev(b(col("x", 0), Op.Or, col("y", 1)), tf, ft).values == [True, True, True, True, False, None, True, None, None]
    assert ev(q.IsNull(col("x", 0)), V(I64, [1, None])).values == [False, True] and ev(q.IsNotNull(col("x", 0)), V(I64, [1, None])).values == [True, False]
    iff = q.CaseExpr([(col("m", 0), col("x", 1))], col("y", 2))
    assert ev(iff, V(BOOL, [True, False, None]), V(I64, [1, 2, 3]), V(I64, [10, None, 30])).values == [1, None, 30]
    # ... both sides are evaluated for every row: the side that is never taken raises all the same
    never = q.CaseExpr([(col("m", 0), b(col("x", 1), Op.Div, col("y", 2)))], col("x", 1))
    assert ev(never, V(BOOL, [False]), V(I64, [1]), V(I64, [0])) == M.DIVIDE_BY_ZERO


def test_buffers_round_trip_and_garbage_lies_under_nulls():
    for t, vals, g in ((I8, [-128, None, 127], 55), (U64, [None, (1 << 64) - 1], 7), (F32, [0.5, None, -0.0], math.inf), (F64, [math.nan, None], 1e300),
                       (dec(38, 10), [-(10 ** 38 - 1), None, 1 << 100], (1 << 127) - 1), (BOOL, [True, None, False], True), (D64, [None, -5], 9), (D32, [3, None], 9)):
        arr = M.to_arrow(t, vals, g)
        assert arr.type == t and arr.null_count == sum(v is None for v in vals)
        back = M.from_arrow(arr)
        assert M.same_values(t, back.values, vals) is None
        if not pa.types.is_boolean(t):
            # the garbage really is in the values buffer
            raw = M.from_arrow(pa.Array.from_buffers(t, len(vals), [None, arr.buffers()[1]]))
            assert M.same_values(t, [raw.values[k] for k, v in enumerate(vals) if v is None], [g] * arr.null_count) is None
    assert M.same_values(F64, [0.0], [-0.0]) is not None and M.same_values(F64, [math.nan], [math.nan]) is None and M.same_values(F64, [math.nan], [-math.nan]) is not None


# ----------------------------------------------------------------------------------------------------- against Arrow C++
def test_model_against_arrow_cpp_where_it_agrees_with_arrow_rs():
    ints = C.vector_set("ints")
    by_name = dict(zip(ints.names, ints.cols))
    arrays = dict(zip(ints.names, ints.batch.columns))
    # int -> int in range, int -> float (one rounding: Arrow C++ converts directly), float -> float
    for src, to in (("s64", I8), ("s64", I16), ("a16", I32), ("a32", I64), ("u8", U64), ("u32", I64), ("a64", F32), ("a64", F64), ("u64", F32), ("u64", F64), ("a32", F32)):
        want = M.from_arrow(pc.cast(arrays[src], to, safe=False))
        got = ev(cast(col(src, 0), to), by_name[src])
        assert M.same_values(to, got.values, want.values) is None, (src, to)
    floats = C.vector_set("floats")
    x64, y32 = floats.cols[floats.names.index("x64")], floats.cols[floats.names.index("y32")]
    assert M.same_values(F32, ev(cast(col("x", 0), F32), x64).values, M.from_arrow(pc.cast(floats.batch.column(0), F32, safe=False)).values) is None
    assert M.same_values(F64, ev(cast(col("y", 0), F64), y32).values, M.from_arrow(pc.cast(floats.batch.column(floats.names.index("y32")), F64)).values) is None
    # wrapping + - * through numpy, comparisons through pyarrow.compute
    for name, t, npt in (("a8", I8, np.int8), ("a16", I16, np.int16), ("a32", I32, np.int32), ("a64", I64, np.int64), ("u8", U8, np.uint8), ("u16", U16, np.uint16),
                         ("u32", U32, np.uint32), ("u64", U64, np.uint64)):
        x = by_name[name]
        y = V(t, list(reversed(x.values)))
        xs, ys = np.array([v or 0 for v in x.values], dtype=npt), np.array([v or 0 for v in y.values], dtype=npt)
        with np.errstate(over="ignore"):
            for op, fn in ((Op.Add, np.add), (Op.Sub, np.subtract), (Op.Mul, np.multiply)):
                want = [None if a is None or c is None else int(w) for a, c, w in zip(x.values, y.values, fn(xs, ys))]
                assert ev(b(col("x", 0), op, col("y", 1)), x, y).values == want, (name, op)
        ax, ay = pa.array(x.values, type=t), pa.array(y.values, type=t)
        for op, fn in ((Op.Eq, pc.equal), (Op.NotEq, pc.not_equal), (Op.Lt, pc.less), (Op.LtEq, pc.less_equal), (Op.Gt, pc.greater), (Op.GtEq, pc.greater_equal)):
            assert ev(b(col("x", 0), op, col("y", 1)), x, y).values == fn(ax, ay).to_pylist(), (name, op)


# --------------------------------------------------------------------------------------------------- against the oracle
def test_no_value_vector_raises():
    """The model returns a value, never an error, for every expression of every vector set: the GPU tests leave nothing out."""
    total = 0
    for name in C.SET_NAMES:
        vs = C.vector_set(name)
        every = ([e for _, e in vs.exprs] + [e for _, e in vs.filters] + [a[1] for a in vs.agg_args] + [vs.agg_key, vs.agg_filter, vs.join_filter] + vs.join_keys)
        for e in every:
            r = M.evaluate(e, vs.cols)
            assert not isinstance(r, str), (name, str(e), r)
            total += 1
        assert all(len(c.values) == C.N == 3 * 1024 + 37 for c in vs.cols)
        assert all(0.05 < sum(v is None for v in c.values) / C.N < 0.15 for c in vs.cols[:-1])
    assert total > 200
    et = C.error_table()
    assert all(not isinstance(M.evaluate(e, et.case()[0]), str) for _, e in et.exprs())


@pytest.mark.parametrize("name", C.SET_NAMES)
def test_oracle_agrees_with_the_model_on_every_vector_set(oracle, name):
    vs = C.vector_set(name)
    for label, e in vs.exprs + vs.filters + [(a[0], a[1]) for a in vs.agg_args] + [("group key", vs.agg_key)] + [("join key", k) for k in vs.join_keys]:
        want = M.evaluate(e, vs.cols)
        got = oracle.evaluate(e, vs.batch)
        assert got.type == want.type, (label, got.type, want.type)
        assert M.same_values(want.type, M.from_arrow(got).values, want.values) is None, (name, label, M.same_values(want.type, M.from_arrow(got).values, want.values))


def test_oracle_agrees_with_the_model_on_every_error_case(oracle):
    et = C.error_table()
    for n, (pname, _poison, kind) in enumerate(et.POISONS):
        for row in (C.POISON_ROWS[0], C.POISON_ROWS[-1]):
            live, batch = et.case(pname, row, "live")
            kinds = {fam: M.evaluate(e, live) for fam, e in et.exprs()}
            assert {k for k in kinds.values() if isinstance(k, str)} == {kind}, (pname, kinds)
            for fam, e in et.exprs():
                if isinstance(kinds[fam], str):
                    with pytest.raises(oracle.OracleError, match=M.MESSAGE[kind]):
                        oracle.evaluate(e, batch)
                else:
                    assert M.same_values(kinds[fam].type, M.from_arrow(oracle.evaluate(e, batch)).values, kinds[fam].values) is None, (pname, fam)
        # under a NULL the poison is never read
        nulled, batch = et.case(pname, C.POISON_ROWS[n % 3], "null")
        for fam, e in et.exprs():
            want = M.evaluate(e, nulled)
            assert not isinstance(want, str), (pname, fam)
            assert M.same_values(want.type, M.from_arrow(oracle.evaluate(e, batch)).values, want.values) is None, (pname, fam)


# ------------------------------------------------------------------------------- literal casts are folded on the host
def _folds(value_type, v, to):
    """plans CAST(literal AS to) next to a column; a folding error surfaces as the planner's error"""
    planning.projection_source(pa.schema([pa.field("x", I64)]), [cast(lit(value_type, v), to)])


@pytest.mark.parametrize("frm, v, to, legal", [
    (I64, 10 ** 18, dec(38, 30), False), (I64, 10 ** 8, dec(38, 30), False), (I64, 10 ** 8 - 1, dec(38, 30), True), (I64, 1 - 10 ** 8, dec(38, 30), True),
    (dec(38, 0), 10 ** 30, dec(38, 9), False), (dec(38, 0), -10 ** 29, dec(38, 9), False), (dec(38, 0), 10 ** 29 - 1, dec(38, 9), True),
    (I32, 1, dec(2, 5), False), (I32, 0, dec(2, 5), True),
    (F64, float(1 << 63), I64, False), (F64, C.below(float(1 << 63)), I64, True), (F64, -float(1 << 63), I64, True), (F64, C.below(-float(1 << 63)), I64, False),
    (F64, float(1 << 64), U64, False), (F64, C.below(float(1 << 64)), U64, True), (F64, -0.5, U64, True), (F64, float(1 << 31), I32, False),
    (F64, float(10 ** 23), dec(23, 0), True), (F64, C.above(float(10 ** 23)), dec(23, 0), False), (F64, float(10 ** 38), dec(38, 0), True),
    (dec(9, 2), 999999950, dec(7, 0), False), (dec(9, 2), 999999949, dec(7, 0), True),
])
def test_literal_cast_folding_raises_exactly_where_the_model_does(frm, v, to, legal):
    assert (cast1(frm, to, v) != M.CAST_OVERFLOW) == legal
    if legal:
        _folds(frm, v, to)
    else:
        with pytest.raises(q.QuriousError, match="Cast error"):
            _folds(frm, v, to)
