"""Device expressions against the exact model (tests/expr_model.py), directly — not through the oracle, which restates the same
reading of arrow-rs as the kernels do. Integers and decimals must be equal, floats equal bit for bit (NaN included): every
case is one correctly rounded operation (a Decimal128 -> Float32 cast: the two roundings the reference makes).

The value vectors and expressions are those of tests/expr_cases.py (three tiles of 1024 rows and a ragged tail, ~10 % NULLs
with garbage under them that would raise if read). Each family runs where the generator differs:
  (P) Projection                  non-raw loads
  (F) Filter predicate            the mask kernel, raw tile loads
  (A) fused aggregate             argument of SUM / MIN / MAX and GROUP BY key, with and without a fused predicate
  (K) inner hash join key         both sides under a fused scan filter, `auto` and `hashed` layouts
  and one sort key.
Error cases are ONE plan per context over a table in which exactly one row is poisoned (first tile, last full tile, ragged
tail), then the same poison under a NULL and under a row the fused filter rejects: those two must give the model's values.

Many expressions share a kernel (a Projection takes 20 here) and plans are rebuilt over new data with the same text, so
the file compiles about 55 generated modules (10 projections, 19 masks, 15 aggregates, 8 join-key pairs, a sort key and a few
layout variants of the error table) and runs in about 40 s alone on an MI355X, compiles included."""
from __future__ import annotations

import pyarrow as pa
import pytest

import qurious_amd as q
from qurious_amd import JoinType
from qurious_amd import Operator as Op

from . import expr_cases as C
from . import expr_model as M
from .expr_cases import F32, F64, I32, I64, U64, b, cast, dec, lit

pytestmark = pytest.mark.gpu

_TABLES = {}
MEMO = M.Memo()   # the model's results, shared by every test (tables that differ in one column share the rest)


def _table(name):
    """a vector set's MemoryTable: uploaded once, shared by every test"""
    if name not in _TABLES:
        _TABLES[name] = C.vector_set(name).table()
    return _TABLES[name]


def _columns(batches, schema=None):
    """the output columns as model Values"""
    if not batches:
        return []
    return [M.from_arrow(pa.chunked_array([bt.column(k) for bt in batches])) for k in range(batches[0].num_columns)]


def _check(label, got: M.Value, want: M.Value):
    assert got.type == want.type, (label, got.type, want.type)
    diff = M.same_values(want.type, got.values, want.values)
    assert diff is None, (label, diff)


# ------------------------------------------------------------------------------------------------------- (P) projection
@pytest.mark.parametrize("name", C.SET_NAMES)
def test_projection_equals_the_model(ctx, name):
    vs = C.vector_set(name)
    scan = vs.scan(table=_table(name))
    for chunk in C.chunks(vs.exprs):
        out = _columns(q.Projection(None, scan, [e for _, e in chunk]).execute())
        assert len(out) == len(chunk)
        for (label, e), got in zip(chunk, out):
            _check((name, label), got, M.evaluate(e, vs.cols))


def test_folded_literal_casts_equal_the_casts_of_a_column(ctx):
    """A literal cast is folded on the host (fold_literal_cast) and must give what the kernel gives for a column: the Int64 ->
    Float32 literal used to be rounded twice."""
    vs = C.vector_set("ints")
    v = (1 << 60) + (1 << 36) + 1
    exprs = [cast(lit(I64, v), F32), cast(lit(U64, v), F32), cast(lit(I64, (1 << 24) + 3), F32), cast(lit(I64, (1 << 53) + 1), F64), cast(lit(U64, (1 << 64) - 1), F32),
             cast(lit(I64, 10 ** 8 - 1), dec(38, 30)), cast(lit(dec(38, 0), 1 - 10 ** 29), dec(38, 9)), cast(lit(F64, float(10 ** 23)), dec(23, 0)),
             cast(lit(F64, float(10 ** 38)), dec(38, 0)), cast(lit(F64, C.below(float(1 << 63))), I64), cast(lit(F64, C.below(float(1 << 64))), U64),
             cast(lit(F64, C.below(-float(1 << 31))), I32), cast(lit(dec(9, 2), -999999949), dec(7, 0)), cast(lit(F64, -0.125), dec(10, 2))]
    # (next to a column, so that the plan is a kernel and not a constant)
    out = _columns(q.Projection(None, vs.scan(table=_table("ints")), [vs.id] + exprs).execute())
    for e, got in zip(exprs, out[1:]):
        _check(str(e), got, M.evaluate(e, vs.cols))


# ----------------------------------------------------------------------------------------------------------- (F) filter
@pytest.mark.parametrize("name", C.SET_NAMES)
def test_filter_predicate_equals_the_model(ctx, name):
    vs = C.vector_set(name)
    scan = vs.scan(table=_table(name))
    for label, pred in vs.filters:
        out = _columns(q.Filter(scan, pred).execute())
        mask = M.evaluate(pred, vs.cols)
        want = [k for k, m in enumerate(mask.values) if m]
        assert 0 < len(want) < C.N, label   # (the literal splits the vector)
        assert (out[-1].values if out else []) == want, (name, label)


# -------------------------------------------------------------------------------------------------- (A) fused aggregate
_AGG = {"sum": q.SumAggregateExpr, "min": q.MinAggregateExpr, "max": q.MaxAggregateExpr}


def _agg_exprs(args):
    """[(label, kind, expression, type)] and the AggregateExprs"""
    flat = [(label, kind, e) for label, e, kinds in args for kind in kinds]
    return flat


def _model_aggregate(cols, flat, key_expr, pred):
    if pred is not None:
        cols = MEMO.keep_rows(cols, MEMO.evaluate(pred, cols))
    groups = None
    if key_expr is not None:
        kv = MEMO.evaluate(key_expr, cols)
        assert not isinstance(kv, str)
        groups = kv.values
    out = []
    for label, kind, e in flat:
        v = MEMO.evaluate(e, cols)
        if isinstance(v, str):
            return v
        out.append((v.type, MEMO.aggregate(kind, v, groups)))
    return out


def _run_aggregate(source, flat, types, key_expr):
    aggs = [_AGG[kind](e, t) for (label, kind, e), t in zip(flat, types)]
    out = _columns(q.HashAggregate(None, source, [key_expr] if key_expr is not None else [], aggs).execute())
    nk = 1 if key_expr is not None else 0
    keys = out[0].values if nk else [()] * len(out[0].values)
    assert len(set(keys)) == len(keys)
    return keys, out[nk:]


def _check_aggregate(label, source, cols, flat, key_expr, pred):
    want = _model_aggregate(cols, flat, key_expr, pred)
    assert not isinstance(want, str), (label, want)
    keys, got = _run_aggregate(source, flat, [t for t, _ in want], key_expr)
    assert sorted(keys, key=lambda k: (k is not None, k)) == sorted(want[0][1], key=lambda k: (k is not None, k)), (label, "groups")
    for (alabel, kind, _e), (t, per_group), col_ in zip(flat, want, got):
        assert col_.type == t, (label, alabel, kind, col_.type, t)
        diff = M.same_values(t, col_.values, [per_group[k] for k in keys])
        assert diff is None, (label, alabel, kind, diff)


@pytest.mark.parametrize("fused", ["no predicate", "Scan(filter)", "Filter(Scan)"])
@pytest.mark.parametrize("grouped", ["grouped", "ungrouped"])
@pytest.mark.parametrize("name", C.SET_NAMES)
def test_fused_aggregate_equals_the_model(ctx, name, grouped, fused):
    vs = C.vector_set(name)
    pred = None if fused == "no predicate" else vs.agg_filter
    table = _table(name)
    source = vs.scan(table=table) if pred is None else vs.scan(pred, table) if fused == "Scan(filter)" else q.Filter(vs.scan(table=table), pred)
    _check_aggregate((name, grouped, fused), source, vs.cols, _agg_exprs(vs.agg_args), vs.agg_key if grouped == "grouped" else None, pred)


# ------------------------------------------------------------------------------------------------------- (K) join keys
def _model_join(lcols, rcols, keys, lpred, rpred):
    """sorted (left id, right id) of the inner join on the key expressions, each side filtered first; or an error kind"""
    sides = []
    for cols, pred in ((lcols, lpred), (rcols, rpred)):
        if pred is not None:
            mask = MEMO.evaluate(pred, cols)
            if isinstance(mask, str):
                return mask
            cols = MEMO.keep_rows(cols, mask)
        kv = [MEMO.evaluate(k, cols) for k in keys]
        for v in kv:
            if isinstance(v, str):
                return v
        sides.append([(tuple(v.values[r] for v in kv), cols[-1].values[r]) for r in range(len(cols[-1].values))])
    build = {}
    for key, rid in sides[0]:
        if None not in key:
            build.setdefault(key, []).append(rid)
    return sorted((lid, rid) for key, rid in sides[1] if None not in key for lid in build.get(key, []))


def _run_join(schema, ltable, rtable, keys, lpred, rpred):
    left, right = q.Scan(schema, ltable, None, lpred), q.Scan(schema, rtable, None, rpred)
    out = _columns(q.HashJoinExec.try_new(left, right, JoinType.Inner, [(k, k) for k in keys], None).execute())
    n = len(schema)
    return sorted(zip(out[n - 1].values, out[2 * n - 1].values)) if out else []


# the join_layout fixture, under its `auto` and `hashed` layouts only: a key EXPRESSION never takes the dense layouts
_auto_and_hashed = pytest.mark.parametrize("join_layout", ["auto", "hashed"], indirect=True)


@_auto_and_hashed
@pytest.mark.parametrize("name", C.SET_NAMES)
def test_join_key_expressions_equal_the_model(ctx, join_layout, name):
    vs = C.vector_set(name)
    small = M.keep_rows(vs.cols, M.Value(pa.bool_(), [r % 11 == 0 for r in range(C.N)]))   # the build side: every 11th row
    small_batch = vs.batch.take(pa.array(small[-1].values, type=I64))
    got = _run_join(vs.schema, q.MemoryTable.try_new(vs.schema, [small_batch]), _table(name), vs.join_keys, vs.join_filter, vs.join_filter)
    want = _model_join(small, vs.cols, vs.join_keys, vs.join_filter, vs.join_filter)
    assert not isinstance(want, str) and len(want) > 100
    assert got == want


# -------------------------------------------------------------------------------------------------------- one sort key
def test_sort_key_expression_equals_the_model(ctx):
    vs = C.vector_set("ints")
    key = cast(vs.c("a64"), F32)
    plan = q.Sort([q.PhysicalSortExpr(key, q.SortOptions(descending=False, nulls_first=True)), q.PhysicalSortExpr(vs.id, q.SortOptions(False, True))],
                  vs.scan(table=_table("ints")))
    got = _columns(plan.execute())[-1].values
    kv = M.evaluate(key, vs.cols).values
    want = sorted(range(C.N), key=lambda r: (kv[r] is not None, M.total_order_key(kv[r]) if kv[r] is not None else 0, r))
    assert got == want


# ---------------------------------------------------------------------------------------------------------- error cases
def _err_exprs():
    return C.error_table().exprs()


_KINDS = {}


def _expected_kind(case, cols, exprs):
    """the one error kind the model ends with over `cols`, or None; computed once per case and shared by the contexts"""
    if case not in _KINDS:
        kinds = {k for k in (MEMO.evaluate(e, cols) for e in exprs) if isinstance(k, str)}
        assert len(kinds) <= 1
        _KINDS[case] = kinds.pop() if kinds else None
    return _KINDS[case]


def _error_runs():
    """(poison name, row, mode): live in each of the three positions, then under a NULL and under a rejected row"""
    et = C.error_table()
    for n, (pname, _p, _k) in enumerate(et.POISONS):
        for row in C.POISON_ROWS:
            yield pname, row, "live"
        yield pname, C.POISON_ROWS[n % 3], "null"
        yield pname, C.POISON_ROWS[(n + 1) % 3], "rejected"


def _any_null(exprs):
    """a predicate that evaluates every expression: e1 IS NULL OR e2 IS NULL OR ..."""
    pred = q.IsNull(exprs[0])
    for e in exprs[1:]:
        pred = b(pred, Op.Or, q.IsNull(e))
    return pred


def test_errors_in_a_projection(ctx):
    et = C.error_table()
    exprs = [e for _, e in _err_exprs()]
    for pname, row, mode in _error_runs():
        if mode == "rejected":
            continue   # (no filter in this plan)
        cols, batch = et.case(pname, row, mode)
        plan = q.Projection(None, q.Scan(et.schema, q.MemoryTable.try_new(et.schema, [batch]), None, None), exprs)
        kind = _expected_kind((pname, row, mode), cols, exprs)
        assert (kind is not None) == (mode == "live")
        if kind:
            with pytest.raises(q.QuriousError, match=M.MESSAGE[kind]):
                plan.execute()
        else:
            for e, got in zip(exprs, _columns(plan.execute())):
                _check((pname, mode, str(e)), got, MEMO.evaluate(e, cols))


def test_errors_in_a_filter_predicate(ctx):
    et = C.error_table()
    exprs = [e for _, e in _err_exprs()]
    pred = _any_null(exprs)
    for pname, row, mode in _error_runs():
        if mode == "rejected":
            continue
        cols, batch = et.case(pname, row, mode)
        plan = q.Filter(q.Scan(et.schema, q.MemoryTable.try_new(et.schema, [batch]), None, None), pred)
        kind = _expected_kind((pname, row, mode), cols, exprs)
        if kind:
            with pytest.raises(q.QuriousError, match=M.MESSAGE[kind]):
                plan.execute()
        else:
            want = [k for k, m in enumerate(MEMO.evaluate(pred, cols).values) if m]
            assert _columns(plan.execute())[-1].values == want, (pname, mode)


@pytest.mark.parametrize("fused", ["no predicate", "Scan(filter)", "Filter(Scan)", "the predicate evaluates the poison"])
def test_errors_in_a_fused_aggregate(ctx, fused):
    """Keys and arguments raise only for rows the fused filter passes: the reference filters first. What the predicate itself
    evaluates raises for every row: the reference evaluates the predicate on every row."""
    et = C.error_table()
    fam = dict(_err_exprs())
    key = fam["ci"]   # GROUP BY CAST(ci AS Int32): a fallible key
    flat = [(name, "min", e) for name, e in _err_exprs() if name != "ci"]
    exprs = [e for _, e in _err_exprs()]
    types = [MEMO.evaluate(e, et.case()[0]).type for _, _, e in flat]
    if fused == "no predicate":
        pred = None
    elif fused == "the predicate evaluates the poison":
        pred = b(et.filter(), Op.And, q.IsNotNull(b(_any_null(exprs), Op.Or, q.IsNull(et.c("g")))))   # g > 0 AND (always true, evaluates everything)
    else:
        pred = et.filter()
    for pname, row, mode in _error_runs():
        if mode == "rejected" and pred is None:
            continue
        cols, batch = et.case(pname, row, mode)
        table = q.MemoryTable.try_new(et.schema, [batch])
        source = q.Scan(et.schema, table, None, None) if pred is None else q.Filter(q.Scan(et.schema, table, None, None), pred) if fused == "Filter(Scan)" \
            else q.Scan(et.schema, table, None, pred)
        if fused == "the predicate evaluates the poison" or pred is None:
            kind = _expected_kind((pname, row, mode), cols, exprs)             # the predicate sees every row, rejected ones included
            assert (kind is not None) == (mode != "null")
        else:
            kind = _expected_kind((pname, row, mode, "filtered"), MEMO.keep_rows(cols, MEMO.evaluate(pred, cols)), exprs)
            assert (kind is not None) == (mode == "live")
        if kind:
            with pytest.raises(q.QuriousError, match=M.MESSAGE[kind]):
                _run_aggregate(source, flat, types, key)
        else:
            _check_aggregate((fused, pname, mode), source, cols, flat, key, pred)


@_auto_and_hashed
def test_errors_in_join_keys_under_scan_filters(ctx, join_layout):
    et = C.error_table()
    fam = dict(_err_exprs())
    keys = [fam["div"], fam["ci"], fam["cf"], fam["cid"], fam["cdd"]]   # hasher types only: 7 key words
    used = {"num", "den", "ci", "cf", "cid", "cdd"}
    pred = et.filter()
    clean_cols, clean_batch = et.case()
    clean = q.MemoryTable.try_new(et.schema, [clean_batch])
    want_clean = _model_join(clean_cols, clean_cols, keys, pred, pred)
    assert len(want_clean) > 100
    for n, (pname, row, mode) in enumerate(_error_runs()):
        poison = next(p for name, p, _ in et.POISONS if name == pname)
        if not set(poison) <= used:
            continue
        cols, batch = et.case(pname, row, mode)
        dirty = q.MemoryTable.try_new(et.schema, [batch])
        # the poisoned table is the build side and the probe side in turn (non-raw and raw key kernels)
        for lt, rt, lc, rc in ((dirty, clean, cols, clean_cols), (clean, dirty, clean_cols, cols)):
            want = _model_join(lc, rc, keys, pred, pred)
            assert isinstance(want, str) == (mode == "live"), (pname, mode, want if isinstance(want, str) else None)
            if isinstance(want, str):
                with pytest.raises(q.QuriousError, match=M.MESSAGE[want]):
                    _run_join(et.schema, lt, rt, keys, pred, pred)
            else:
                assert _run_join(et.schema, lt, rt, keys, pred, pred) == want, (pname, mode)
