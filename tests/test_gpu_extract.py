"""GPU: EXTRACT(part FROM date / timestamp) inside every accelerated consumer, by substitution differential. The expected
result is the CPU oracle's execution of the same plan with every EXTRACT node replaced by a Column over an Int64 column that
pyarrow.compute precomputed (year / month / day / iso_week / hour / minute / second; Date64 through timestamp[ms]) and that is
appended to the input table; the HIP plan, which evaluates EXTRACT in its generated kernels, must give the same batches.
Inputs: Date32, Date64 and the four Timestamp units, ~5 % NULLs, pre-1970 values, values outside chrono's range (NULL
results), ragged batches and row counts that are not multiples of 64."""
import json
import os

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import qurious_amd as q
from qurious_amd import JoinType, Operator, exchange, synth
from qurious_amd import ScalarValue as S

from .helpers import rows_of, sorted_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = pa.int64()
PARTS = ["year", "month", "day", "hour", "minute", "second", "week"]
MIN_DAYS, MAX_DAYS = -96465658, 95026601   # chrono's NaiveDate range in days since 1970-01-01
ARGS = [("d32", pa.date32()), ("d64", pa.date64()), ("ts", pa.timestamp("s")), ("tms", pa.timestamp("ms")),
        ("tus", pa.timestamp("us")), ("tns", pa.timestamp("ns"))]
PER_SEC = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}


def _ints(batches):
    """rows with Date / Timestamp values as their integers (Python's datetime cannot hold the far ones)"""
    def plain(c):
        if pa.types.is_date32(c.type):
            return c.cast(pa.int32())
        return c.cast(I64) if pa.types.is_date64(c.type) or pa.types.is_timestamp(c.type) else c
    return rows_of([pa.RecordBatch.from_arrays([plain(c) for c in b.columns], names=b.schema.names) for b in batches])


def _batches_equal(got, want):
    assert [b.num_rows for b in got] == [b.num_rows for b in want]
    assert _ints(got) == _ints(want)
    for g, w in zip(got, want):
        assert [f.type for f in g.schema] == [f.type for f in w.schema]


def _per_day(t):
    return 86400 * PER_SEC["ms" if pa.types.is_date64(t) else t.unit] if not pa.types.is_date32(t) else 1


def expected(arr, part):
    """pyarrow's EXTRACT of `arr` as Int64; NULL where arr is NULL or outside chrono's range (Date32 time parts: 0)"""
    t = arr.type
    raw = np.array(arr.cast(pa.int32() if pa.types.is_date32(t) else I64).fill_null(0)).astype(np.int64)
    valid = np.array(arr.is_valid())
    if pa.types.is_date32(t) and part in ("hour", "minute", "second"):
        return pa.array(np.zeros(len(arr), dtype=np.int64), type=I64, mask=~valid)
    days = raw // _per_day(t)
    ok = valid & (days >= MIN_DAYS) & (days <= MAX_DAYS)
    safe = pa.array(np.where(ok, raw, 0), type=pa.int32() if pa.types.is_date32(t) else I64).cast(t)
    if pa.types.is_date64(t):
        safe = safe.cast(pa.timestamp("ms"))
    fn = {"year": pc.year, "month": pc.month, "day": pc.day, "week": pc.iso_week, "hour": pc.hour, "minute": pc.minute, "second": pc.second}[part]
    return pa.array(np.array(fn(safe)).astype(np.int64), type=I64, mask=~ok)


def _make(n, seed, year_lo=1, year_hi=9999, null_p=0.05):
    """one batch: the six argument columns, an Int64 payload `v` and a Utf8 key `s`"""
    rng = np.random.default_rng(seed)
    d0 = lambda y: (np.datetime64(f"{y:04d}-01-01") - np.datetime64("1970-01-01")).astype(np.int64)   # noqa: E731
    lo, hi = d0(year_lo), d0(year_hi + 1) if year_hi < 9999 else d0(9999) + 364
    cols, names = [], []
    for name, t in ARGS:
        pd = _per_day(t)
        dlo, dhi = (max(lo, -106751), min(hi, 106750)) if name == "tns" else (lo, hi)
        days = rng.integers(dlo, dhi, n)
        vals = days * pd + (rng.integers(0, pd, n) if pd > 1 else 0)
        if year_lo == 1 and name != "tns":
            # values just outside chrono's range, and the extremes of the storage type (pyarrow, the reference of these tests,
            # does not compute the parts of the range's own far ends: tests/test_extract_cpu.py checks those)
            far = np.array([MIN_DAYS - 1, MAX_DAYS + 1, MIN_DAYS - 1000, MAX_DAYS + 1000], dtype=np.int64) * pd
            far = np.concatenate([far, [-2**31, 2**31 - 1] if name == "d32" else [-2**63 + 1, 2**63 - 1]])
            vals[7::211][:len(far)] = far[:len(vals[7::211])]
        mask = rng.random(n) < null_p
        if name == "d32":
            cols.append(pa.array(vals.astype(np.int32), type=pa.int32(), mask=mask).cast(t))
        else:
            cols.append(pa.array(vals, type=I64, mask=mask).cast(t))
        names.append(name)
    cols.append(pa.array(rng.integers(-10**6, 10**6, n), type=I64, mask=rng.random(n) < null_p))
    cols.append(pa.array(["k%d" % v for v in rng.integers(0, 5, n)], type=pa.string(), mask=rng.random(n) < null_p))
    names += ["v", "s"]
    return pa.RecordBatch.from_arrays(cols, names=names)


class Sub:
    """Builds the HIP plan (EXTRACT) and the oracle plan (precomputed Int64 columns appended to the batch) side by side."""

    def __init__(self, batch):
        self.base = batch
        self.extra = []   # (arg column name, part)

    def col(self, name):
        return q.Column(name, self.base.schema.get_field_index(name))

    def x(self, part, name):
        """(EXTRACT(part FROM name), Column of its precomputed values)"""
        if (name, part) not in self.extra:
            self.extra.append((name, part))
        k = self.base.num_columns + self.extra.index((name, part))
        return q.Function(q.DatetimeExtract(), [q.Literal(S.Utf8(part.upper())), self.col(name)]), q.Column(f"x_{part}_{name}", k)

    def table(self):
        cols = list(self.base.columns) + [expected(self.base.column(nm), p) for nm, p in self.extra]
        names = self.base.schema.names + [f"x_{p}_{nm}" for nm, p in self.extra]
        return pa.RecordBatch.from_arrays(cols, names=names)


def _scan(batch, cuts, filter=None):
    cuts = [c for c in cuts if c <= batch.num_rows] + [batch.num_rows]
    batches = [batch.slice(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    return q.Scan(batch.schema, q.MemoryTable.try_new(batch.schema, batches), None, filter)


CUTS = [0, 63, 64, 1000, 1000, 1001, 4097, 9000]
N = 12_011


@pytest.fixture(scope="module")
def data():
    return _make(N, 7)


def test_projection_every_part_and_type(ctx, oracle, data):
    s = Sub(data)
    pairs = [s.x(p, nm) for nm, _ in ARGS for p in PARTS]
    tbl = s.table()
    scan = _scan(tbl, CUTS)
    for half in (pairs[:21], pairs[21:]):
        got = q.Projection(None, scan, [h for h, _ in half] + [s.col("v")]).execute()
        want = oracle.execute(q.Projection(None, scan, [w for _, w in half] + [s.col("v")]))
        _batches_equal(got, want)
    # a literal argument is folded on the host (tests/sql/basic_test.slt:35-39)
    with open(os.path.join(ROOT, "tests", "golden", "extract_vectors.json")) as f:
        g = json.load(f)
    day = q.CastExpr(q.Literal(S.Utf8(g["date"])), pa.date32())
    got = q.Projection(None, scan, [q.Function(q.DatetimeExtract(), [q.Literal(S.Utf8(p)), day]) for p in g["parts"]]).execute()
    want = oracle.execute(q.Projection(None, scan, [q.Literal(S.Int64(v)) for v in g["expected"]]))
    _batches_equal(got, want)
    assert rows_of(got)[0] == tuple(g["expected"])


def test_filter_and_fused_scan_filters(ctx, oracle, data):
    s = Sub(data)
    (y32, Y32), (m_us, M_US), (h_ns, H_NS), (w64, W64), (s_s, S_S) = (s.x("year", "d32"), s.x("month", "tus"), s.x("hour", "tns"),
                                                                     s.x("week", "d64"), s.x("second", "ts"))

    def pred(y, m, h, w, sec):
        a = q.BinaryExpr(q.BinaryExpr(y, Operator.Lt, q.Literal(S.Int64(1970))), Operator.And, q.BinaryExpr(m, Operator.LtEq, q.Literal(S.Int64(6))))
        b = q.BinaryExpr(q.BinaryExpr(h, Operator.Eq, q.Literal(S.Int64(3))), Operator.Or, q.BinaryExpr(w, Operator.Gt, sec))
        return q.BinaryExpr(a, Operator.Or, b)

    tbl = s.table()
    scan = _scan(tbl, CUTS)
    got = q.Filter(scan, pred(y32, m_us, h_ns, w64, s_s)).execute()
    want = oracle.execute(q.Filter(scan, pred(Y32, M_US, H_NS, W64, S_S)))
    _batches_equal(got, want)
    assert 0 < sum(b.num_rows for b in got) < N
    # ... fused into an aggregate (Scan with a pushed-down filter under HashAggregate)
    agg = lambda p: q.HashAggregate(None, _scan(tbl, CUTS, p), [s.col("s")], [q.SumAggregateExpr(s.col("v"), I64)])   # noqa: E731
    assert sorted_rows(agg(pred(y32, m_us, h_ns, w64, s_s)).execute()) == sorted_rows(oracle.execute(agg(pred(Y32, M_US, H_NS, W64, S_S))))
    # ... and into an Inner join's probe side
    left = _scan(tbl.select(["v", "s"]).slice(0, 300), [0, 100])
    join = lambda p: q.HashJoinExec.try_new(left, _scan(tbl, CUTS, p), JoinType.Inner, [(q.Column("s", 1), s.col("s"))], None)   # noqa: E731
    _batches_equal(join(q.BinaryExpr(m_us, Operator.Eq, q.Literal(S.Int64(2)))).execute(),
                   oracle.execute(join(q.BinaryExpr(M_US, Operator.Eq, q.Literal(S.Int64(2))))))


def test_group_by_and_aggregates(ctx, oracle, data):
    s = Sub(data)
    (y64, Y64), (d_s, D_S), (w32, W32), (sec_ms, SEC_MS), (mo_us, MO_US) = (s.x("year", "d64"), s.x("day", "ts"), s.x("week", "d32"),
                                                                           s.x("second", "tms"), s.x("month", "tus"))
    tbl = s.table()
    scan = _scan(tbl, CUTS)

    def plans(y, d, w, sec, mo):
        aggs = [q.SumAggregateExpr(d, I64), q.MinAggregateExpr(w, I64), q.MaxAggregateExpr(sec, I64), q.CountAggregateExpr(w)]
        return [q.HashAggregate(None, scan, [y], aggs),                        # EXTRACT alone as the key (many groups)
                q.HashAggregate(None, scan, [mo, s.col("s")], aggs),           # ... beside a Utf8 key
                q.NoGroupingAggregate(None, scan, aggs)]

    for g, w in zip(plans(y64, d_s, w32, sec_ms, mo_us), plans(Y64, D_S, W32, SEC_MS, MO_US)):
        got, want = g.execute(), oracle.execute(w)
        assert sorted_rows(got) == sorted_rows(want)
        assert [f.type for f in got[0].schema] == [f.type for f in want[0].schema]
    assert len(rows_of(plans(y64, d_s, w32, sec_ms, mo_us)[0].execute())) > 1000


@pytest.mark.parametrize("jt", list(JoinType))
def test_join_keys_on_both_sides(ctx, oracle, jt):
    lb, rb = _make(1500, 21, 1950, 2049), _make(2501, 22, 1950, 2049)
    ls, rs = Sub(lb), Sub(rb)
    (kl, KL), (kr, KR) = ls.x("year", "d32"), rs.x("year", "tms")
    lt, rt = ls.table(), rs.table()
    left, right = _scan(lt, [0, 700]), _scan(rt, [0, 64, 64, 1300])
    got = q.HashJoinExec.try_new(left, right, jt, [(kl, kr)], None).execute()
    want = oracle.execute(q.HashJoinExec.try_new(left, right, jt, [(KL, KR)], None))
    _batches_equal(got, want)
    assert sum(b.num_rows for b in got) > 0


def test_order_by_desc_with_limit(ctx, oracle, data):
    s = Sub(data)
    (w, W), (y, Y) = s.x("week", "tns"), s.x("year", "ts")
    scan = _scan(s.table(), CUTS)
    for nulls_first in (True, False):
        opts = q.SortOptions(descending=True, nulls_first=nulls_first)
        got = q.Sort([q.PhysicalSortExpr(w, opts), q.PhysicalSortExpr(y, opts)], scan, 150).execute()
        want = oracle.execute(q.Sort([q.PhysicalSortExpr(W, opts), q.PhysicalSortExpr(Y, opts)], scan, 150))
        _batches_equal(got, want)


def test_partition_by_extract_key(ctx, oracle, data):
    s = Sub(data)
    (m, _), (d, _) = s.x("month", "d64"), s.x("day", "tus")
    tbl = s.table()
    dev = _scan(tbl, CUTS).execute_device()
    n_parts = 8
    parts = exchange.partition_filtered(dev, [m, d], n_parts)
    pid = oracle.partition_ids([tbl.column("x_month_d64"), tbl.column("x_day_tus")], n_parts)
    for p, part in enumerate(parts):
        want = tbl.filter(pa.array(pid == p))
        assert part.num_rows == want.num_rows
        assert _ints(part.to_batches()) == _ints([want])
    assert sum(p.num_rows for p in parts) == N


def test_q9_shaped_pipeline(ctx, oracle):
    """orders |><| lineitem, project EXTRACT(YEAR FROM o_orderdate) AS o_year and the revenue, GROUP BY o_year, ORDER BY
    o_year DESC: three executions, all equal to the substituted oracle plan"""
    _, orders, lineitem = synth.q3_tables(0.01)
    o_sch = synth.ORDERS_SCHEMA.append(pa.field("o_year", I64))
    orders_x = [pa.RecordBatch.from_arrays(list(b.columns) + [expected(b.column("o_orderdate"), "year")], schema=o_sch) for b in orders]
    o = q.Scan(o_sch, q.MemoryTable.try_new(o_sch, orders_x), None, None)
    li = q.Scan(synth.LINEITEM_Q3_SCHEMA, q.MemoryTable.try_new(synth.LINEITEM_Q3_SCHEMA, lineitem), None, None)
    join = q.HashJoinExec.try_new(o, li, JoinType.Inner, [(q.Column("o_orderkey", 0), q.Column("l_orderkey", 0))], None)
    one = q.CastExpr(q.Literal(S.Int64(1)), pa.decimal128(20, 0))
    revenue = q.BinaryExpr(q.Column("l_extendedprice", 7), Operator.Mul, q.BinaryExpr(one, Operator.Sub, q.Column("l_discount", 8)))

    t4 = pa.decimal128(38, 4)

    def plan(year):
        proj = q.Projection(pa.schema([pa.field("o_year", I64), pa.field("revenue", t4)]), join, [year, revenue])
        agg = q.HashAggregate(pa.schema([pa.field("o_year", I64), pa.field("SUM(revenue)", t4)]), proj, [q.Column("o_year", 0)],
                              [q.SumAggregateExpr(q.Column("revenue", 1), t4)])
        return q.Sort([q.PhysicalSortExpr(q.Column("o_year", 0), q.SortOptions(descending=True, nulls_first=False))], agg)

    hip = plan(q.Function(q.DatetimeExtract(), [q.Literal(S.Utf8("YEAR")), q.Column("o_orderdate", 2)]))
    want = oracle.execute(plan(q.Column("o_year", 4)))
    runs = [hip.execute() for _ in range(3)]
    for got in runs:
        _batches_equal(got, want)
    assert len(rows_of(want)) >= 5
