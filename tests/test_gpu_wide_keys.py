"""GROUP BY on keys of any width: a key that does not fit the packed 8 key words (a Utf8 value of more than 55 bytes, many
columns) is encoded to one 32-bit group code per row in front of the aggregate (csrc/agg.cpp maybe_encode_wide_key,
csrc/device/qhip_widekey.inc), the way the reference hashes keys of any length and any number of columns
(utils/array.rs:171-210). The switch is QHIP_AGG_WIDE_KEYS (0 off — the default —, 1 when the key does not fit, 2 every grouped
aggregate over plain key columns); every test sets it with monkeypatch.

The model of every comparison is a Python dict over the rows' key tuples (exact ints and Decimals, None its own value per
column). The CPU oracle is used in addition where at most one key column is nullable: the reference merges (NULL, x) with
(x, NULL)."""
import datetime
import decimal

import numpy as np
import pyarrow as pa
import pytest

import qurious_amd as q
from qurious_amd import JoinType, Operator
from tests.helpers import col, lit_i64, rows_of, table_scan

pytestmark = pytest.mark.gpu

I64 = pa.int64()
DEC = pa.decimal128(15, 2)


def _model(rows, n_keys, aggs, keep=None):
    """rows: tuples (keys ..., arguments ...); aggs: ("sum" | "min" | "max", index into the row) or ("count",) = COUNT(1)."""
    groups = {}
    for r in rows:
        if keep is not None and not keep(r):
            continue
        groups.setdefault(tuple(r[:n_keys]), []).append(r)
    out = []
    for key, rs in groups.items():
        vals = []
        for a in aggs:
            if a[0] == "count":
                vals.append(len(rs))
                continue
            xs = [r[a[1]] for r in rs if r[a[1]] is not None]
            vals.append(None if not xs else sum(xs) if a[0] == "sum" else min(xs) if a[0] == "min" else max(xs))
        out.append(key + tuple(vals))
    return sorted(out, key=repr)


def _got(plan):
    return sorted(rows_of(plan.execute()), key=repr)


def _batch(schema, rows):
    cols = list(zip(*rows)) if rows else [[] for _ in schema]
    return pa.RecordBatch.from_arrays([pa.array(list(c), type=f.type) for c, f in zip(cols, schema)], schema=schema)


def _ragged(batch, cuts):
    edges = [0] + [c for c in cuts if c < batch.num_rows] + [batch.num_rows]
    return [batch.slice(a, b - a) for a, b in zip(edges, edges[1:])]


# ---------------------------------------------------------------- TPC-H Q10's GROUP BY
Q10_SCHEMA = pa.schema([pa.field("c_custkey", I64), pa.field("c_name", pa.string()), pa.field("c_acctbal", DEC), pa.field("c_phone", pa.string()),
                        pa.field("n_name", pa.string()), pa.field("c_address", pa.string()), pa.field("c_comment", pa.string()),
                        pa.field("revenue", DEC), pa.field("qty", I64)])


def _q10_rows(n, n_keys, seed):
    """n rows over n_keys distinct keys. Three keys in a row share the first six columns and the comment's first 100 or so bytes:
    they differ in the comment's last characters only."""
    rng = np.random.default_rng(seed)
    nations = ["ALGERIA", "UNITED KINGDOM", "SAUDI ARABIA", "UNITED STATES", "MOZAMBIQUE", "RUSSIAN FEDERATION" + " " * 7]
    words = ["quickly", "ironic", "déposits", "blithely", "über", "furiously", "señor", "pending", "日本", "requests"]
    keys = []
    for g in range(n_keys):
        c = g // 3
        comment = " ".join(words[(c * 7 + j * 3) % len(words)] for j in range(40))
        while len(comment.encode()) > 113:
            comment = comment[:-1]
        comment += ["", "é", "zz"][g % 3] + "."
        assert len(comment.encode()) <= 117
        address = ("%d Long Street, Springfield, Block %d" % (c, c % 97))[:40]
        keys.append((c, "Customer#%09d" % c, decimal.Decimal(c * 37 % 100000 - 5000).scaleb(-2), "%02d-%03d-%03d-%04d" % (c % 25 + 10, c % 1000, c * 7 % 1000, c % 10000),
                     nations[c % len(nations)], address, comment))
    assert len(set(keys)) == n_keys and max(len(k[6].encode()) for k in keys) > 100 and all(len(k[3]) == 15 for k in keys)
    pick = rng.integers(0, n_keys, n)
    rev = rng.integers(-100000, 1000000, n)
    qty = rng.integers(1, 51, n)
    return [keys[int(pick[i])] + (decimal.Decimal(int(rev[i])).scaleb(-2), int(qty[i])) for i in range(n)]


Q10_KEYS = [col(f.name, k) for k, f in enumerate(Q10_SCHEMA)][:7]
Q10_AGGS = [q.SumAggregateExpr(col("revenue", 7), DEC), q.CountAggregateExpr(lit_i64(1)), q.MinAggregateExpr(col("qty", 8), I64),
            q.MaxAggregateExpr(col("qty", 8), I64)]
Q10_MODEL_AGGS = [("sum", 7), ("count",), ("min", 8), ("max", 8)]


@pytest.fixture(scope="module")
def q10():
    rows = _q10_rows(30000, 3000, 10)
    return rows, _ragged(_batch(Q10_SCHEMA, rows), [7000, 7001, 19000, 29999])


@pytest.mark.parametrize("with_predicate", [False, True])
def test_q10_shaped_group_by(ctx, oracle, monkeypatch, q10, with_predicate):
    rows, batches = q10
    pred = q.BinaryExpr(col("qty", 8), Operator.Gt, lit_i64(20)) if with_predicate else None
    plan = q.HashAggregate(None, table_scan(Q10_SCHEMA, batches, filter=pred), Q10_KEYS, Q10_AGGS)   # (the Scan's filter is fused into the aggregate)
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "0")
    with pytest.raises(q.UnsupportedError):
        plan.execute()
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "1")
    before = ctx.wide_key_aggregates()
    got = _got(plan)
    assert ctx.wide_key_aggregates() == before + 1
    want = _model(rows, 7, Q10_MODEL_AGGS, keep=(lambda r: r[8] > 20) if with_predicate else None)
    assert len(want) > 2900
    assert got == want
    assert got == sorted(rows_of(oracle.execute(plan)), key=repr)


# ---------------------------------------------------------------- long values that differ late
def _late_values():
    base = "".join(chr(ord("A") + k % 23) for k in range(300))
    vals = ["", base]
    for n in (56, 57, 63, 64, 65, 71, 72, 73, 117, 128, 255, 256, 299):
        vals.append(base[:n])                                            # differs in length only
        vals.append(base[:n - 1] + "?")                                  # ... in the last byte
        for at in range(8, n, 8):                                        # ... on either side of every 8-byte boundary
            vals.append(base[:at] + "#" + base[at + 1:n])
            vals.append(base[:at - 1] + "#" + base[at:n])
    assert len(set(vals)) == len(vals) and max(map(len, vals)) == 300
    return vals


def test_long_keys_that_differ_late(ctx, oracle, monkeypatch):
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "1")
    rng = np.random.default_rng(21)
    vals = _late_values()
    n = 3 * len(vals) + 11
    pick = rng.integers(0, len(vals), n)
    null = rng.random(n) < 0.05
    rows = [(None if null[i] else vals[int(pick[i])], int(rng.integers(-1000, 1000))) for i in range(n)]
    rows += [(v, 1) for v in vals]   # (every value at least once)
    schema = pa.schema([pa.field("s", pa.string()), pa.field("v", I64)])
    plan = q.HashAggregate(None, table_scan(schema, _ragged(_batch(schema, rows), [100, 163, 1000])), [col("s", 0)],
                           [q.SumAggregateExpr(col("v", 1), I64), q.CountAggregateExpr(lit_i64(1))])
    want = _model(rows, 1, [("sum", 1), ("count",)])
    assert len(want) == len(vals) + 1
    for call in range(2):   # (the second call runs with what the first learnt about the plan)
        before = ctx.wide_key_aggregates()
        assert _got(plan) == want
        assert ctx.wide_key_aggregates() == before + 1
    assert sorted(rows_of(oracle.execute(plan)), key=repr) == want


# ---------------------------------------------------------------- many key columns
def _int_key_plan(n_keys, n_rows, seed, computed=None):
    rng = np.random.default_rng(seed)
    schema = pa.schema([pa.field("k%d" % k, I64) for k in range(n_keys)] + [pa.field("v", I64)])
    base = rng.integers(0, 3, (40, n_keys))   # 40 keys or fewer
    pick = rng.integers(0, 40, n_rows)
    rows = [tuple(int(x) for x in base[int(pick[i])]) + (int(rng.integers(0, 100)),) for i in range(n_rows)]
    keys = [col("k%d" % k, k) for k in range(n_keys)]
    if computed is not None:
        keys[computed] = q.BinaryExpr(keys[computed], Operator.Add, lit_i64(0))
    plan = q.HashAggregate(None, table_scan(schema, _ragged(_batch(schema, rows), [333])), keys, [q.SumAggregateExpr(col("v", n_keys), I64), q.CountAggregateExpr(lit_i64(1))])
    return plan, _model(rows, n_keys, [("sum", n_keys), ("count",)])


@pytest.mark.parametrize("n_keys", [9, 32])
def test_many_key_columns(ctx, oracle, monkeypatch, n_keys):
    plan, want = _int_key_plan(n_keys, 1000, n_keys)
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "0")
    with pytest.raises(q.UnsupportedError, match="wider than 8 words"):
        plan.execute()
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "1")
    assert _got(plan) == want
    assert sorted(rows_of(oracle.execute(plan)), key=repr) == want


def test_more_than_32_key_columns_and_computed_keys_stay_unsupported(ctx, monkeypatch):
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "1")
    plan, _ = _int_key_plan(33, 100, 33)
    with pytest.raises(q.UnsupportedError, match="more than 32 columns"):
        plan.execute()
    plan, _ = _int_key_plan(9, 100, 34, computed=4)
    before = ctx.wide_key_aggregates()
    with pytest.raises(q.UnsupportedError, match="wider than 8 words.*computed key expressions are not encoded"):
        plan.execute()
    assert ctx.wide_key_aggregates() == before


# ---------------------------------------------------------------- several nullable key columns
def test_several_nullable_key_columns(ctx, monkeypatch):
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "1")
    rng = np.random.default_rng(5)
    long = "a wide value of more than fifty-five bytes, the same in every row that has one"
    assert len(long) > 55
    rows = [(None, 5, long, 1), (5, None, long, 2), (None, 5, long, 4), (5, None, None, 8), (None, None, None, 16), (None, None, long, 32), (5, 5, long, 64),
            (None, None, None, 128), (0, None, long, 256), (None, 0, long, 512), (0, 0, "", 1024), (0, 0, None, 2048)]
    for _ in range(500):
        rows.append((None if rng.random() < 0.3 else int(rng.integers(0, 3)), None if rng.random() < 0.3 else int(rng.integers(0, 3)),
                     None if rng.random() < 0.3 else long[:int(rng.integers(56, len(long) + 1))], int(rng.integers(0, 10))))
    schema = pa.schema([pa.field("a", I64), pa.field("b", I64), pa.field("s", pa.string()), pa.field("v", I64)])
    plan = q.HashAggregate(None, table_scan(schema, _ragged(_batch(schema, rows), [5, 200])), [col("a", 0), col("b", 1), col("s", 2)],
                           [q.SumAggregateExpr(col("v", 3), I64), q.CountAggregateExpr(lit_i64(1))])
    got, want = _got(plan), _model(rows, 3, [("sum", 3), ("count",)])
    assert got == want
    assert (None, 5, long, 5, 2) in got and (5, None, long, 2, 1) in got   # (NULL, 5) and (5, NULL) stay two groups


# ---------------------------------------------------------------- row counts
WIDE = "%04d: sixty bytes and more of a value that only differs in its first four characters"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_row_counts(ctx, oracle, monkeypatch, n):
    schema = pa.schema([pa.field("s", pa.string()), pa.field("v", I64)])
    aggs = [q.SumAggregateExpr(col("v", 1), I64), q.CountAggregateExpr(lit_i64(1))]
    for what in ("one group", "every row its own group"):
        rows = [(WIDE % (0 if what == "one group" else i), i) for i in range(n)]
        plan = q.HashAggregate(None, table_scan(schema, _ragged(_batch(schema, rows), [64])), [col("s", 0)], aggs)
        monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "1")
        out = plan.execute()
        want = _model(rows, 1, [("sum", 1), ("count",)])
        assert len(want) == (0 if n == 0 else 1 if what == "one group" else n)
        assert sorted(rows_of(out), key=repr) == want, what
        if n in (0, 65):
            assert sorted(rows_of(oracle.execute(plan)), key=repr) == want
        if n == 0:   # no rows, and no batches at all: the batches a key that fits gives today
            narrow = q.HashAggregate(None, table_scan(schema, [_batch(schema, [])]), [col("v", 1)], aggs)
            monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "0")
            assert [b.num_rows for b in out] == [b.num_rows for b in narrow.execute()]
            none = q.Scan(schema, q.MemoryTable.try_new(schema, []), None, None)
            narrow_none = q.HashAggregate(None, none, [col("v", 1)], aggs).execute()
            monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "2")
            before = ctx.wide_key_aggregates()
            assert [b.num_rows for b in q.HashAggregate(None, none, [col("s", 0)], aggs).execute()] == [b.num_rows for b in narrow_none]
            assert ctx.wide_key_aggregates() == before + 1


# ---------------------------------------------------------------- colliding hashes
def test_colliding_hashes(ctx, monkeypatch):
    """QHIP_AGG_WIDE_KEY_HASH_BITS=3 leaves the encoding 8 hash values: 300 keys share 8 start slots and one tag, so every probe
    walks a long chain of equal tags on different keys."""
    rng = np.random.default_rng(8)
    keys = [(WIDE % (g % 150), g // 150, None if g % 7 == 0 else "x" * (g % 5)) for g in range(300)]
    pick = rng.integers(0, 300, 5000)
    rows = [keys[int(pick[i])] + (int(rng.integers(0, 1000)),) for i in range(5000)]
    schema = pa.schema([pa.field("s", pa.string()), pa.field("k", I64), pa.field("t", pa.string()), pa.field("v", I64)])
    plan = q.HashAggregate(None, table_scan(schema, _ragged(_batch(schema, rows), [1000, 1001])), [col("s", 0), col("k", 1), col("t", 2)],
                           [q.SumAggregateExpr(col("v", 3), I64), q.CountAggregateExpr(lit_i64(1)), q.MaxAggregateExpr(col("v", 3), I64)])
    want = _model(rows, 3, [("sum", 3), ("count",), ("max", 3)])
    assert len(want) == 300
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "1")
    plain = _got(plan)
    monkeypatch.setenv("QHIP_AGG_WIDE_KEY_HASH_BITS", "3")
    assert _got(plan) == plain == want


# ---------------------------------------------------------------- mode 2: keys that fit
def _mode_results(monkeypatch, ctx, plan, stage_runs):
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "0")
    ordinary = _got(plan)
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "2")
    before = ctx.wide_key_aggregates()
    forced = [_got(plan), _got(plan)]   # (twice: a join below leaves its size on the device the second time)
    assert ctx.wide_key_aggregates() == before + (2 if stage_runs else 0)
    assert forced[0] == forced[1] == ordinary
    return ordinary


def test_mode_2_one_int64_key_over_a_filter_output(ctx, oracle, monkeypatch):
    rng = np.random.default_rng(12)
    n = 20000
    rows = [(int(rng.integers(0, 700)) if rng.random() > 0.03 else None, int(rng.integers(0, 100)), int(rng.integers(-50, 50))) for _ in range(n)]
    schema = pa.schema([pa.field("k", I64), pa.field("f", I64), pa.field("v", I64)])
    scan = table_scan(schema, _ragged(_batch(schema, rows), [4096, 4100]))
    # (two Filters: the aggregate fuses one Filter over a Scan into its kernel, the second one's OUTPUT is its input)
    filtered = q.Filter(q.Filter(scan, q.BinaryExpr(col("f", 1), Operator.Lt, lit_i64(80))), q.BinaryExpr(col("f", 1), Operator.GtEq, lit_i64(10)))
    aggs = [q.SumAggregateExpr(col("v", 2), I64), q.CountAggregateExpr(lit_i64(1)), q.MinAggregateExpr(col("v", 2), I64)]
    plan = q.HashAggregate(None, filtered, [col("k", 0)], aggs)
    want = _model(rows, 1, [("sum", 2), ("count",), ("min", 2)], keep=lambda r: 10 <= r[1] < 80)
    assert _mode_results(monkeypatch, ctx, plan, True) == want
    assert sorted(rows_of(oracle.execute(plan)), key=repr) == want
    # a computed key takes the ordinary path, silently
    computed = q.HashAggregate(None, filtered, [q.BinaryExpr(col("k", 0), Operator.Add, lit_i64(1))], aggs)
    want1 = _model([(None if r[0] is None else r[0] + 1,) + r[1:] for r in rows], 1, [("sum", 2), ("count",), ("min", 2)], keep=lambda r: 10 <= r[1] < 80)
    assert _mode_results(monkeypatch, ctx, computed, False) == want1


def test_mode_2_utf8_and_date_key_over_a_join_output(ctx, oracle, monkeypatch):
    rng = np.random.default_rng(13)
    dims = [(i, None if i % 11 == 0 else "segment %d" % (i % 9)) for i in range(200)]
    day0 = datetime.date(1995, 1, 1)
    facts = [(int(rng.integers(0, 260)), day0 + datetime.timedelta(days=int(rng.integers(0, 6))), int(rng.integers(0, 1000))) for _ in range(20000)]
    ds = pa.schema([pa.field("id", I64), pa.field("seg", pa.string())])
    fs = pa.schema([pa.field("fid", I64), pa.field("day", pa.date32()), pa.field("v", I64)])
    join = q.HashJoinExec.try_new(table_scan(ds, [_batch(ds, dims)]), table_scan(fs, _ragged(_batch(fs, facts), [5000, 12345])), JoinType.Inner,
                                  [(col("id", 0), col("fid", 0))], None)
    plan = q.HashAggregate(None, join, [col("seg", 1), col("day", 3)], [q.SumAggregateExpr(col("v", 4), I64), q.CountAggregateExpr(lit_i64(1))])
    seg = dict(dims)
    joined = [(seg[f[0]], f[1], f[2]) for f in facts if f[0] in seg]
    want = _model(joined, 2, [("sum", 2), ("count",)])
    assert len(want) == 60
    assert _mode_results(monkeypatch, ctx, plan, True) == want
    assert sorted(rows_of(oracle.execute(plan)), key=repr) == want


# ---------------------------------------------------------------- downstream of the stage
def test_sort_limit_and_arrow_round_trip_over_the_gathered_keys(ctx, monkeypatch, q10):
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "1")
    rows, batches = q10
    agg = q.HashAggregate(None, table_scan(Q10_SCHEMA, batches), Q10_KEYS, Q10_AGGS)
    want = _model(rows, 7, Q10_MODEL_AGGS)
    # ORDER BY revenue DESC, c_comment, c_custkey LIMIT 20 (Q10's tail), read from the gathered key columns on the device
    order = [q.PhysicalSortExpr(col("revenue", 7), q.SortOptions(True, False)), q.PhysicalSortExpr(col("c_comment", 6), q.SortOptions(False, True)),
             q.PhysicalSortExpr(col("c_custkey", 0), q.SortOptions(False, True))]
    top = rows_of(q.Limit(q.Sort(order, agg), 20, 0).execute())
    assert top == sorted(want, key=lambda r: (-r[7], r[6].encode(), r[0]))[:20]
    # the exported result, ingested again and grouped by the same keys: every group once, with the values it went out with
    out = agg.execute()
    out_schema = pa.schema([pa.field(f.name, f.type) for f in Q10_SCHEMA][:7] + [pa.field("revenue", DEC), pa.field("n", I64), pa.field("lo", I64), pa.field("hi", I64)])
    again = [pa.RecordBatch.from_arrays(b.columns, schema=out_schema) for b in out]
    back = q.HashAggregate(None, table_scan(out_schema, again), Q10_KEYS,
                           [q.SumAggregateExpr(col("revenue", 7), DEC), q.SumAggregateExpr(col("n", 8), I64), q.MinAggregateExpr(col("lo", 9), I64), q.MaxAggregateExpr(col("hi", 10), I64)])
    assert _got(back) == want
