"""GPU parity of the SORTED form of the dense join build (csrc/join.cpp, qh_join_dense_build_sorted_body): a build side whose
key column is strictly ascending stores every bitmap word once with plain stores — rank form (rank[w] instead of row_of[])
when every build row is inserted, row_of form under a fused scan filter. The kernel verifies the order itself; a build side
found out of order (or with NULL keys) runs again with the atomic build and is remembered. Every result is compared with the
CPU oracle, with the form chosen automatically (QHIP_JOIN_DENSE_SORTED=1), always tried (2) and switched off (0)."""
import numpy as np
import pyarrow as pa
import pytest

import qurious_amd as q
from qurious_amd import JoinType, Operator
from qurious_amd import ScalarValue as S

from qurious_amd.exchange import column_ascending, sorted_build_counts

from .helpers import col, rows_of, table_scan

pytestmark = pytest.mark.gpu
I64 = pa.int64()
LS = pa.schema([pa.field("bk", I64), pa.field("bv", I64)])
RS = pa.schema([pa.field("pk", I64), pa.field("pv", I64)])
ROWS_PER_WG = 1024   # build rows one workgroup of the sorted build owns (QH_SORTED_ROWS)


def _same(got, want):
    assert [b.num_rows for b in got] == [b.num_rows for b in want]
    assert rows_of(got) == rows_of(want)


@pytest.fixture(params=["0", "1", "2"])
def sorted_mode(request, monkeypatch):
    monkeypatch.setenv("QHIP_JOIN_DENSE", "2")
    monkeypatch.setenv("QHIP_JOIN_DENSE_SORTED", request.param)
    return request.param


def _table(schema, keys, mask=None, batch=None, vals=None):
    keys = np.asarray(keys, dtype=np.int64)
    vals = np.arange(len(keys)) if vals is None else vals
    rb = pa.RecordBatch.from_arrays([pa.array(keys, I64, mask=mask), pa.array(vals, I64)], schema=schema)
    if batch is None or len(keys) == 0:
        return table_scan(schema, [rb])
    return table_scan(schema, [rb.slice(a, batch) for a in range(0, len(keys), batch)])


def _probe(rng, lo, hi, n, hits=None):
    span = hi - lo + 1
    pk = rng.integers(lo - span // 8 - 3, hi + span // 8 + 3, n, endpoint=True)
    if hits is not None:
        pk[: len(hits)] = hits
        rng.shuffle(pk)
    return _table(RS, pk, batch=40_000)


def _check_all(oracle, left, right, repeat=2):
    for jt in JoinType:
        plan = q.HashJoinExec.try_new(left, right, jt, [(col("bk", 0), col("pk", 0))], None)
        want = oracle.execute(plan)
        for _ in range(repeat):
            _same(plan.execute(), want)


@pytest.mark.parametrize("shape", ["dense", "sparse", "wide_gaps", "at_kmin_kmax", "one_row", "range_end", "range_end_plus_one"])
def test_sorted_dense_build_shapes_every_join_type(ctx, oracle, sorted_mode, shape):
    rng = np.random.default_rng(len(shape) * 7 + 1)
    if shape == "dense":
        keys = np.arange(1, 30_001)
    elif shape == "sparse":            # TPC-H's order keys: 8 of every 32 values
        n = np.arange(40_000)
        keys = (n // 8) * 32 + n % 8 + 1
    elif shape == "wide_gaps":         # gaps far wider than one workgroup's word range (1024 rows ~ 32 words when dense)
        keys = np.concatenate([np.arange(0, 3000), 3000 + 200_000 + np.arange(500), [900_000, 900_001], 2_000_000 + np.arange(3000) * 3])
    elif shape == "at_kmin_kmax":      # keys at the ends of the range, the probe hits both ends
        keys = np.concatenate([[-(2 ** 40)], np.arange(-(2 ** 40) + 5, -(2 ** 40) + 20_000, 7), [-(2 ** 40) + 60_000]])
    elif shape == "one_row":
        keys = np.array([123_456_789])
    elif shape == "range_end":         # the row count ends exactly at a workgroup's range
        keys = np.arange(3 * ROWS_PER_WG) * 5 + 11
    else:
        keys = np.arange(3 * ROWS_PER_WG + 1) * 33 + 11   # one row past it, a word per key
    left = _table(LS, keys, batch=7000)
    right = _probe(rng, int(keys.min()), int(keys.max()), 120_000, hits=np.concatenate([keys[:50], keys[-50:], [keys.min(), keys.max()]]))
    ctx.forget_plans()   # (a build side remembered as unsuitable by another parametrisation would not launch the kernel)
    launched, _ = sorted_build_counts(ctx)
    _check_all(oracle, left, right)
    # the sorted kernel ran (automatic mode: the key column is a base column in key order) — or, switched off, never
    now, fallbacks = sorted_build_counts(ctx)
    assert (now > launched) == (sorted_mode != "0"), (shape, now, launched)


def test_sorted_dense_build_row_of_form_under_a_fused_scan_filter(ctx, oracle, sorted_mode):
    """the build rows the filter rejects keep their row_of entries and set no bit"""
    n = np.arange(50_000)
    keys = (n // 8) * 32 + n % 8 + 1
    rng = np.random.default_rng(5)
    vals = rng.integers(0, 5, len(keys))
    lb = pa.RecordBatch.from_arrays([pa.array(keys, I64), pa.array(vals, I64)], schema=LS)
    pred = q.BinaryExpr(col("bv", 1), Operator.Eq, q.Literal(S.Int64(2)))
    left = table_scan(LS, [lb.slice(0, 20_000), lb.slice(20_000, 30_000)], pred)
    right = _probe(rng, 1, int(keys.max()), 200_000)
    plan = q.HashJoinExec.try_new(left, right, JoinType.Inner, [(col("bk", 0), col("pk", 0))], None)
    want = oracle.execute(plan)
    for _ in range(2):
        _same(plan.execute(), want)


def test_sorted_dense_build_null_keys_and_duplicates_fall_back(ctx, oracle, sorted_mode):
    rng = np.random.default_rng(9)
    keys = np.arange(10_000) * 3
    mask = np.zeros(len(keys), dtype=bool)
    mask[[0, 17, 5000, 9999]] = True
    right = _probe(rng, 0, int(keys.max()), 60_000)
    _check_all(oracle, _table(LS, keys, mask=mask, batch=4000), right)
    # adjacent duplicates: the CSR layout with today's (ascending-chain) results
    dup = np.sort(np.concatenate([keys, [300, 301, 29_997]]))
    _check_all(oracle, _table(LS, dup, batch=4000), right)
    assert ctx.last_stats()["main_kernel_name"] in ("qk_join_probe", "qk_join_probe_onetable")


@pytest.mark.parametrize("where", ["inside", "boundary"])
def test_sorted_dense_build_detects_a_descent_and_runs_again_once(ctx, oracle, monkeypatch, where):
    """ascending except for ONE descent (inside a workgroup's range / at a range boundary): with the sorted form always tried
    the kernel reports it, the join runs again with the atomic build, and the build side is remembered — the next execution
    of the same plan waits for the device exactly as often as an ascending build side does"""
    monkeypatch.setenv("QHIP_JOIN_DENSE", "2")
    monkeypatch.setenv("QHIP_JOIN_DENSE_SORTED", "2")
    keys = np.arange(5 * ROWS_PER_WG) * 4 + 1
    at = 2 * ROWS_PER_WG + 100 if where == "inside" else 2 * ROWS_PER_WG - 1
    keys[at], keys[at + 1] = keys[at + 1], keys[at]
    rng = np.random.default_rng(at)
    right = _probe(rng, 1, int(keys.max()), 80_000)
    ordered = _table(LS, np.sort(keys)[:-1], batch=3000)   # (one row fewer: a build side of its own, not the remembered one)
    ctx.forget_plans()
    for k, jt in enumerate((JoinType.Inner, JoinType.Left, JoinType.LeftAnti)):
        left = _table(LS, keys, batch=3000)
        plan = q.HashJoinExec.try_new(left, right, jt, [(col("bk", 0), col("pk", 0))], None)
        want = oracle.execute(plan)
        _, fb0 = sorted_build_counts(ctx)
        before = ctx.sync_count()
        _same(plan.execute(), want)          # detected, run again (the first join type; then the build side is remembered)
        first = ctx.sync_count() - before
        _, fb1 = sorted_build_counts(ctx)
        assert fb1 - fb0 == (1 if k == 0 else 0), (jt, fb0, fb1)
        before = ctx.sync_count()
        _same(plan.execute(), want)          # remembered: no second attempt
        once = ctx.sync_count() - before
        assert sorted_build_counts(ctx)[1] == fb1
        if k == 0:
            assert first > once, (first, once)
        plan_ok = q.HashJoinExec.try_new(ordered, right, jt, [(col("bk", 0), col("pk", 0))], None)
        _same(plan_ok.execute(), oracle.execute(plan_ok))
        before = ctx.sync_count()
        plan_ok.execute()
        assert once == ctx.sync_count() - before, jt


def test_sorted_dense_build_side_of_deferred_size(ctx, oracle, sorted_mode):
    """Q3's second join: the build side is an Inner join's output of deferred size (the kernel reads the row count on the
    device; the pad rows behind it repeat row 0 and take no part) whose key reaches the base column through the join's
    probe-side index vector, ascending"""
    rng = np.random.default_rng(77)
    na, nbb, nc = 30_000, 250_000, 800_000
    a_s = pa.schema([pa.field("ak", I64), pa.field("av", I64)])
    b_s = pa.schema([pa.field("bk", I64), pa.field("b_ak", I64), pa.field("bd", I64)])
    c_s = pa.schema([pa.field("c_bk", I64), pa.field("cv", I64)])
    A = pa.RecordBatch.from_arrays([pa.array(np.arange(1, na + 1), I64), pa.array(rng.integers(0, 5, na), I64)], schema=a_s)
    Bk = (np.arange(nbb) // 8) * 32 + np.arange(nbb) % 8 + 1
    B = pa.RecordBatch.from_arrays([pa.array(Bk, I64), pa.array(rng.integers(1, na * 2, nbb), I64), pa.array(rng.integers(0, 7, nbb), I64)], schema=b_s)
    Ck = np.sort(Bk[rng.integers(0, nbb, nc)])
    C = pa.RecordBatch.from_arrays([pa.array(Ck, I64), pa.array(rng.integers(0, 1000, nc), I64)], schema=c_s)
    apred = q.BinaryExpr(col("av", 1), Operator.Eq, q.Literal(S.Int64(2)))
    ta = table_scan(a_s, [A], apred)
    tb = table_scan(b_s, [B.slice(k, 60_000) for k in range(0, nbb, 60_000)])
    tc = table_scan(c_s, [C.slice(k, 300_000) for k in range(0, nc, 300_000)])
    want = None
    for execution in range(4):
        j1 = q.HashJoinExec.try_new(ta, tb, JoinType.Inner, [(col("ak", 0), col("b_ak", 1))], None)
        j2 = q.HashJoinExec.try_new(j1, tc, JoinType.Inner, [(col("bk", 2), col("c_bk", 0))], None)
        agg = q.HashAggregate(pa.schema([pa.field("bd", I64), pa.field("n", I64), pa.field("s", I64)]), j2, [col("bd", 4)],
                              [q.CountAggregateExpr(q.Literal(S.Int64(1))), q.SumAggregateExpr(col("cv", 6), I64)])
        if want is None:
            want = sorted(rows_of(oracle.execute(agg)))
        assert sorted(rows_of(agg.execute())) == want, execution
    before = ctx.sync_count()
    agg.execute_device()
    assert ctx.sync_count() - before == 1


def test_sorted_dense_build_out_of_order_side_of_deferred_size_runs_again(ctx, oracle, monkeypatch):
    """a build side of deferred size found out of order by a join that did not wait for its own size either: the status reaches
    the host through the consumer's synchronisation (verify_pending_sizes), the plan's input runs again, the result is right"""
    monkeypatch.setenv("QHIP_JOIN_DENSE", "2")
    rng = np.random.default_rng(91)
    na, nbb, nc = 20_000, 120_000, 400_000
    a_s = pa.schema([pa.field("ak", I64), pa.field("av", I64)])
    b_s = pa.schema([pa.field("bk", I64), pa.field("b_ak", I64), pa.field("bd", I64)])
    c_s = pa.schema([pa.field("c_bk", I64), pa.field("cv", I64)])
    A = pa.RecordBatch.from_arrays([pa.array(np.arange(1, na + 1), I64), pa.array(rng.integers(0, 5, na), I64)], schema=a_s)
    Bk = (np.arange(nbb) // 8) * 32 + np.arange(nbb) % 8 + 1
    Bk[5000:7000] = Bk[5000:7000][::-1].copy()                     # descents that survive join 1's selection of the rows
    B = pa.RecordBatch.from_arrays([pa.array(Bk, I64), pa.array(rng.integers(1, na * 2, nbb), I64), pa.array(rng.integers(0, 7, nbb), I64)], schema=b_s)
    C = pa.RecordBatch.from_arrays([pa.array(np.sort(Bk[rng.integers(0, nbb, nc)]), I64), pa.array(rng.integers(0, 1000, nc), I64)], schema=c_s)
    apred = q.BinaryExpr(col("av", 1), Operator.Eq, q.Literal(S.Int64(2)))
    ta, tb, tc = table_scan(a_s, [A], apred), table_scan(b_s, [B]), table_scan(c_s, [C])
    j1 = q.HashJoinExec.try_new(ta, tb, JoinType.Inner, [(col("ak", 0), col("b_ak", 1))], None)
    j2 = q.HashJoinExec.try_new(j1, tc, JoinType.Inner, [(col("bk", 2), col("c_bk", 0))], None)
    agg = q.HashAggregate(pa.schema([pa.field("bd", I64), pa.field("n", I64), pa.field("s", I64)]), j2, [col("bd", 4)],
                          [q.CountAggregateExpr(q.Literal(S.Int64(1))), q.SumAggregateExpr(col("cv", 6), I64)])
    want = sorted(rows_of(oracle.execute(agg)))
    ctx.forget_plans()
    monkeypatch.setenv("QHIP_JOIN_DENSE_SORTED", "0")   # the joins learn their sizes with the atomic build
    for _ in range(3):
        assert sorted(rows_of(agg.execute())) == want
    monkeypatch.setenv("QHIP_JOIN_DENSE_SORTED", "2")   # ... then both run of deferred size, join 2 tries the sorted build
    launched, fb = sorted_build_counts(ctx)
    assert sorted(rows_of(agg.execute())) == want
    launched2, fb2 = sorted_build_counts(ctx)
    assert launched2 > launched and fb2 > fb
    for _ in range(2):   # remembered: no further attempt on this build side
        assert sorted(rows_of(agg.execute())) == want
    assert sorted_build_counts(ctx)[1] == fb2


def test_ascending_statistic(ctx):
    """qhip_table_column_ascending: strictly ascending values, no NULLs; through index vectors only where they keep the order"""
    def scan(keys, mask=None):
        return _table(LS, keys, mask=mask)
    assert column_ascending(scan([1, 2, 5, 9, 10]).execute_device(), 0)
    assert column_ascending(scan([7]).execute_device(), 0)
    assert not column_ascending(scan([1, 2, 2, 3]).execute_device(), 0)          # equal neighbours
    assert not column_ascending(scan([4, 3, 2, 1]).execute_device(), 0)          # descending
    assert not column_ascending(scan(list(range(5000)) + [4998] + list(range(5001, 9000))).execute_device(), 0)
    assert not column_ascending(scan([1, 2, 3, 4], mask=np.array([False, True, False, False])).execute_device(), 0)   # a NULL
    # a Filter's compaction keeps the order
    keys = np.arange(20_000) * 3
    filt = q.Filter(scan(keys), q.BinaryExpr(col("bv", 1), Operator.Lt, q.Literal(S.Int64(7000))))
    assert column_ascending(filt.execute_device(), 0)
    # an Inner join with unique build keys: its probe side's index ascends, its build side's does not (the value columns, bv /
    # pv = 0, 1, 2, ... in their tables, are read through the index vectors; the key columns may come out as plain copies)
    build = _table(LS, np.random.default_rng(1).permutation(20_000))
    probe = _table(RS, np.arange(0, 40_000, 2))
    j = q.HashJoinExec.try_new(build, probe, JoinType.Inner, [(col("bk", 0), col("pk", 0))], None).execute_device()
    assert column_ascending(j, 3) and not column_ascending(j, 1)
    # duplicate build keys: a probe row may appear twice, the probe side's index no longer ascends strictly
    dup = _table(LS, np.concatenate([np.arange(1000), np.arange(500)]))
    j = q.HashJoinExec.try_new(dup, probe, JoinType.Inner, [(col("bk", 0), col("pk", 0))], None).execute_device()
    assert not column_ascending(j, 3)
    # a Left join's probe side is not taken as ordered (the tail rows come behind the pairs)
    j = q.HashJoinExec.try_new(build, probe, JoinType.Left, [(col("bk", 0), col("pk", 0))], None).execute_device()
    assert not column_ascending(j, 3)
