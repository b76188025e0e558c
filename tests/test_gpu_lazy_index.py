"""GPU parity of index vectors that are OWED like the columns behind them (csrc/common.hpp LazyIndex, relops.cpp index_rows).

A dense Inner join with unique build keys leaves its build-side index vector as the probe's key indices (key - min) and the key
column unwritten when no column of its build side is itself a pending gather; a parent join composes index vectors per group
of columns only when a column of the group is read. Every test runs with QHIP_JOIN_LAZY_INDEX=0 (everything at once, as
before) and 1, and compares with the CPU oracle — batch structure and row order included wherever batches are exported."""
import numpy as np
import pyarrow as pa
import pytest

import qurious_amd as q
from qurious_amd import JoinType, Operator, exchange, queries, synth
from qurious_amd.exchange import (INDEX_NOTHING, INDEX_PENDING_COMPOSITION, INDEX_PENDING_KEY, INDEX_PENDING_TRANSLATION, INDEX_READY,
                                  DeviceSource, column_index_state, lazy_index_counts)

from .helpers import col, lit_i64, rows_of

pytestmark = pytest.mark.gpu
I64 = pa.int64()
KMIN = -(1 << 40) + 77    # key minimum negative and far from 0


@pytest.fixture(params=["0", "1"], ids=["eager", "lazy"])
def lazy(request, monkeypatch):
    monkeypatch.setenv("QHIP_JOIN_LAZY_INDEX", request.param)
    monkeypatch.setenv("QHIP_JOIN_DENSE", "2")   # the dense layout wherever the key qualifies
    return request.param == "1"


@pytest.fixture(params=["row_of", "rank"])
def form(request, monkeypatch):
    """unordered build keys: row_of[key - min]; ascending build keys under the sorted build: rank + bitmap"""
    if request.param == "rank":
        monkeypatch.setenv("QHIP_JOIN_DENSE_SORTED", "2")
    return request.param


def _table(names, arrays, batch_rows=None):
    schema = pa.schema([pa.field(n, a.type, True) for n, a in zip(names, arrays)])
    n = len(arrays[0])
    step = batch_rows or max(n, 1)
    batches = [pa.RecordBatch.from_arrays([a.slice(o, step) for a in arrays], schema=schema) for o in range(0, max(n, 1), step)]
    return schema, q.MemoryTable.try_new(schema, batches)


def _same(got, want, what=None):
    assert [b.num_rows for b in got] == [b.num_rows for b in want], what
    assert rows_of(got) == rows_of(want), what


def _sides(form, matches, nb=70, npr=300, seed=1, pid=False):
    """build (bk, bv): nb unique keys with gaps from KMIN on; probe (pk, pv): keys of the build side, between them, and outside
    its range on both ends — or none of the build side's (`none`), or only those (`all`)"""
    rng = np.random.default_rng(seed)
    steps = np.arange(nb) * 3
    bk = KMIN + (steps if form == "rank" else rng.permutation(steps))
    build = _table(["bk", "bv"], [pa.array(bk, I64), pa.array(rng.integers(0, 1000, nb), I64)])
    hit = bk[rng.integers(0, nb, npr)]
    miss = np.where(rng.random(npr) < 0.5, hit + 1, np.where(rng.random(npr) < 0.5, KMIN - 1 - rng.integers(0, 50, npr), KMIN + 3 * nb + rng.integers(0, 50, npr)))
    pk = {"all": hit, "none": miss, "mixed": np.where(rng.random(npr) < 0.6, hit, miss)}[matches]
    cols = [pa.array(pk, I64), pa.array(rng.integers(0, 23, npr), I64)]
    if pid:   # (a unique probe-side column to key a second join on)
        cols.append(pa.array(np.arange(npr) * 2 + 5, I64))
    probe = _table(["pk", "pv", "pid"][:len(cols)], cols, 128 if npr <= 300 else 1024)
    return build, probe


def _join(build, probe, on=("bk", 0, "pk", 0)):
    (bs, bt), (ps, pt) = build, probe
    return q.HashJoinExec.try_new(q.Scan(bs, bt), q.Scan(ps, pt), JoinType.Inner, [(col(on[0], on[1]), col(on[2], on[3]))], None)


def _only(j, columns):
    js = j.schema()
    return q.Projection(pa.schema([js.field(k) for k in columns]), j, [col(js.field(k).name, k) for k in columns])


@pytest.mark.parametrize("matches", ["mixed", "none", "all"])
@pytest.mark.parametrize("read", ["whole", "build_column", "build_key", "probe_key", "probe_columns"])
def test_what_is_read_of_a_join_output(ctx, oracle, lazy, form, matches, read):
    build, probe = _sides(form, matches)
    j = _join(build, probe)
    plan = {"whole": j, "build_column": _only(j, [1]), "build_key": _only(j, [0]), "probe_key": _only(j, [2]), "probe_columns": _only(j, [3])}[read]
    want = oracle.execute(plan)
    before = lazy_index_counts(ctx)
    _same(plan.execute(), want, (form, matches, read))
    owed, translated, _, keys = (b - a for a, b in zip(before, lazy_index_counts(ctx)))
    if not lazy:
        assert (owed, translated, keys) == (0, 0, 0)
        return
    assert owed == 1
    if matches == "none":   # a join output without rows: its readers have nothing to gather, so nothing that is owed is ever asked for
        assert (translated, keys) == (0, 0), (read, translated, keys)
        return
    assert translated == (1 if read in ("whole", "build_column") else 0), (read, translated)
    assert keys == {"whole": 2, "build_key": 1, "probe_key": 1}.get(read, 0), (read, keys)


def test_the_pending_state_is_visible_without_a_launch(ctx, oracle, lazy, form):
    build, probe = _sides(form, "mixed")
    j = _join(build, probe)
    t = j.execute_device()
    before = lazy_index_counts(ctx)
    states = [column_index_state(t, k) for k in range(4)]
    if lazy:
        assert states == [INDEX_PENDING_KEY, INDEX_PENDING_TRANSLATION, INDEX_PENDING_KEY, INDEX_READY], states
    else:
        assert states == [INDEX_NOTHING, INDEX_READY, INDEX_NOTHING, INDEX_READY], states
    assert lazy_index_counts(ctx) == before
    _same(t.to_batches(), oracle.execute(j))
    assert [column_index_state(t, k) for k in range(4)] == [INDEX_NOTHING] * 4


def test_two_tables_share_one_resolution_and_plans_are_forgotten(ctx, oracle, lazy, form):
    build, probe = _sides(form, "mixed", seed=2)
    j = _join(build, probe)
    want = oracle.execute(j)
    t = j.execute_device()
    src = DeviceSource(j.schema(), t)
    before = lazy_index_counts(ctx)
    # a projection's table shares the join output's columns: what it resolves, the join output finds resolved
    _same(_only(src, [1, 3]).execute(), oracle.execute(_only(j, [1, 3])))
    _same(_only(src, [1]).execute(), oracle.execute(_only(j, [1])))
    _same(t.to_batches(), want)
    _, translated, _, keys = (b - a for a, b in zip(before, lazy_index_counts(ctx)))
    assert (translated, keys) == ((1, 2) if lazy else (0, 0))
    ctx.forget_plans()
    _same(j.execute(), want)
    _same(t.to_batches(), want)   # the earlier output outlives the plans


def test_readers_above_the_join(ctx, oracle, lazy, form):
    build, probe = _sides(form, "mixed", nb=700, npr=3000, seed=3)
    j = _join(build, probe)
    readers = [
        q.Filter(j, q.BinaryExpr(col("bv", 1), Operator.Gt, lit_i64(400))),
        q.Filter(j, q.BinaryExpr(col("pv", 3), Operator.Gt, lit_i64(4))),
        q.Sort([q.PhysicalSortExpr(col("bv", 1), q.SortOptions()), q.PhysicalSortExpr(col("pk", 2), q.SortOptions()),
                q.PhysicalSortExpr(col("pv", 3), q.SortOptions())], j),
        q.Limit(j, 1000, 100),
    ]
    for plan in readers:
        for _ in range(2):
            _same(plan.execute(), oracle.execute(plan), type(plan).__name__)
    # an aggregate reads the build-side column through the index vector (indirectly), from the second execution on over a join of deferred size
    schema = pa.schema([pa.field("pv", I64), pa.field("n", I64), pa.field("s", I64), pa.field("k", I64)])
    agg = q.HashAggregate(schema, j, [col("pv", 3)], [q.CountAggregateExpr(q.Literal(q.ScalarValue.Int64(1))), q.SumAggregateExpr(col("bv", 1), I64),
                                                      q.MinAggregateExpr(col("bk", 0), I64)])
    want = sorted(rows_of(oracle.execute(agg)))
    for _ in range(3):
        assert sorted(rows_of(agg.execute())) == want


def test_partition_over_the_join_output(ctx, oracle, lazy, form):
    build, probe = _sides(form, "mixed", nb=700, npr=5000, seed=4)
    j = _join(build, probe)
    whole = pa.Table.from_batches(oracle.execute(j)).combine_chunks().to_batches()[0]
    for key, keep in ((1, None), (3, [False, True, False, True]), (0, [True, True, False, False])):
        out = j.execute_device()
        parts = exchange.partition_filtered(out, [col(whole.schema.field(key).name, key)], 8, keep=keep)
        pid = oracle.partition_ids([whole.column(key)], 8)
        for p, part in enumerate(parts):
            want_rows = rows_of([whole.filter(pa.array(pid == p))])
            if keep is not None:
                want_rows = [tuple(v if keep[c] else None for c, v in enumerate(r)) for r in want_rows]
            assert rows_of(part.to_batches()) == want_rows, (key, p)


@pytest.mark.parametrize("rows", [1000, 3000, 12000])
def test_second_join_keyed_on_a_probe_side_column(ctx, oracle, lazy, form, rows):
    """Q3's shape: the first join's output is the second join's build side, keyed on a column of the first join's PROBE side; the
    aggregate above reads a column of the first join's build side (a composition over a translation, at the aggregate) or not"""
    build, probe2 = _sides(form, "mixed", nb=rows // 4, npr=rows, seed=5, pid=True)
    rng = np.random.default_rng(rows)
    third = _table(["k3", "w"], [pa.array(rng.integers(0, rows * 2 + 9, rows * 3), I64), pa.array(rng.integers(0, 7, rows * 3), I64)], 4096)

    def plans():
        j1 = _join(build, probe2)
        j2 = q.HashJoinExec.try_new(j1, q.Scan(*third), JoinType.Inner, [(col("pid", 4), col("k3", 0))], None)
        s1 = pa.schema([pa.field("w", I64), pa.field("n", I64), pa.field("s", I64)])
        reads_build = q.HashAggregate(s1, j2, [col("w", 6)], [q.CountAggregateExpr(q.Literal(q.ScalarValue.Int64(1))), q.SumAggregateExpr(col("bv", 1), I64)])
        reads_probe = q.HashAggregate(s1, j2, [col("w", 6)], [q.CountAggregateExpr(q.Literal(q.ScalarValue.Int64(1))), q.SumAggregateExpr(col("pv", 3), I64)])
        return j2, reads_build, reads_probe

    j2, reads_build, reads_probe = plans()
    want2 = oracle.execute(j2)
    want_b, want_p = sorted(rows_of(oracle.execute(reads_build))), sorted(rows_of(oracle.execute(reads_probe)))
    for execution in range(3):
        j2, reads_build, reads_probe = plans()
        before = lazy_index_counts(ctx)
        assert sorted(rows_of(reads_probe.execute())) == want_p, execution
        _, translated, composed, _ = (b - a for a, b in zip(before, lazy_index_counts(ctx)))
        if lazy:
            assert translated == 0 and composed == 1, (translated, composed)   # only the first join's probe-side group was read
        assert sorted(rows_of(reads_build.execute())) == want_b, execution
        _same(j2.execute(), want2, execution)


def test_second_join_keyed_on_a_build_side_column(ctx, oracle, lazy, form):
    """the second join's key is a column of the first join's BUILD side: reading it forces the translation, through the composition
    when a third join sits above"""
    rng = np.random.default_rng(6)
    nb, npr = 500, 2000
    steps = np.arange(nb) * 3
    bk = KMIN + (steps if form == "rank" else rng.permutation(steps))
    build = _table(["bk", "bu"], [pa.array(bk, I64), pa.array(rng.permutation(nb) * 5 + 1, I64)])       # bu: unique
    probe = _table(["pk", "pv"], [pa.array(KMIN + 3 * rng.permutation(npr)[:npr], I64), pa.array(rng.integers(0, 23, npr), I64)], 512)
    third = _table(["k3", "w"], [pa.array(rng.integers(0, nb * 6, 4000), I64), pa.array(rng.integers(0, 7, 4000), I64)], 1024)
    fourth = _table(["k4", "z"], [pa.array(rng.integers(0, 23, 900), I64), pa.array(rng.integers(0, 5, 900), I64)], 512)
    for execution in range(3):
        j1 = _join(build, probe)                     # every pk is distinct: (bk, bu, pk, pv) has unique bu
        j2 = q.HashJoinExec.try_new(j1, q.Scan(*third), JoinType.Inner, [(col("bu", 1), col("k3", 0))], None)
        _same(j2.execute(), oracle.execute(j2), execution)
        j3 = q.HashJoinExec.try_new(q.Scan(*fourth), j2, JoinType.Inner, [(col("k4", 0), col("pv", 3))], None)
        got, want = j3.execute(), oracle.execute(j3)
        assert sorted(rows_of(got)) == sorted(rows_of(want)) and [b.num_rows for b in got] == [b.num_rows for b in want], execution


def test_three_joins_deep_only_the_innermost_build_side_read(ctx, oracle, lazy, form):
    """a pending composition over a pending composition over a pending translation, resolved by the one reader at the top"""
    rng = np.random.default_rng(7)
    na, nbb, nc, nd = 300, 900, 2500, 6000
    steps = np.arange(na) * 3
    ak = KMIN + (steps if form == "rank" else rng.permutation(steps))
    A = _table(["ak", "av"], [pa.array(ak, I64), pa.array(rng.integers(0, 1000, na), I64)])
    B = _table(["bk", "bid"], [pa.array(KMIN + rng.integers(-20, 3 * na + 20, nbb), I64), pa.array(np.arange(nbb) * 2 + 1, I64)], 256)
    C = _table(["ck", "cid"], [pa.array(rng.integers(-9, 2 * nbb + 9, nc), I64), pa.array(np.arange(nc) * 3 + 2, I64)], 512)
    D = _table(["dk", "g"], [pa.array(rng.integers(-9, 3 * nc + 9, nd), I64), pa.array(rng.integers(0, 11, nd), I64)], 1024)

    def plans():
        j1 = q.HashJoinExec.try_new(q.Scan(*A), q.Scan(*B), JoinType.Inner, [(col("ak", 0), col("bk", 0))], None)      # ak av bk bid
        j2 = q.HashJoinExec.try_new(j1, q.Scan(*C), JoinType.Inner, [(col("bid", 3), col("ck", 0))], None)           # + ck cid
        j3 = q.HashJoinExec.try_new(j2, q.Scan(*D), JoinType.Inner, [(col("cid", 5), col("dk", 0))], None)           # + dk g
        top = q.HashAggregate(pa.schema([pa.field("g", I64), pa.field("n", I64), pa.field("s", I64)]), j3, [col("g", 7)],
                              [q.CountAggregateExpr(q.Literal(q.ScalarValue.Int64(1))), q.SumAggregateExpr(col("av", 1), I64)])
        return j3, top, _only(j3, [1]), _only(j3, [0, 7])

    j3, top, only_av, key_and_g = plans()
    wants = [oracle.execute(p) for p in (j3, top, only_av, key_and_g)]
    assert len(rows_of(wants[0])) > 50
    for execution in range(3):
        j3, top, only_av, key_and_g = plans()
        assert sorted(rows_of(top.execute())) == sorted(rows_of(wants[1])), execution
        _same(only_av.execute(), wants[2], execution)
        _same(key_and_g.execute(), wants[3], execution)
        _same(j3.execute(), wants[0], execution)
    if lazy:
        t = j3.execute_device()
        assert column_index_state(t, 1) == INDEX_PENDING_COMPOSITION and column_index_state(t, 7) == INDEX_READY


def _syncs(ctx, fn):
    before = ctx.sync_count()
    out = fn()
    return out, ctx.sync_count() - before


def test_repeated_executions_with_deferred_sizes(ctx, oracle, lazy):
    """two joins + an aggregate, repeated: the second and third execution defer both joins' sizes, wait once and give the oracle's
    result; Q3's first join owes its build-side vector and nobody asks for it"""
    c, o, l = synth.q3_tables(0.05, orders_per_batch=4096)
    tabs = (q.MemoryTable.try_new(synth.CUSTOMER_SCHEMA, c), q.MemoryTable.try_new(synth.ORDERS_SCHEMA, o),
            q.MemoryTable.try_new(synth.LINEITEM_Q3_SCHEMA, l))
    plan = queries.q3(*tabs)
    want = sorted(rows_of(oracle.execute(plan)))
    assert sorted(rows_of(plan.execute())) == want and len(want) > 200
    plan.execute_device()
    for _ in range(2):
        before = lazy_index_counts(ctx)
        t, waits = _syncs(ctx, plan.execute_device)
        assert waits == 1, waits
        assert sorted(rows_of(t.to_batches())) == want
        owed, translated, composed, keys = (b - a for a, b in zip(before, lazy_index_counts(ctx)))
        if lazy:
            assert (owed, translated, keys) == (1, 0, 0) and composed <= 1, (owed, translated, composed, keys)


def test_overflow_of_a_remembered_size_with_an_owed_vector(ctx, oracle, lazy, form):
    """the data changes between executions: more pairs than the remembered room, the input runs again, and the build-side column
    read by the aggregate (through the translation) is the oracle's"""
    rng = np.random.default_rng(9)
    nb, npr = 4000, 60001
    steps = np.arange(nb) * 2
    bk = KMIN + (steps if form == "rank" else rng.permutation(steps))
    build = _table(["bk", "bv"], [pa.array(bk, I64), pa.array(rng.integers(0, 1000, nb), I64)])
    few = _table(["pk", "pv"], [pa.array(KMIN + rng.integers(2 * nb - 100, nb * 40, npr), I64), pa.array(rng.integers(0, 37, npr), I64)], 8192)
    many = _table(["pk", "pv"], [pa.array(KMIN + 2 * rng.integers(0, nb, npr), I64), pa.array(rng.integers(0, 37, npr), I64)], 8192)
    schema = pa.schema([pa.field("pv", I64), pa.field("n", I64), pa.field("s", I64)])
    for probe in (few, few, many, many, few):
        agg = q.HashAggregate(schema, _join(build, probe), [col("pv", 3)], [q.CountAggregateExpr(q.Literal(q.ScalarValue.Int64(1))),
                                                                              q.SumAggregateExpr(col("bv", 1), I64)])
        assert sorted(rows_of(agg.execute())) == sorted(rows_of(oracle.execute(agg)))
    agg = q.HashAggregate(schema, _join(build, many), [col("pv", 3)], [q.CountAggregateExpr(q.Literal(q.ScalarValue.Int64(1))),
                                                                         q.SumAggregateExpr(col("bv", 1), I64)])
    agg.execute_device()
    _, waits = _syncs(ctx, agg.execute_device)
    assert waits == 1, waits
