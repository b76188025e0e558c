"""GPU parity of the hash join's pass 2 when it sums the per-chunk pair counters ITSELF (csrc/kernels_rel.hip k_join_emit, `fold`).

A join of deferred size (its consumer reads the row count on the device) needs neither the chunk offsets nor the pair total
on the host before pass 2, so the one-workgroup scan launch in front of pass 2 is dropped when the probe has at most 8 192
chunks: every workgroup of pass 2 loads all the counters and reduces them to the sum below its first chunk and the grand
total. QHIP_JOIN_FOLD_SCAN=0 keeps the separate scan; QHIP_JOIN_FOLD_SCAN_MAX_CHUNKS lowers the threshold (tests: the scan
runs although the join defers). Every test compares with the CPU oracle under each of the three, and the pair ORDER is
compared, not only the pair set (hash_join.rs:475-512 pins probe-row-major order): a Left join over the deferred join's
output lists its unmatched build rows — the deferred join's pairs — in their order."""
import numpy as np
import pyarrow as pa
import pytest

import qurious_amd as q
from qurious_amd import JoinType, queries, synth
from qurious_amd.exchange import join_scan_counts

from .helpers import col, rows_of

pytestmark = pytest.mark.gpu
I64 = pa.int64()

# (name, environment): pass 2 sums the counters / the separate scan as before / the scan because the threshold is exceeded
MODES = [("fold", {"QHIP_JOIN_FOLD_SCAN": "1"}), ("scan", {"QHIP_JOIN_FOLD_SCAN": "0"}),
         ("over_threshold", {"QHIP_JOIN_FOLD_SCAN": "1", "QHIP_JOIN_FOLD_SCAN_MAX_CHUNKS": "1"})]


@pytest.fixture(params=MODES, ids=[m[0] for m in MODES])
def mode(request, monkeypatch):
    for k, v in request.param[1].items():
        monkeypatch.setenv(k, v)
    return request.param[0]


def _table(names, arrays, batch_rows=None):
    schema = pa.schema([pa.field(n, a.type, True) for n, a in zip(names, arrays)])
    n = len(arrays[0])
    step = batch_rows or max(n, 1)
    batches = [pa.RecordBatch.from_arrays([a.slice(o, step) for a in arrays], schema=schema) for o in range(0, max(n, 1), step)]
    return schema, q.MemoryTable.try_new(schema, batches)


def _same_batches(got, want, what):
    """the same batches, row for row and in the same order (Arrow arrays compared: the big shapes have 600 k rows)"""
    assert [b.num_rows for b in got] == [b.num_rows for b in want], what
    for g, w in zip(got, want):
        for k in range(w.num_columns):
            assert g.column(k).equals(w.column(k)), (what, "column", k)


def _syncs(ctx, fn):
    before = ctx.sync_count()
    out = fn()
    return out, ctx.sync_count() - before


def _folded(ctx, mode, fn):
    """run fn; the number of probes whose pass 2 summed the counters must fit the mode"""
    f0, _ = join_scan_counts(ctx)
    out = fn()
    f1, _ = join_scan_counts(ctx)
    if mode != "fold":
        assert f1 == f0, (mode, f0, f1)
    return out, f1 - f0


# probe rows P and which of them find a build row: (P, [(first row, rows) ranges that MISS]). The probe's chunks are runs of
# consecutive tiles of 256 rows (1 024 for the consecutive-rows dense probe), a workgroup of pass 2 owns four of them.
SHAPES = [
    (100, []),                                             # one chunk with entries, the workgroup's others empty
    (300, []),                                             # two chunks
    (97, [(0, 97)]),                                       # no pair at all
    (256 * 5 + 7, [(0, 256 * 2 + 9)]),                     # empty chunks in front; not a multiple of the workgroup's four
    (256 * 13 + 1, [(256 * 3, 256 * 4), (256 * 11, 300)]),  # empty chunks in the middle and at the end, several workgroups
    (256 * 41 + 3, [(256 * 8 - 5, 256 * 8 + 11)]),         # a workgroup whose four chunks are all empty
    (256 * 2300 + 3, [(0, 3000), (256 * 1000, 256 * 300), (256 * 2290, 256 * 10 + 3)]),   # > 1 024 chunks: several 16-byte loads per thread
]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_pair_order_of_a_join_of_deferred_size(ctx, oracle, mode, shape):
    P, miss = shape
    rng = np.random.default_rng(P)
    # (build row counts no other test uses: the context remembers a build side with duplicate keys by its key expressions and its
    # row count — a hint, not a record — and a join whose build side it takes for one neither speculates nor defers its size)
    nb = 733
    kmin = -(1 << 40) + 12345                      # (key minimum negative and far from 0)
    bk = kmin + rng.permutation(nb) * 3            # unique, unordered, with gaps
    build = _table(["bk", "bv"], [pa.array(bk, I64), pa.array(rng.integers(0, 1000, nb), I64)])
    pk = bk[rng.integers(0, nb, P)]
    sparse = rng.random(P) < 0.2                   # a fifth of the remaining rows miss too: between the build keys, outside their range
    pk = np.where(sparse, np.where(rng.random(P) < 0.5, pk + 1, kmin - 1 - rng.integers(0, 99, P)), pk)
    for first, rows in miss:
        pk[first:first + rows] = kmin + 3 * nb + 5 + np.arange(len(pk[first:first + rows]))
    probe = _table(["pk", "pid"], [pa.array(pk, I64), pa.array(np.arange(P) * 2 + 10, I64)], 4096)
    # the outer join's probe side matches three rows of the inner join's output at most: everything else is its tail
    k3 = np.array([10, 10 + 2 * (P // 2), 10 + 2 * (P - 1), 7, 9], dtype=np.int64)
    third = _table(["k3", "w"], [pa.array(k3, I64), pa.array(np.arange(5), I64)])
    (bs, bt), (ps, pt) = build, probe

    def plan():
        inner = q.HashJoinExec.try_new(q.Scan(bs, bt), q.Scan(ps, pt), JoinType.Inner, [(col("bk", 0), col("pk", 0))], None)
        return q.HashJoinExec.try_new(inner, q.Scan(*third), JoinType.Left, [(col("pid", 3), col("k3", 0))], None)

    want = oracle.execute(plan())
    folded = 0
    for execution in range(3):   # the first waits for the inner join's size and remembers it, the others defer it
        got, f = _folded(ctx, mode, plan().execute)
        folded += f
        _same_batches(got, want, (mode, P, execution))
    if mode == "fold":
        assert folded >= 2, folded


def _join_agg(build, probe):
    """SELECT pv, COUNT(*), SUM(bv) FROM build JOIN probe ON bk = pk GROUP BY pv — build (bk, bv), probe (pk, pv)"""
    (bs, bt), (ps, pt) = build, probe
    j = q.HashJoinExec.try_new(q.Scan(bs, bt), q.Scan(ps, pt), JoinType.Inner, [(col("bk", 0), col("pk", 0))], None)
    schema = pa.schema([pa.field("pv", I64), pa.field("n", I64), pa.field("s", I64)])
    return q.HashAggregate(schema, j, [col("pv", 3)], [q.CountAggregateExpr(q.Literal(q.ScalarValue.Int64(1))),
                                                      q.SumAggregateExpr(col("bv", 1), I64)])


def test_more_pairs_than_room_raises_the_retry(ctx, oracle, mode):
    """the same join over other data: the remembered size is too small, pass 2's own total must say so (QHIP_RETRY, the input
    runs again and waits), and the steady state after it costs one wait"""
    rng = np.random.default_rng(21)
    nb, npr = 5003, 70001      # (a build row count of this test's own, see above)
    build = _table(["bk", "bv"], [pa.array(np.arange(nb) - 2500, I64), pa.array(rng.integers(0, 1000, nb), I64)])
    few = _table(["pk", "pv"], [pa.array(rng.integers(2450, nb * 40, npr), I64), pa.array(rng.integers(0, 37, npr), I64)], 8192)
    many = _table(["pk", "pv"], [pa.array(rng.integers(-2500, 2500, npr), I64), pa.array(rng.integers(0, 37, npr), I64)], 8192)
    none = _table(["pk", "pv"], [pa.array(rng.integers(2600, 9000, npr), I64), pa.array(rng.integers(0, 37, npr), I64)], 8192)

    def run(probes):
        for probe in probes:
            agg = _join_agg(build, probe)
            want = sorted(rows_of(oracle.execute(agg)))
            t, _ = _folded(ctx, mode, agg.execute_device)
            assert sorted(rows_of(t.to_batches())) == want

    run((few, few, many, many, few))
    agg = _join_agg(build, many)
    agg.execute_device()          # more pairs than `few` left room for: runs twice
    (_, f), waits = _syncs(ctx, lambda: _folded(ctx, mode, agg.execute_device))
    assert waits == 1, waits
    assert f == (1 if mode == "fold" else 0), (mode, f)
    run((none, none, many, few, none))   # ... and a remembered size of zero pairs


def test_two_joins_and_an_aggregate_repeated(ctx, oracle, mode):
    """Q3's shape: both joins defer from the second execution on, the results stay the oracle's and the steady state waits once"""
    c, o, l = synth.q3_tables(0.05, orders_per_batch=4096)
    tabs = (q.MemoryTable.try_new(synth.CUSTOMER_SCHEMA, c), q.MemoryTable.try_new(synth.ORDERS_SCHEMA, o),
            q.MemoryTable.try_new(synth.LINEITEM_Q3_SCHEMA, l))
    plan = queries.q3(*tabs)
    want = sorted(rows_of(oracle.execute(plan)))
    assert sorted(rows_of(plan.execute())) == want and len(want) > 200
    plan.execute_device()
    for _ in range(2):
        ((t, f), waits) = _syncs(ctx, lambda: _folded(ctx, mode, plan.execute_device))
        assert waits == 1, waits
        assert f == (2 if mode == "fold" else 0), (mode, f)
        assert sorted(rows_of(t.to_batches())) == want


def test_duplicate_build_keys_take_the_general_branch(ctx, oracle, mode):
    """a remembered size, then a build side with duplicate keys: the attempt under speculation is thrown away whatever pass 2
    wrote, and the CSR attempt (sized on the host, the scan in front) gives the oracle's pairs"""
    rng = np.random.default_rng(22)
    nb, npr = 3011, 20011
    uniq = _table(["bk", "bv"], [pa.array(rng.permutation(nb), I64), pa.array(rng.integers(0, 9, nb), I64)])
    dup = _table(["bk", "bv"], [pa.array(rng.integers(0, nb // 2, nb), I64), pa.array(rng.integers(0, 9, nb), I64)])
    probe = _table(["pk", "pv"], [pa.array(rng.integers(0, nb, npr), I64), pa.array(rng.integers(0, 11, npr), I64)], 4096)
    for build in (uniq, uniq, dup, dup, uniq, uniq):
        agg = _join_agg(build, probe)
        got, _ = _folded(ctx, mode, agg.execute)
        assert sorted(rows_of(got)) == sorted(rows_of(oracle.execute(agg)))


@pytest.mark.parametrize("layout", ["hashed", "dense", "dense_sorted"])
def test_every_layout_under_the_folded_scan(ctx, oracle, mode, monkeypatch, layout):
    """pass 2 is the same kernel behind the hashed table, the dense layout's row_of form and its rank form (ascending build keys)"""
    monkeypatch.setenv("QHIP_JOIN_DENSE", "0" if layout == "hashed" else "2")
    if layout == "dense_sorted":
        monkeypatch.setenv("QHIP_JOIN_DENSE_SORTED", "2")
    rng = np.random.default_rng(23)
    nb, npr = 70, 300
    keys = 1000 + 5 * (np.arange(nb) if layout == "dense_sorted" else rng.permutation(nb))
    build = _table(["bk", "bv"], [pa.array(keys, I64), pa.array(rng.integers(0, 9, nb), I64)])
    probe = _table(["pk", "pv"], [pa.array(rng.integers(990, 1000 + 5 * nb + 10, npr), I64), pa.array(rng.integers(0, 11, npr), I64)], 128)
    third = _table(["k3", "w"], [pa.array(np.array([1000, 1005, 2], dtype=np.int64), I64), pa.array(np.arange(3), I64)])
    (bs, bt), (ps, pt) = build, probe
    for execution in range(3):
        inner = q.HashJoinExec.try_new(q.Scan(bs, bt), q.Scan(ps, pt), JoinType.Inner, [(col("bk", 0), col("pk", 0))], None)
        outer = q.HashJoinExec.try_new(inner, q.Scan(*third), JoinType.Left, [(col("pk", 2), col("k3", 0))], None)
        got, _ = _folded(ctx, mode, outer.execute)
        want = oracle.execute(outer)
        assert [b.num_rows for b in got] == [b.num_rows for b in want] and rows_of(got) == rows_of(want), (layout, execution)
