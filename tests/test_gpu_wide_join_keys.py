"""Hash join on keys of any width: a join key that does not fit the packed 8 key words (a Utf8 value of more than 55 bytes, many
columns) is encoded, on both sides, to one shared 32-bit key code per row in front of the join (csrc/join.cpp
maybe_encode_wide_join_key, csrc/device/qhip_widekey.inc), the way the reference hashes join keys of any length and any number of
columns and compares them on every probe hit (utils/array.rs:171-210, hash_join.rs:191-215). The switch is QHIP_JOIN_WIDE_KEYS
(0 off — the default —, 1 when the key does not fit, 2 every hash join over plain key columns); every test sets it with
monkeypatch.

Expected values come from the CPU oracle, compared in order and with the batch structure, and from a Python dict model of the
join (build rows by key tuple, a key with a None in it matches nothing; pairs in probe order, the build rows of a key ascending;
then the tail of unmatched / matched build rows)."""
import datetime
import decimal
import os
import re

import numpy as np
import pyarrow as pa
import pytest

import qurious_amd as q
from qurious_amd import JoinType, Operator
from tests.helpers import col, lit_i64, rows_of, table_scan

pytestmark = pytest.mark.gpu

I64 = pa.int64()
DEC = pa.decimal128(15, 2)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_TYPES = [JoinType.Inner, JoinType.Left, JoinType.Right, JoinType.Full, JoinType.LeftSemi, JoinType.LeftAnti]


def _batch(schema, rows):
    cols = list(zip(*rows)) if rows else [[] for _ in schema]
    return pa.RecordBatch.from_arrays([pa.array(list(c), type=f.type) for c, f in zip(cols, schema)], schema=schema)


def _ragged(batch, cuts):
    edges = [0] + [c for c in cuts if c < batch.num_rows] + [batch.num_rows]
    return [batch.slice(a, b - a) for a, b in zip(edges, edges[1:])]


def _batches_equal(got, want):
    assert [b.num_rows for b in got] == [b.num_rows for b in want]
    assert rows_of(got) == rows_of(want)
    for g, w in zip(got, want):
        assert [f.type for f in g.schema] == [f.type for f in w.schema]
        assert g.schema.names == w.schema.names


def _model(lrows, rrows, lkeys, rkeys, jt, keep_pair=None, keep_l=None, keep_r=None, width=(0, 0)):
    """The join's rows in the reference's order. keep_pair: the residual filter; keep_l / keep_r: fused scan filters (Inner)."""
    build = {}
    for i, l in enumerate(lrows):
        k = tuple(l[c] for c in lkeys)
        if None not in k and (keep_l is None or keep_l(l)):
            build.setdefault(k, []).append(i)
    nl, nr = len(lrows[0]) if lrows else width[0], len(rrows[0]) if rrows else width[1]   # (width: the columns of a side without rows)
    visited, out = set(), []
    for r in rrows:
        if keep_r is not None and not keep_r(r):
            continue
        hits = [i for i in build.get(tuple(r[c] for c in rkeys), []) if keep_pair is None or keep_pair(lrows[i], r)]
        visited.update(hits)
        if jt in (JoinType.LeftSemi, JoinType.LeftAnti):
            continue
        out.extend(lrows[i] + r for i in hits)
        if not hits and jt in (JoinType.Right, JoinType.Full):
            out.append((None,) * nl + r)
    if jt in (JoinType.Left, JoinType.Full):
        out.extend(l + (None,) * nr for i, l in enumerate(lrows) if i not in visited)
    if jt == JoinType.LeftSemi:
        out.extend(l for i, l in enumerate(lrows) if i in visited)
    if jt == JoinType.LeftAnti:
        out.extend(l for i, l in enumerate(lrows) if i not in visited)
    return out


def _counted(ctx, plan, calls=1):
    before = ctx.wide_key_joins()
    out = plan.execute()
    assert ctx.wide_key_joins() == before + calls
    return out


# ---------------------------------------------------------------- 1. the gap itself: one Utf8 key of up to 117 bytes
STEM = ("the first hundred bytes are the same in every value, ÿ and ü included; " * 2)[:98]
assert len(STEM.encode()) == 100


def _long_value(g):
    return STEM + ["", "a", "b", "é", "aa", "ab", "0123456789abc", "0123456789abd"][g % 8] + "%d" % (g // 8) * (g % 3)


LS = pa.schema([pa.field("b_name", pa.string()), pa.field("b_id", I64), pa.field("b_pay", pa.string())])
RS = pa.schema([pa.field("p_id", I64), pa.field("p_name", pa.string()), pa.field("p_v", pa.int32())])


@pytest.fixture(scope="module")
def gap(oracle):
    rng = np.random.default_rng(41)
    vals = sorted({_long_value(g) for g in range(260)})
    assert max(len(v.encode()) for v in vals) <= 117 and max(len(v.encode()) for v in vals) > 110 and len(vals) > 150
    lrows = [(None if rng.random() < 0.05 else vals[int(rng.integers(0, 120))], i, None if i % 13 == 0 else "pay-%d" % i) for i in range(300)]
    rrows = [(i, None if rng.random() < 0.05 else vals[int(rng.integers(0, len(vals)))], int(rng.integers(0, 1000))) for i in range(3000)]
    left = table_scan(LS, _ragged(_batch(LS, lrows), [100, 101]))
    right = table_scan(RS, _ragged(_batch(RS, rrows), [64, 64, 700, 701, 2999]))
    plans = {jt: q.HashJoinExec.try_new(left, right, jt, [(col("b_name", 0), col("p_name", 1))], None) for jt in ALL_TYPES}
    want = {jt: oracle.execute(p) for jt, p in plans.items()}
    for jt in ALL_TYPES:   # (the oracle against the dict model, once)
        assert rows_of(want[jt]) == _model(lrows, rrows, [0], [1], jt), jt
    assert sum(b.num_rows for b in want[JoinType.Inner]) > 3000   # duplicate build keys
    return plans, want


@pytest.mark.parametrize("jt", ALL_TYPES)
def test_wide_utf8_key_is_unsupported_without_the_switch_and_equal_to_the_oracle_with_it(ctx, monkeypatch, gap, jt, join_layout):
    plans, want = gap
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "0")
    before = ctx.wide_key_joins()
    with pytest.raises(q.UnsupportedError, match="longer than 55 bytes"):
        plans[jt].execute()
    assert ctx.wide_key_joins() == before
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    _batches_equal(_counted(ctx, plans[jt]), want[jt])
    _batches_equal(_counted(ctx, plans[jt]), want[jt])   # (the second call runs with what the first learnt about the join)


def test_the_context_switch_goes_before_the_environment(monkeypatch, gap):
    """On a context of its own (a mode, once set, stays set): qhip_ctx_set_wide_join_keys decides, whatever the environment says."""
    plans, want = gap
    fresh = q.Context()   # (the current device)
    assert fresh.wide_key_joins() == 0
    tables = []
    try:
        _context_switch(fresh, tables, monkeypatch, plans, want)
    finally:
        for t in tables:
            t.close()
        fresh.close()


def _context_switch(fresh, tables, monkeypatch, plans, want):
    lb = [b for b in plans[JoinType.Inner].left.datasource.data]
    rb = [b for b in plans[JoinType.Inner].right.datasource.data]
    lt, rt = q.DeviceTable.from_batches(fresh, LS, lb), q.DeviceTable.from_batches(fresh, RS, rb)
    tables += [lt, rt]
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "0")
    fresh.set_wide_join_keys(1)
    out = plans[JoinType.Inner]._join_tables(lt, rt)
    tables.append(out)
    _batches_equal(out.to_batches(), want[JoinType.Inner])
    assert fresh.wide_key_joins() == 1
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    fresh.set_wide_join_keys(0)
    with pytest.raises(q.UnsupportedError):
        plans[JoinType.Inner]._join_tables(lt, rt)
    for bad in (-1, 3):
        with pytest.raises(q.QuriousError):
            fresh.set_wide_join_keys(bad)
    assert fresh.wide_key_joins() == 1


# ---------------------------------------------------------------- 2. many key columns
def _nine_int_sides(rng, nb, np_, n_keys=9, bad_type=None):
    base = rng.integers(0, 3, (60, n_keys))
    ls = pa.schema([pa.field("bk%d" % k, I64) for k in range(n_keys)] + [pa.field("b_v", I64)])
    rs = pa.schema([pa.field("p_v", I64)] + [pa.field("pk%d" % k, pa.int32() if k == bad_type else I64) for k in range(n_keys)])
    lrows = [tuple(int(x) for x in base[int(rng.integers(0, 40))]) + (i,) for i in range(nb)]
    rrows = [(i,) + tuple(int(x) for x in base[int(rng.integers(0, 60))]) for i in range(np_)]
    on = [(col("bk%d" % k, k), col("pk%d" % k, k + 1)) for k in range(n_keys)]
    return ls, lrows, rs, rrows, on


@pytest.mark.parametrize("jt", [JoinType.Inner, JoinType.Full, JoinType.LeftAnti])
def test_nine_int64_key_columns(ctx, oracle, monkeypatch, jt):
    ls, lrows, rs, rrows, on = _nine_int_sides(np.random.default_rng(9), 200, 1500)
    plan = q.HashJoinExec.try_new(table_scan(ls, _ragged(_batch(ls, lrows), [77])), table_scan(rs, _ragged(_batch(rs, rrows), [333, 1000])), jt, on, None)
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "0")
    with pytest.raises(q.UnsupportedError, match="wider than 8 words"):
        plan.execute()
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    got = _counted(ctx, plan)
    assert rows_of(got) == _model(lrows, rrows, list(range(9)), list(range(1, 10)), jt)
    _batches_equal(got, oracle.execute(plan))


LONG = "a wide value of more than fifty-five bytes, the same in every row that has one, but for its end: "
assert len(LONG) > 55


@pytest.mark.parametrize("jt", ALL_TYPES)
def test_mixed_key_with_nulls_in_several_columns(ctx, oracle, monkeypatch, jt):
    """Int64 + Decimal128 + Date32 + Utf8(> 55 bytes) + UInt8, every key column nullable on both sides: a key with a NULL in it
    matches nothing, (NULL, x) does not match (NULL, x)."""
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    rng = np.random.default_rng(22)
    day0 = datetime.date(1996, 2, 27)
    types = [I64, DEC, pa.date32(), pa.string(), pa.uint8()]

    def key(g):
        return (g % 5, decimal.Decimal(g % 3 * 10**11 - 7).scaleb(-2), day0 + datetime.timedelta(days=g % 4), LONG + "%d" % (g % 7), g % 2)

    def side(n, n_keys, first):
        rows = list(first)
        for i in range(n):
            k = list(key(int(rng.integers(0, n_keys))))
            for c in range(5):
                if rng.random() < 0.06:
                    k[c] = None
            rows.append(tuple(k) + (i,))
        return rows
    # (NULL, x ...) on both sides, (x, NULL ...) on both sides, and the same keys without the NULL
    fixed = [(None,) + key(1)[1:] + (-1,), key(1)[:1] + (None,) + key(1)[2:] + (-2,), key(1) + (-3,), key(1)[:3] + (None, 1, -4), (None,) * 5 + (-5,)]
    lrows, rrows = side(250, 150, fixed), side(1200, 420, fixed)
    ls = pa.schema([pa.field("b%d" % c, t) for c, t in enumerate(types)] + [pa.field("b_v", I64)])
    rs = pa.schema([pa.field("p%d" % c, t) for c, t in enumerate(types)] + [pa.field("p_v", I64)])
    on = [(col("b%d" % c, c), col("p%d" % c, c)) for c in range(5)]
    plan = q.HashJoinExec.try_new(table_scan(ls, _ragged(_batch(ls, lrows), [3, 100])), table_scan(rs, _ragged(_batch(rs, rrows), [2, 5, 600])), jt, on, None)
    got = _counted(ctx, plan)
    want = _model(lrows, rrows, list(range(5)), list(range(5)), jt)
    assert rows_of(got) == want
    _batches_equal(got, oracle.execute(plan))
    if jt == JoinType.Inner:
        pairs = {(r[5], r[11]) for r in want}
        assert (-3, -3) in pairs and not any(a in (-1, -2, -4, -5) or b in (-1, -2, -4, -5) for a, b in pairs)


# ---------------------------------------------------------------- 3. duplicate build keys and unique ones
@pytest.mark.parametrize("forcing", [None, "QHIP_JOIN_FORCE_CSR", "QHIP_JOIN_NO_SPECULATION"])
@pytest.mark.parametrize("unique_build", [True, False])
def test_unique_and_duplicate_build_keys(ctx, oracle, monkeypatch, unique_build, forcing):
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    if forcing:
        monkeypatch.setenv(forcing, "1")
    rng = np.random.default_rng(33)
    nb = 400
    names = [LONG + "%05d" % g for g in (rng.permutation(nb) if unique_build else rng.integers(0, nb // 5, nb))]
    ls = pa.schema([pa.field("b_name", pa.string()), pa.field("b_v", I64)])
    rs = pa.schema([pa.field("p_name", pa.string()), pa.field("p_v", I64)])
    lrows = [(names[i], i) for i in range(nb)]
    rrows = [(LONG + "%05d" % int(rng.integers(0, nb + 100)), i) for i in range(2500)]
    left, right = table_scan(ls, [_batch(ls, lrows)]), table_scan(rs, _ragged(_batch(rs, rrows), [1000, 1001]))
    for jt in (JoinType.Inner, JoinType.Left, JoinType.Right, JoinType.LeftSemi):
        plan = q.HashJoinExec.try_new(left, right, jt, [(col("b_name", 0), col("p_name", 0))], None)
        want = oracle.execute(plan)
        for call in range(2):   # (the second call knows whether the build keys were unique)
            _batches_equal(_counted(ctx, plan), want)
        assert rows_of(want) == _model(lrows, rrows, [0], [0], jt)


# ---------------------------------------------------------------- 4. residual JoinFilter
@pytest.mark.parametrize("jt", [JoinType.Left, JoinType.Full, JoinType.Inner, JoinType.LeftSemi])
def test_residual_join_filter(ctx, oracle, monkeypatch, gap, jt):
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    plans, _ = gap
    left, right = plans[jt].left, plans[jt].right
    fschema = pa.schema([pa.field("b_id", I64), pa.field("p_id", I64)])
    jf = q.JoinFilter(q.BinaryExpr(q.BinaryExpr(col("b_id", 0), Operator.Mul, lit_i64(10)), Operator.Lt, col("p_id", 1)),
                      [(1, q.JoinSide.Left), (0, q.JoinSide.Right)], fschema)
    plan = q.HashJoinExec.try_new(left, right, jt, [(col("b_name", 0), col("p_name", 1))], jf)
    got = _counted(ctx, plan)
    _batches_equal(got, oracle.execute(plan))
    lrows, rrows = rows_of(left.datasource.data), rows_of(right.datasource.data)
    assert rows_of(got) == _model(lrows, rrows, [0], [1], jt, keep_pair=lambda l, r: l[1] * 10 < r[0])


# ---------------------------------------------------------------- 5. fused scan filters on both sides
def test_inner_join_with_fused_scan_filters(ctx, oracle, monkeypatch):
    """Scan(filter) children of an Inner join are fused into it. Every build key has five rows of which the filter passes ONE —
    the first, the last or a middle one, by key — so whichever row the encoding made the key's representative, most keys are
    represented by a row the filter rejects."""
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    rng = np.random.default_rng(55)
    ls = pa.schema([pa.field("b_name", pa.string()), pa.field("b_ok", I64), pa.field("b_v", I64)])
    rs = pa.schema([pa.field("p_name", pa.string()), pa.field("p_f", I64), pa.field("p_v", I64)])
    lrows = [(LONG + "%04d" % g, 1 if j == g % 5 else 0, g * 5 + j) for g in range(120) for j in range(5)]
    order = rng.permutation(len(lrows))
    lrows = [lrows[int(k)] for k in order]
    rrows = [(None if i % 29 == 0 else LONG + "%04d" % int(rng.integers(0, 150)), int(rng.integers(0, 10)), i) for i in range(3000)]
    lpred = q.BinaryExpr(col("b_ok", 1), Operator.Eq, lit_i64(1))
    rpred = q.BinaryExpr(col("p_f", 1), Operator.Lt, lit_i64(6))
    plan = q.HashJoinExec.try_new(table_scan(ls, _ragged(_batch(ls, lrows), [256]), lpred), table_scan(rs, _ragged(_batch(rs, rrows), [500, 1700]), rpred),
                                  JoinType.Inner, [(col("b_name", 0), col("p_name", 0))], None)
    want = _model(lrows, rrows, [0], [0], JoinType.Inner, keep_l=lambda l: l[1] == 1, keep_r=lambda r: r[1] < 6)
    assert len(want) > 1000 and {l[0] for l in lrows if l[1] == 1} == {LONG + "%04d" % g for g in range(120)}
    for call in range(2):
        got = _counted(ctx, plan)
        assert rows_of(got) == want
    _batches_equal(got, oracle.execute(plan))


# ---------------------------------------------------------------- 6. row counts
def _count_sides(nb, np_):
    """the same join twice: on a wide Utf8 key, and on the Int64 column that names the same key (a key that fits)"""
    ls = pa.schema([pa.field("b_name", pa.string()), pa.field("b_k", I64), pa.field("b_v", I64)])
    rs = pa.schema([pa.field("p_name", pa.string()), pa.field("p_k", I64), pa.field("p_v", I64)])
    lrows = [(LONG + "%d" % (i % 50), i % 50, i) for i in range(nb)]
    rrows = [(LONG + "%d" % (i * 7 % 80), i * 7 % 80, i) for i in range(np_)]
    return ls, lrows, rs, rrows


@pytest.mark.parametrize("nb,np_", [(0, 0), (0, 65), (1, 1), (1, 257), (63, 64), (64, 0), (65, 63), (257, 65), (64, 257)])
def test_row_counts(ctx, oracle, monkeypatch, nb, np_):
    ls, lrows, rs, rrows = _count_sides(nb, np_)
    left, right = table_scan(ls, _ragged(_batch(ls, lrows), [40])), table_scan(rs, _ragged(_batch(rs, rrows), [1, 64, 64, 200]))
    for jt in ALL_TYPES:
        wide = q.HashJoinExec.try_new(left, right, jt, [(col("b_name", 0), col("p_name", 0))], None)
        narrow = q.HashJoinExec.try_new(left, right, jt, [(col("b_k", 1), col("p_k", 1))], None)
        monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
        got = _counted(ctx, wide, calls=1 if nb + np_ else 0)   # (no value on either side: the key fits, the stage stays out)
        _batches_equal(got, oracle.execute(wide))
        assert rows_of(got) == _model(lrows, rrows, [0], [0], jt, width=(3, 3))
        monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "0")
        _batches_equal(got, narrow.execute())   # the batches a key that fits gives for the same shapes


@pytest.mark.parametrize("empty_side", ["build", "probe", "both"])
def test_zero_batches(ctx, oracle, monkeypatch, empty_side):
    ls, lrows, rs, rrows = _count_sides(65, 257)
    none_l, none_r = q.Scan(ls, q.MemoryTable.try_new(ls, []), None, None), q.Scan(rs, q.MemoryTable.try_new(rs, []), None, None)
    left = none_l if empty_side in ("build", "both") else table_scan(ls, [_batch(ls, lrows)])
    right = none_r if empty_side in ("probe", "both") else table_scan(rs, _ragged(_batch(rs, rrows), [100]))
    for jt in ALL_TYPES:
        wide = q.HashJoinExec.try_new(left, right, jt, [(col("b_name", 0), col("p_name", 0))], None)
        narrow = q.HashJoinExec.try_new(left, right, jt, [(col("b_k", 1), col("p_k", 1))], None)
        monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "2")   # (no rows: nothing to measure a key's width from)
        got = _counted(ctx, wide)
        _batches_equal(got, oracle.execute(wide))
        monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "0")
        _batches_equal(got, narrow.execute())


# ---------------------------------------------------------------- 7. more probe rows than one trip of the lookup's grid
def _lookup_grid_rows():
    """rows one trip of the lookup launch covers: its grid cap x QH_BLOCK, read from the launch code"""
    csrc = os.path.join(ROOT, "qurious_amd", "csrc")
    with open(os.path.join(csrc, "kernels.hpp")) as f:
        cap = int(re.search(r"constexpr unsigned kWideKeyGridCap = (\d+);", f.read()).group(1))
    with open(os.path.join(csrc, "kernels_rel.hip")) as f:
        text = f.read()
    launch = text[text.index("void launch_widekey_join_lookup("):]
    assert "grid_for(nrows, QH_BLOCK, kWideKeyGridCap)" in launch[:launch.index("\n}")]
    with open(os.path.join(csrc, "device", "qhip_device.hpp")) as f:
        block = int(re.search(r"#define QH_BLOCK (\d+)", f.read()).group(1))
    return cap * block


def test_probe_side_one_row_past_the_lookup_grid(ctx, monkeypatch):
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    rng = np.random.default_rng(77)
    nb, P = 1000, _lookup_grid_rows() + 1
    assert P == 8192 * 256 + 1
    bk = rng.integers(0, 4, (nb, 9)).astype(np.int64)
    bk[:, 0] = np.arange(nb)   # unique build keys
    pick = rng.integers(0, nb + 500, P)
    pick[-1] = 7               # the row of the second trip matches
    pk = bk[pick % nb].copy()
    pk[pick >= nb, 8] += 1000  # ... and a third of the probe rows match nothing
    p_v = rng.integers(0, 1000, P).astype(np.int64)
    ls = pa.schema([pa.field("bk%d" % k, I64) for k in range(9)] + [pa.field("b_g", I64)])
    rs = pa.schema([pa.field("pk%d" % k, I64) for k in range(9)] + [pa.field("p_v", I64)])
    lb = pa.RecordBatch.from_arrays([pa.array(bk[:, k]) for k in range(9)] + [pa.array(np.arange(nb, dtype=np.int64) % 7)], schema=ls)
    rb = pa.RecordBatch.from_arrays([pa.array(np.ascontiguousarray(pk[:, k])) for k in range(9)] + [pa.array(p_v)], schema=rs)
    join = q.HashJoinExec.try_new(table_scan(ls, [lb]), table_scan(rs, [rb]), JoinType.Inner, [(col("bk%d" % k, k), col("pk%d" % k, k)) for k in range(9)], None)
    plan = q.HashAggregate(None, join, [col("b_g", 9)], [q.CountAggregateExpr(lit_i64(1)), q.SumAggregateExpr(col("p_v", 19), I64), q.MaxAggregateExpr(col("bk0", 0), I64)])
    before = ctx.wide_key_joins()
    got = sorted(rows_of(plan.execute()))
    assert ctx.wide_key_joins() == before + 1
    hit = pick < nb
    g = (pick[hit] % nb) % 7
    want = [(int(k), int(np.sum(g == k)), int(p_v[hit][g == k].sum()), int(pick[hit][g == k].max())) for k in range(7)]
    assert got == want and hit[-1]


# ---------------------------------------------------------------- 8. colliding hashes
def test_colliding_hashes(ctx, monkeypatch, gap):
    """QHIP_JOIN_WIDE_KEY_HASH_BITS=3 leaves the encoding 8 hash values: all keys share 8 start slots and one tag, so every build
    row and every lookup walks a long chain of equal tags on different keys."""
    plans, want = gap
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEY_HASH_BITS", "3")
    for jt in (JoinType.Inner, JoinType.Full, JoinType.LeftAnti):
        _batches_equal(_counted(ctx, plans[jt]), want[jt])


# ---------------------------------------------------------------- 9. mode 2: keys that fit
def _modes_agree(monkeypatch, ctx, plan, stage_calls):
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "0")
    ordinary = plan.execute()
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "2")
    for call in range(2):   # (twice: a join below leaves its size on the device the second time)
        before = ctx.wide_key_joins()
        _batches_equal(plan.execute(), ordinary)
        assert ctx.wide_key_joins() == before + stage_calls
    return ordinary


@pytest.mark.parametrize("jt", ALL_TYPES)
def test_mode_2_one_int64_key(ctx, oracle, monkeypatch, jt):
    rng = np.random.default_rng(91)
    ls = pa.schema([pa.field("b_k", I64), pa.field("b_v", I64)])
    rs = pa.schema([pa.field("p_k", I64), pa.field("p_f", I64), pa.field("p_v", I64)])
    lrows = [(None if i % 17 == 0 else int(rng.integers(0, 300)), i) for i in range(400)]
    rrows = [(None if i % 19 == 0 else int(rng.integers(0, 400)), int(rng.integers(0, 10)), i) for i in range(4000)]
    left = table_scan(ls, [_batch(ls, lrows)])
    # (two Filters: a join fuses nothing but a Scan's own filter, the probe side is the second Filter's OUTPUT)
    right = q.Filter(q.Filter(table_scan(rs, _ragged(_batch(rs, rrows), [1000, 1001])), q.BinaryExpr(col("p_f", 1), Operator.Lt, lit_i64(8))),
                     q.BinaryExpr(col("p_f", 1), Operator.GtEq, lit_i64(1)))
    plan = q.HashJoinExec.try_new(left, right, jt, [(col("b_k", 0), col("p_k", 0))], None)
    ordinary = _modes_agree(monkeypatch, ctx, plan, 1)
    assert rows_of(ordinary) == _model(lrows, [r for r in rrows if 1 <= r[1] < 8], [0], [0], jt)
    # a computed key takes the ordinary path, silently
    computed = q.HashJoinExec.try_new(left, right, jt, [(q.BinaryExpr(col("b_k", 0), Operator.Add, lit_i64(0)), col("p_k", 0))], None)
    _batches_equal(_modes_agree(monkeypatch, ctx, computed, 0), ordinary)


def test_mode_2_utf8_and_date_key_over_a_join_output(ctx, oracle, monkeypatch):
    """the build side is itself a join's output (of deferred size the second time it runs), keyed by Utf8 + Date32"""
    rng = np.random.default_rng(92)
    day0 = datetime.date(1995, 1, 1)
    ds = pa.schema([pa.field("id", I64), pa.field("seg", pa.string())])
    fs = pa.schema([pa.field("fid", I64), pa.field("day", pa.date32()), pa.field("v", I64)])
    ps = pa.schema([pa.field("p_seg", pa.string()), pa.field("p_day", pa.date32()), pa.field("p_v", I64)])
    dims = [(i, None if i % 11 == 0 else "segment %d" % (i % 9)) for i in range(200)]
    facts = [(int(rng.integers(0, 260)), day0 + datetime.timedelta(days=int(rng.integers(0, 6))), i) for i in range(3000)]
    probe = [(None if i % 23 == 0 else "segment %d" % int(rng.integers(0, 11)), day0 + datetime.timedelta(days=int(rng.integers(0, 8))), i) for i in range(500)]
    inner = q.HashJoinExec.try_new(table_scan(ds, [_batch(ds, dims)]), table_scan(fs, _ragged(_batch(fs, facts), [500, 2345])), JoinType.Inner,
                                   [(col("id", 0), col("fid", 0))], None)
    for jt in (JoinType.Inner, JoinType.Left, JoinType.Right):
        plan = q.HashJoinExec.try_new(inner, table_scan(ps, _ragged(_batch(ps, probe), [100])), jt, [(col("seg", 1), col("p_seg", 0)), (col("day", 3), col("p_day", 1))], None)
        ordinary = _modes_agree(monkeypatch, ctx, plan, 2)   # (both joins go through the stage)
        _batches_equal(ordinary, oracle.execute(plan))


# ---------------------------------------------------------------- 10. errors kept
def test_errors_kept(ctx, monkeypatch):
    # a pairwise type mismatch: the reference's text, on a key that fits (both modes) and on one that does not
    ls, lrows, rs, rrows, on = _nine_int_sides(np.random.default_rng(10), 50, 80, n_keys=2, bad_type=1)
    fits = q.HashJoinExec.try_new(table_scan(ls, [_batch(ls, lrows)]), table_scan(rs, [_batch(rs, rrows)]), JoinType.Inner, on, None)
    texts = []
    for mode in ("0", "1", "2"):
        monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", mode)
        with pytest.raises(q.QuriousError, match="Invalid argument error: Invalid comparison operation: Int64 == Int32") as e:
            fits.execute()
        texts.append((type(e.value), str(e.value)))
    assert texts[0] == texts[1] == texts[2]
    ls, lrows, rs, rrows, on = _nine_int_sides(np.random.default_rng(11), 50, 80, n_keys=9, bad_type=4)
    wide = q.HashJoinExec.try_new(table_scan(ls, [_batch(ls, lrows)]), table_scan(rs, [_batch(rs, rrows)]), JoinType.Left, on, None)
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    before = ctx.wide_key_joins()
    with pytest.raises(q.QuriousError, match="Invalid argument error: Invalid comparison operation: Int64 == Int32") as e:
        wide.execute()
    assert type(e.value) is texts[0][0] and ctx.wide_key_joins() == before
    # a key type the reference's hasher does not take: its text, in every mode
    fl = pa.schema([pa.field("b_f", pa.float64()), pa.field("b_v", I64)])
    fr = pa.schema([pa.field("p_f", pa.float64()), pa.field("p_v", I64)])
    floats = q.HashJoinExec.try_new(table_scan(fl, [(1.5, 1), (2.5, 2)]), table_scan(fr, [(1.5, 1)]), JoinType.Inner, [(col("b_f", 0), col("p_f", 0))], None)
    texts = []
    for mode in ("0", "2"):
        monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", mode)
        with pytest.raises(q.QuriousError, match="Unsupported data type in hasher") as e:
            floats.execute()
        texts.append((type(e.value), str(e.value)))
    assert texts[0] == texts[1]
    # 33 key columns
    ls, lrows, rs, rrows, on = _nine_int_sides(np.random.default_rng(12), 20, 30, n_keys=33)
    many = q.HashJoinExec.try_new(table_scan(ls, [_batch(ls, lrows)]), table_scan(rs, [_batch(rs, rrows)]), JoinType.Inner, on, None)
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    with pytest.raises(q.UnsupportedError, match="more than 32 columns"):
        many.execute()
    # a computed key that does not fit
    ls, lrows, rs, rrows, on = _nine_int_sides(np.random.default_rng(13), 50, 80)
    on[4] = (q.BinaryExpr(on[4][0], Operator.Add, lit_i64(0)), on[4][1])
    computed = q.HashJoinExec.try_new(table_scan(ls, [_batch(ls, lrows)]), table_scan(rs, [_batch(rs, rrows)]), JoinType.Inner, on, None)
    before = ctx.wide_key_joins()
    with pytest.raises(q.UnsupportedError, match="wider than 8 words.*computed join keys are not encoded"):
        computed.execute()
    assert ctx.wide_key_joins() == before
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "0")
    with pytest.raises(q.UnsupportedError, match="wider than 8 words$"):
        computed.execute()


# ---------------------------------------------------------------- 11. the Q10 shape end to end
def test_q10_shape_end_to_end(ctx, monkeypatch):
    """customer ⋈ orders on (c_name, c_address, c_comment) under Q10's seven-column GROUP BY, both switches on, then ORDER BY +
    LIMIT; the exported result ingested again."""
    monkeypatch.setenv("QHIP_JOIN_WIDE_KEYS", "1")
    monkeypatch.setenv("QHIP_AGG_WIDE_KEYS", "1")
    rng = np.random.default_rng(10)
    cs = pa.schema([pa.field("c_custkey", I64), pa.field("c_name", pa.string()), pa.field("c_acctbal", DEC), pa.field("c_phone", pa.string()),
                    pa.field("n_name", pa.string()), pa.field("c_address", pa.string()), pa.field("c_comment", pa.string())])
    os_ = pa.schema([pa.field("o_name", pa.string()), pa.field("o_address", pa.string()), pa.field("o_comment", pa.string()), pa.field("revenue", DEC), pa.field("qty", I64)])
    words = ["quickly", "ironic", "déposits", "blithely", "über", "furiously", "señor", "pending", "日本", "requests"]

    def customer(c):
        comment = " ".join(words[(c // 3 * 7 + j * 3) % len(words)] for j in range(40))
        while len(comment.encode()) > 113:
            comment = comment[:-1]
        comment += ["", "é", "zz"][c % 3] + "."
        return (c, "Customer#%09d" % (c // 2), decimal.Decimal(c * 37 % 100000 - 5000).scaleb(-2), "%02d-%03d" % (c % 25 + 10, c % 1000),
                ["ALGERIA", "UNITED KINGDOM", "MOZAMBIQUE"][c % 3], ("%d Long Street, Springfield, Block %d" % (c // 2, c % 97))[:40], comment)
    custs = [customer(c) for c in range(600)]
    assert len({c[1:2] + c[5:7] for c in custs}) == 600 and max(len(c[6].encode()) for c in custs) > 100
    orders = []
    for i in range(6000):
        c = custs[int(rng.integers(0, 600))]
        name = c[1] if i % 31 else None
        comment = c[6] if i % 37 else c[6][:-1] + "?"   # (a comment no customer has)
        orders.append((name, c[5], comment, decimal.Decimal(int(rng.integers(-100000, 1000000))).scaleb(-2), int(rng.integers(1, 51))))
    join = q.HashJoinExec.try_new(table_scan(cs, _ragged(_batch(cs, custs), [250])), table_scan(os_, _ragged(_batch(os_, orders), [2000, 2001, 5999])), JoinType.Inner,
                                  [(col("c_name", 1), col("o_name", 0)), (col("c_address", 5), col("o_address", 1)), (col("c_comment", 6), col("o_comment", 2))], None)
    keys = [col(f.name, k) for k, f in enumerate(cs)]
    agg = q.HashAggregate(None, join, keys, [q.SumAggregateExpr(col("revenue", 10), DEC), q.CountAggregateExpr(lit_i64(1)), q.MaxAggregateExpr(col("qty", 11), I64)])
    groups = {}
    for r in _model(custs, orders, [1, 5, 6], [0, 1, 2], JoinType.Inner):
        g = groups.setdefault(r[:7], [decimal.Decimal(0), 0, 0])
        g[0] += r[10]; g[1] += 1; g[2] = max(g[2], r[11])
    want = [k + tuple(v) for k, v in groups.items()]
    assert 500 < len(want) <= 600
    order = [q.PhysicalSortExpr(col("revenue", 7), q.SortOptions(True, False)), q.PhysicalSortExpr(col("c_comment", 6), q.SortOptions(False, True)),
             q.PhysicalSortExpr(col("c_custkey", 0), q.SortOptions(False, True))]
    joins, aggs = ctx.wide_key_joins(), ctx.wide_key_aggregates()
    top = rows_of(q.Limit(q.Sort(order, agg), 20, 0).execute())
    assert (ctx.wide_key_joins(), ctx.wide_key_aggregates()) == (joins + 1, aggs + 1)
    assert top == sorted(want, key=lambda r: (-r[7], r[6].encode(), r[0]))[:20]
    # the exported result, ingested again and joined back to the customers on the same wide key: every group once
    out = agg.execute()
    assert sorted(rows_of(out), key=repr) == sorted(want, key=repr)
    out_schema = pa.schema([pa.field("g_" + f.name, f.type) for f in cs] + [pa.field("revenue", DEC), pa.field("n", I64), pa.field("hi", I64)])
    again = [pa.RecordBatch.from_arrays(b.columns, schema=out_schema) for b in out]
    back = q.HashJoinExec.try_new(table_scan(out_schema, again), table_scan(cs, [_batch(cs, custs)]), JoinType.Right,
                                  [(col("g_c_name", 1), col("c_name", 1)), (col("g_c_address", 5), col("c_address", 5)), (col("g_c_comment", 6), col("c_comment", 6))], None)
    by_key = {w[:7]: w for w in want}
    assert rows_of(_counted(ctx, back)) == [by_key.get(c, (None,) * 10) + c for c in custs]
