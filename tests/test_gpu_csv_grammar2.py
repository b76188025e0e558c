"""Grammar level 2 of the device CSV decoder (qhip_ctx_set_csv_grammar(ctx, 2); csrc/csv.cpp, k_csv_decode<2>, k_csv_copy_utf8_q;
DESIGN §3.8): quoted fields, Boolean and Timestamp columns against the host path — `datasource.read_csv(device=False)`, Arrow C++
with an explicit schema — over the same bytes, compared exactly: schema, values, validity, no validity buffer without NULLs, batch
split. A file outside the grammar answers UnsupportedError at the low level and comes back from `read_csv(device=True)` as the host
path's table or the host path's error. Every input is well formed for the walk; a needs-host input is a normal return."""
import datetime
import io
import random

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

from qurious_amd import datasource
from qurious_amd._ffi import DeviceTable, UnsupportedError
from qurious_amd.expr import Column, CountAggregateExpr, MaxAggregateExpr, MinAggregateExpr, SumAggregateExpr
from qurious_amd.plan import HashAggregate, Scan

pytestmark = pytest.mark.gpu

DEC = pa.decimal128(15, 2)
TS_US = pa.timestamp("us")


@pytest.fixture(autouse=True)
def grammar2(ctx):
    """level 2 for the test, the default level behind it: the context is the process's"""
    ctx.set_csv_grammar(2)
    yield ctx
    ctx.set_csv_grammar(1)


def _write(tmp_path, data, name="t.csv"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _bits(col):
    return pa.compute.fill_null(col, 0.0).to_numpy(zero_copy_only=False).view(np.uint64)


def _assert_same(dev_batches, dev_schema, host, decoded=True):
    """the decoded batches against the host path's MemoryTable: schema, batch split, values, validity (decoded=False: both
    came from the host parse, whose batches are slices that share one validity buffer)"""
    assert dev_schema == host.schema()
    assert [b.num_rows for b in dev_batches] == [b.num_rows for b in host.data]
    for a, b in zip(dev_batches, host.data):
        assert a.schema == b.schema
        for ca, cb, f in zip(a.columns, b.columns, a.schema):
            assert ca.null_count == cb.null_count, f.name
            assert ca.equals(cb), f.name
            if ca.null_count == 0 and decoded:
                assert ca.buffers()[0] is None, f.name      # no NULLs, no validity buffer — as after an upload
            assert ca.is_valid().equals(cb.is_valid()), f.name
            if pa.types.is_float64(f.type):
                assert np.array_equal(_bits(ca), _bits(cb)), f.name


def _both(tmp_path, data, schema, header=True, batch_rows=None, columns=None):
    path = _write(tmp_path, data)
    o = datasource.CsvReadOptions(has_header=header)
    host = datasource.read_csv(path, o, schema, batch_rows, device=False, columns=columns)
    dev = datasource.read_csv(path, o, schema, batch_rows, device=True, columns=columns)
    return dev, host


def _same_as_host(tmp_path, data, schema, **kw):
    dev, host = _both(tmp_path, data, schema, **kw)
    assert dev.decoded_on_device is True and host.decoded_on_device is False
    _assert_same(dev.data, dev.schema(), host)
    return pa.Table.from_batches(dev.data, schema=dev.schema())


def _quoted(s):
    return '"' + s.replace('"', '""') + '"'


WORDS = ["", "a", "x,y", 'say "hi"', '"', '""', "ä€\U0001f600", "comma, and \"quote\", both", "plain words", ",", "tab\there", "nul\x00byte"]


def _default_writer_table(n, seed):
    rng = random.Random(seed)
    pick = lambda f: [None if rng.random() < 0.1 else f() for _ in range(n)]   # noqa: E731
    return pa.table({
        "k": pa.array(range(n), pa.int64()),
        "i": pa.array(pick(lambda: rng.randint(-2 ** 31, 2 ** 31 - 1)), pa.int32()),
        "d": pa.array(pick(lambda: datetime.date.fromordinal(rng.randint(1, 3652059))), pa.date32()),
        "m": pa.array(pick(lambda: __import__("decimal").Decimal(rng.randint(-10 ** 9, 10 ** 9)).scaleb(-2)), DEC),
        "f": pa.array(pick(lambda: rng.randint(-10 ** 6, 10 ** 6) / 4.0), pa.float64()),
        "s": pa.array([rng.choice(WORDS) for _ in range(n)], pa.string()),
        "c": pa.array([", ".join(rng.choice(WORDS) for _ in range(rng.randint(0, 4))) for _ in range(n)], pa.string()),
    })


def test_a_file_from_arrows_writer_with_default_options(ctx, tmp_path):
    """pacsv.write_csv puts every string value in quotes: the device decodes the file at level 2 and hands it to the host at
    level 1, on the same context"""
    tbl = _default_writer_table(5000, 1)
    path = str(tmp_path / "w.csv")
    pacsv.write_csv(tbl, path)
    with open(path, "rb") as f:
        data = f.read()
    assert b'"x,y"' in data and b'""hi""' in data
    host = datasource.read_csv(path, schema=tbl.schema, batch_rows=1024, device=False)
    dev = datasource.read_csv(path, schema=tbl.schema, batch_rows=1024, device=True)
    assert dev.decoded_on_device is True
    assert ctx.last_stats()["main_kernel_name"] == "k_csv_decode" and ctx.last_stats()["rows_out"] == 5000
    _assert_same(dev.data, dev.schema(), host)
    assert pa.Table.from_batches(dev.data).equals(tbl)
    ctx.set_csv_grammar(1)
    again = datasource.read_csv(path, schema=tbl.schema, batch_rows=1024, device=True)
    assert again.decoded_on_device is False
    _assert_same(again.data, again.schema(), host, decoded=False)
    with pytest.raises(UnsupportedError, match="a quote character"):
        DeviceTable.from_csv_bytes(ctx, tbl.schema, data)
    for bad in (0, 3):
        with pytest.raises(Exception):
            ctx.set_csv_grammar(bad)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_edges_of_lanes_wavefronts_and_vectors(ctx, n):
    types = [pa.int32(), pa.string(), pa.bool_(), TS_US]
    rng = random.Random(200 + n)
    recs = []
    for k in range(n):
        s = rng.choice(WORDS)
        b = rng.choice(["true", "false", "", '"true"', '""'])
        t = rng.choice(["", "1995-03-15 01:02:03", '"2024-02-29T23:59:59.999999"', "0001-01-01 00:00:00.5"])
        recs.append("%d,%s,%s,%s" % (k, _quoted(s) if (rng.random() < 0.8 or "," in s or '"' in s) else s, b, t))
    for shift in range(0, 18):
        names = ["k" + "x" * shift, "s", "b", "t"]       # the data begins 0 to 17 bytes later: quotes and pairs on every alignment of a 16-byte load
        schema = pa.schema([pa.field(a, t) for a, t in zip(names, types)])
        for final in (False, True):
            data = (",".join(names) + "\n" + "\n".join(recs) + ("\n" if final else "")).encode()
            dev = DeviceTable.from_csv_bytes(ctx, schema, data, batch_rows=100)
            assert dev.num_rows == n and dev.batch_offsets() == list(range(0, n, 100)) + [n]
            want = pacsv.read_csv(io.BytesIO(data), convert_options=pacsv.ConvertOptions(column_types=schema)).combine_chunks()
            assert pa.Table.from_batches(dev.to_batches()).equals(want), (n, shift, final)


def test_boolean_and_validity_words_at_the_64_row_edges(ctx, tmp_path):
    n = 300
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("b", pa.bool_()), pa.field("c", pa.bool_()), pa.field("s", pa.string())])
    special = (63, 64, 127, n - 1)
    # (a column with NULLs has them in every batch of 100: an exported batch carries the column's validity buffer or none)
    for null_at, true_at in ((special, ()), ((), special), ((63, 127, 250), (64, 151, n - 1))):
        rows = []
        for k in range(n):
            b = "" if k in null_at else ("true" if k in true_at else "false")
            c = "true" if k % 3 == 0 else ("" if k in true_at else "false")
            rows.append('%d,%s,"%s","r%d"' % (k, b, c, k))
        got = _same_as_host(tmp_path, ("k,b,c,s\n" + "\n".join(rows) + "\n").encode(), schema, batch_rows=100)   # (batches cut the bits at 100, 200)
        assert got["b"].to_pylist() == [None if k in null_at else k in true_at for k in range(n)]
        assert got["b"].null_count == len(null_at)


def _with_pairs_at(length, where):
    """a raw inner span of `length` bytes with one doubled quote whose first half stands at raw offset `where`"""
    raw = ["a"] * length
    raw[where] = raw[where + 1] = '"'
    return "".join(raw)


def test_the_undoubling_copy(ctx, tmp_path):
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string())])
    inners = []
    for length in (63, 64, 65, 127, 128, 129):
        for where in sorted({0, length - 2, 62, 63} - {length - 1}):     # a pair at the first, the last and the 64th byte (63|64 and 62|63)
            if where + 1 < length:
                inners.append(_with_pairs_at(length, where))
    for run in (2, 4, 130):                                              # a run of quotes across a 64-byte step
        for lead in (63, 62, 1):
            inners.append("b" * lead + '"' * run + "c" * 70)
    inners.append('""' + "x" * 100 + '""' * 33 + "y" * 61 + '""')
    big = ("ä€\U0001f600" + "x" * 86 + '""') * 2063                      # 9 + 86 + 2 = 97 bytes: a pair every 97 bytes, multi-byte characters
    big = big[:-2] + "z" * 91
    assert len(big.encode()) == 200_200 and len(big.replace('""', '"').encode()) > 198_000
    rows = ['%d,"%s"' % (k, v) for k, v in enumerate(inners)]
    rows += ['%d,"%s"' % (len(rows), big)]                               # larger than the LDS tile: walked in global memory, copied by the wavefront
    rows += ['%d,"short ""%d"""' % (k, k) for k in range(len(rows), len(rows) + 200)]
    got = _same_as_host(tmp_path, ("k,s\n" + "\n".join(rows) + "\n").encode(), schema, batch_rows=64)
    vals = got["s"].to_pylist()
    assert vals[:len(inners)] == [v.replace('""', '"') for v in inners] and vals[len(inners)] == big.replace('""', '"')


def test_the_200_000_byte_quoted_field(ctx, tmp_path):
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string()), pa.field("t", pa.string())])
    unit = "ä€\U0001f600" + "x" * 86 + '""'                               # 97 bytes raw
    big = unit * 2061 + "ä" * 41 + "w"                                   # 199 917 + 82 + 1 = 200 000 bytes
    assert len(big.encode()) == 200_000
    rows = ['%d,"w%d","%s"' % (k, k, "ü" * (k % 23)) for k in range(300)]
    rows[150] = '150,"%s","after, it"' % big
    got = _same_as_host(tmp_path, ("k,s,t\n" + "\n".join(rows)).encode(), schema, batch_rows=64)
    assert got["s"][150].as_py() == big.replace('""', '"') and got["t"][150].as_py() == "after, it"


@pytest.mark.parametrize("total", [48 * 1024 - 1, 48 * 1024, 48 * 1024 + 1])
def test_a_quoted_field_at_the_edge_of_the_lds_tile(ctx, tmp_path, total):
    """256 records of `total` bytes from byte 0 of the file: one byte below, at, and one byte above the 48 KB tile"""
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string())])
    rows = ['%d,"v,%d"' % (k, k) for k in range(256)]
    size = sum(len(r) + 1 for r in rows)
    fill = total - size
    unit = 'p,""'
    rows[100] = '100,"v,100' + unit * (fill // 4) + "q" * (fill % 4) + '"'
    first = "\n".join(rows) + "\n"
    assert len(first.encode()) == total
    rest = ['%d,"w""%d"' % (k, k) for k in range(256, 600)]
    got = _same_as_host(tmp_path, (first + "\n".join(rest) + "\n").encode(), schema, header=False, batch_rows=256)
    assert got["s"][100].as_py().startswith('v,100p,"p,"') and got["s"][599].as_py() == 'w"599'


GOOD = {pa.string(): '"ok, fine"', pa.bool_(): "true", TS_US: "1995-03-15 01:02:03.25"}
NEEDS_HOST = [
    # (column type, the offending field, projected?, what the message names)
    (pa.string(), 'ab"c', True, "quoting"), (pa.string(), '"ab"c', True, "quoting"), (pa.string(), '"ab"c"d"', True, "quoting"), (pa.string(), '"abc', True, "quoting"),
    (pa.string(), 'ab"c', False, "quoting"), (pa.string(), '"ab"c', False, "quoting"), (pa.string(), '"abc', False, "quoting"),
    (pa.string(), '"a\nb"', True, "quoting"), (pa.string(), '"a\r\nb"', True, "quoting"), (pa.string(), '"a\nb"', False, "quoting"),
    (pa.bool_(), "True", True, "boolean"), (pa.bool_(), "FALSE", True, "boolean"), (pa.bool_(), "0", True, "boolean"), (pa.bool_(), "1", True, "boolean"),
    (pa.bool_(), '" true"', True, "boolean"),
    (TS_US, "1995-03-15", True, "timestamp"), (TS_US, "1995-03-15 01:02", True, "timestamp"), (TS_US, "1995-03-15 1:02:03", True, "timestamp"),
    (TS_US, "1995-03-15 01:02:03.1234567", True, "timestamp"), (TS_US, "1995-03-15 01:02:03Z", True, "timestamp"), (TS_US, "1995-03-15 01:02:03+01:00", True, "timestamp"),
    (TS_US, "1995-03-15 24:00:00", True, "timestamp"), (TS_US, "1995-03-15 23:59:60", True, "timestamp"), (TS_US, '"1995-02-30 00:00:00"', True, "timestamp"),
]


@pytest.mark.parametrize("case", range(len(NEEDS_HOST)))
def test_needs_host_reasons(ctx, tmp_path, case):
    t, bad, projected, names = NEEDS_HOST[case]
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("v", t), pa.field("w", pa.int64())])
    idx, cols = (None, None) if projected else ([2, 0], ["w", "k"])
    for where in (0, 9999):                                   # in the first and in the last record of 10 000
        lines = [b"%d,%s,%d" % (k, (bad if k == where else GOOD[t]).encode(), k) for k in range(10000)]
        data = b"k,v,w\n" + b"\n".join(lines) + b"\n"
        with pytest.raises(UnsupportedError, match="needs the host path: .*%s.* in record %d$" % (names, where + 1)):
            DeviceTable.from_csv_bytes(ctx, schema, data, columns=idx)
        path = _write(tmp_path, data)
        try:
            host = datasource.read_csv(path, None, schema, 4096, device=False, columns=cols)
        except Exception as e:
            with pytest.raises(type(e)) as got:
                datasource.read_csv(path, None, schema, 4096, device=True, columns=cols)
            assert str(got.value) == str(e)
            continue
        got = datasource.read_csv(path, None, schema, 4096, device=True, columns=cols)
        assert got.decoded_on_device is False and type(got) is type(host)
        _assert_same(got.data, got.schema(), host, decoded=False)


def test_still_outside_the_grammar_at_level_2(ctx):
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("v", pa.string())])
    with pytest.raises(UnsupportedError, match="escape"):
        DeviceTable.from_csv_bytes(ctx, schema, b'k,v\n1,"a"\n', escape="\\")
    with pytest.raises(UnsupportedError, match="carriage return.* in record 2$"):
        DeviceTable.from_csv_bytes(ctx, schema, b'k,v\n1,a\n2,"b\rc"\n')
    for t in (pa.float32(), pa.time32("s"), pa.decimal256(40, 2), pa.timestamp("us", tz="UTC")):
        with pytest.raises(UnsupportedError):
            DeviceTable.from_csv_bytes(ctx, pa.schema([pa.field("k", pa.int64()), pa.field("v", t)]), b"k,v\n1,\n")


def test_an_unprojected_quoted_field_is_skipped(ctx, tmp_path):
    names, types = ["a", "junk", "b", "t", "m"], [pa.int64(), pa.int64(), pa.bool_(), TS_US, DEC]
    schema = pa.schema([pa.field(n, t) for n, t in zip(names, types)])
    rows = ['%d,"not, a ""number"", at all,,",%s,"1995-03-15 00:00:%02d",%d.5' % (k, "true" if k % 2 else "false", k % 60, k) for k in range(500)]
    data = ("a,junk,b,t,m\n" + "\n".join(rows) + "\n").encode()
    got = _same_as_host(tmp_path, data, schema, batch_rows=128, columns=["m", "a", "t", "b"])
    assert got.column_names == ["m", "a", "t", "b"] and got["a"].to_pylist() == list(range(500))
    with pytest.raises(UnsupportedError, match="integer.*record 1$"):
        DeviceTable.from_csv_bytes(ctx, schema, data)                     # projected, the field is no integer


def test_inferred_boolean_and_timestamp_types_pass_through(ctx, tmp_path):
    """schema=None: the types are Arrow's inference, which yields Boolean and Timestamp as the reference's loader does"""
    rows = ['%d,%s,1995-03-15 01:02:%02d,2001-01-01T00:00:00.%09d,"n, %d"' % (k, "true" if k % 2 else "false", k % 60, k, k) for k in range(300)]
    path = _write(tmp_path, ("k,b,t,u,s\n" + "\n".join(rows) + "\n").encode())
    host = datasource.read_csv(path, batch_rows=128, device=False)
    assert [f.type for f in host.schema()] == [pa.int64(), pa.bool_(), pa.timestamp("s"), pa.timestamp("ns"), pa.string()]
    dev = datasource.read_csv(path, batch_rows=128, device=True)
    assert dev.decoded_on_device is True
    _assert_same(dev.data, dev.schema(), host)


def test_a_query_over_a_decoded_quoted_file(ctx, tmp_path):
    n = 20000
    rng = random.Random(3)
    base = datetime.datetime(1995, 1, 1)
    tbl = pa.table({
        "g": pa.array([rng.choice(["a,b", 'q"r', "plain", ""]) for _ in range(n)], pa.string()),
        "v": pa.array([rng.randint(-1000, 1000) for _ in range(n)], pa.int64()),
        "b": pa.array([rng.choice([True, False, None]) for _ in range(n)], pa.bool_()),
        "t": pa.array([None if rng.random() < 0.05 else base + datetime.timedelta(microseconds=rng.randint(0, 10 ** 15)) for _ in range(n)], TS_US),
    })
    path = str(tmp_path / "q.csv")
    pacsv.write_csv(tbl, path)
    host = datasource.read_csv(path, schema=tbl.schema, batch_rows=4096, device=False)
    dev = datasource.read_csv(path, schema=tbl.schema, batch_rows=4096, device=True)
    assert dev.decoded_on_device is True

    def run(table):
        aggs = [SumAggregateExpr(Column("v", 1), pa.int64()), CountAggregateExpr(Column("v", 1)), MinAggregateExpr(Column("t", 3), TS_US),
                MaxAggregateExpr(Column("t", 3), TS_US)]
        plan = HashAggregate(None, Scan(tbl.schema, table, None, Column("b", 2)), [Column("g", 0)], aggs)
        return sorted(tuple(r) for b in plan.execute() for r in zip(*[c.to_pylist() for c in b.columns]))

    got = run(dev)
    assert dev._data is None                                    # the query ran on the decoded table; nothing was downloaded
    want = run(host)
    assert got == want and len(got) == 4
    keep = [i for i, b in enumerate(tbl["b"].to_pylist()) if b]
    assert sum(r[1] for r in got) == sum(tbl["v"][i].as_py() for i in keep)
