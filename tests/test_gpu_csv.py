"""Decoding CSV text on the device (qhip_table_from_csv, csrc/csv.cpp + kernels_csv.hip) against the host path:
`datasource.read_csv(device=False)` — Arrow C++ with an explicit schema — over the same bytes is the yardstick, compared exactly:
schema, values (floats by their bits), validity and batch split. A file outside the device's grammar must answer
UnsupportedError at the low level and come back from `read_csv(device=True)` as the host path's table or the host path's error."""
import datetime
import io
import random

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

from qurious_amd import datasource, queries, synth
from qurious_amd._ffi import DeviceTable, UnsupportedError
from qurious_amd.expr import Column, CountAggregateExpr, MaxAggregateExpr, MinAggregateExpr, SumAggregateExpr
from qurious_amd.plan import Limit, NoGroupingAggregate, Scan

pytestmark = pytest.mark.gpu

DEC = pa.decimal128(15, 2)
TYPES = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64(), pa.float64(), pa.date32(), DEC, pa.string()]
NAMES = ["i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "f", "d", "m", "s"]
SCHEMA = pa.schema([pa.field(n, t) for n, t in zip(NAMES, TYPES)])
WORDS = ["", "a", "xy", "hello", "ä", "€uro", "\U0001f600", "R", "N", "A", "tab\there", "sp ace", "nul\x00byte", "longer value with several words"]


def _field(rng, t):
    if not pa.types.is_string(t) and rng.random() < 0.1:
        return ""
    if pa.types.is_integer(t):
        bits = t.bit_width
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if pa.types.is_signed_integer(t) else (0, (1 << bits) - 1)
        return str(rng.choice([lo, hi, 0, rng.randint(lo, hi), rng.randint(max(lo, -99), min(hi, 99))]))
    if pa.types.is_float64(t):
        return rng.choice(["-0.0", "0", "1.5", "1e22", "123456.789", "-2.5E-3", "9007199254740992", "%d.%02d" % (rng.randint(0, 10 ** 6), rng.randint(0, 99))])
    if pa.types.is_date32(t):
        return datetime.date.fromordinal(rng.randint(1, 3652059)).isoformat()
    if pa.types.is_decimal(t):
        return rng.choice(["12", "12.5", ".5", "5.", "-0", "-9999999999999.99", "%d.%02d" % (rng.randint(0, 10 ** 6), rng.randint(0, 99))])
    return rng.choice(WORDS)


def _records(n, seed, types=TYPES):
    rng = random.Random(seed)
    return [",".join(_field(rng, t) for t in types) for _ in range(n)]


def _text(records, names=NAMES, header=True, ends=("\n", "\r\n"), final=False, seed=0):
    rng = random.Random(seed)
    out = [",".join(names) + "\n"] if header else []
    for k, r in enumerate(records):
        out.append(r + (rng.choice(ends) if (final or k + 1 < len(records)) else ""))
    return "".join(out).encode()


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


def _both(tmp_path, data, schema, header=True, batch_rows=None, columns=None, delimiter=","):
    path = _write(tmp_path, data)
    o = datasource.CsvReadOptions(has_header=header, delimiter=delimiter)
    host = datasource.read_csv(path, o, schema, batch_rows, device=False, columns=columns)
    dev = datasource.read_csv(path, o, schema, batch_rows, device=True, columns=columns)
    return dev, host


@pytest.mark.parametrize("header", [True, False])
def test_canonical_file(ctx, tmp_path, header):
    data = _text(_records(1000, 1), header=header)
    assert not data.endswith(b"\n") and b"\r\n" in data and b",,," in data
    dev, host = _both(tmp_path, data, SCHEMA, header=header, batch_rows=256)
    assert dev.decoded_on_device is True and host.decoded_on_device is False
    assert dev.device_table().batch_offsets() == [0, 256, 512, 768, 1000]
    st = ctx.last_stats()
    assert st["rows_out"] == 1000 and st["main_kernel_name"] == "k_csv_decode"
    _assert_same(dev.data, dev.schema(), host)
    assert any(c.null_count for b in dev.data for c in b.columns)
    # the decoded table is an ordinary MemoryTable from here on
    assert dev.device_table() is dev.device_table()
    dev.insert(host.data[:1])
    assert dev.device_table().num_rows == 1256


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_edges_of_lanes_wavefronts_and_vectors(ctx, n):
    types = [pa.int32(), pa.string(), pa.float64()]
    recs = _records(n, 100 + n, types)
    for shift in range(0, 18):
        names = ["k" + "x" * shift, "s", "f"]       # the data begins 1 to 17 bytes later: every alignment of a 16-byte load
        schema = pa.schema([pa.field(a, t) for a, t in zip(names, types)])
        for final in (False, True):
            data = _text(recs, names=names, final=final, seed=shift)
            dev = DeviceTable.from_csv_bytes(ctx, schema, data, batch_rows=100)
            assert dev.num_rows == n
            want = pacsv.read_csv(io.BytesIO(data), convert_options=pacsv.ConvertOptions(column_types=schema)).combine_chunks()
            got = dev.to_batches()
            assert dev.batch_offsets() == ([0] if n == 0 else list(range(0, n, 100)) + [n])
            if n:
                assert pa.Table.from_batches(got).equals(want), (n, shift, final)
            else:
                assert got == [] and dev.num_batches == 0 and dev.schema() == schema


@pytest.mark.parametrize("edge", [16, 4096, 16384, 32768])
def test_line_end_across_a_block_edge(ctx, tmp_path, edge):
    """'\\r' as the last byte of a vector / iteration / workgroup chunk, '\\n' as the first of the next — and the same edge
    between a '\\n' and the record behind it, and inside a multi-byte character"""
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string())])
    for lead in (b"\r\n", b"\n", "€".encode() + b"\n"):
        for at in (edge - 1, edge, edge + 1):
            head = b"k,s\n1,"
            pad = at - len(head) - (len(lead) - 1)          # lead's last byte lands on position `at`
            if pad < 0:
                continue
            data = head + b"p" * pad + lead + b"2,two\r\n3,\n4,four"
            assert data[at] == lead[-1]
            dev, host = _both(tmp_path, data, schema)
            assert dev.decoded_on_device
            _assert_same(dev.data, dev.schema(), host)
            assert dev.device_table().num_rows == 4


def test_long_and_odd_fields(ctx, tmp_path):
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string()), pa.field("t", pa.string())])
    big = "ä€\U0001f600x" * 20000                          # 10 bytes each: multi-byte characters across every 16-byte edge
    assert len(big.encode()) == 200_000                    # larger than any LDS tile: the global-memory walk
    rows = ["%d,%s,%s" % (k, WORDS[k % len(WORDS)], "ü" * (k % 23)) for k in range(300)]
    rows[150] = "150,%s,after" % big
    rows[151] = "151,,"
    rows[152] = "152,a\x00b,\x00"
    data = _text(rows, names=["k", "s", "t"], final=True)
    dev, host = _both(tmp_path, data, schema, batch_rows=64)
    assert dev.decoded_on_device
    _assert_same(dev.data, dev.schema(), host)
    got = pa.Table.from_batches(dev.data)
    assert got["s"][150].as_py() == big and got["s"][151].as_py() == "" and got["s"][152].as_py() == "a\x00b" and got["t"][151].is_valid


def test_projection_leaves_other_fields_unparsed(ctx, tmp_path):
    types = [pa.int64(), pa.string(), pa.date32(), pa.int64(), pa.float64(), DEC]
    names = ["a", "b", "c", "x", "e", "m"]
    schema = pa.schema([pa.field(n, t) for n, t in zip(names, types)])
    recs = _records(500, 7, types)
    recs = [",".join(f if k != 3 else "gar bage+" for k, f in enumerate(r.split(","))) for r in recs]
    data = _text(recs, names=names)
    path = _write(tmp_path, data)
    dev = DeviceTable.from_csv_bytes(ctx, schema, data, columns=[5, 0, 2], batch_rows=128)
    assert dev.schema() == pa.schema([schema.field(5), schema.field(0), schema.field(2)])
    host = datasource.read_csv(path, schema=schema, batch_rows=128, device=False, columns=["m", "a", "c"])
    _assert_same(dev.to_batches(), dev.schema(), host)
    t = datasource.read_csv(path, schema=schema, batch_rows=128, device=True, columns=["m", "a", "c"])
    assert t.decoded_on_device
    _assert_same(t.data, t.schema(), host)
    with pytest.raises(UnsupportedError, match="integer.*record 1"):
        DeviceTable.from_csv_bytes(ctx, schema, data)                      # projected, the garbage needs the host
    with pytest.raises(UnsupportedError, match="field count.*record 500"):
        DeviceTable.from_csv_bytes(ctx, schema, data + b",1", columns=[5, 0, 2])   # the field count is checked regardless


# (column type, the offending field) or a whole-record rewrite: every reason of the grammar
FIELD_REASONS = [
    (pa.int32(), "+5"), (pa.int32(), " 5"), (pa.int32(), "5 "), (pa.int32(), "5.0"), (pa.int32(), "1e3"), (pa.int32(), "2147483648"),
    (pa.int32(), "NULL"), (pa.int32(), "N/A"), (pa.int32(), "nan"),
    (pa.date32(), "1995-3-15"), (pa.date32(), "1995-02-30"), (pa.date32(), "1995-03-15 "),
    (DEC, "+1.5"), (DEC, "1e2"), (DEC, "1.234"), (DEC, "12345678901234.5"),
    (pa.float64(), "12345678901234567890"), (pa.float64(), "1e300"), (pa.float64(), "inf"), (pa.float64(), "nan"), (pa.float64(), "0x10"),
    (pa.string(), b"\xff\xfe"), (pa.string(), '"quoted"'), (pa.string(), "lone\rcr"),
]
GOOD = {pa.int32(): "5", pa.date32(): "1995-03-15", DEC: "1.5", pa.float64(): "1.5", pa.string(): "ok"}


def _check_needs_host(ctx, tmp_path, data, schema, **opts):
    with pytest.raises(UnsupportedError, match="needs the host path"):
        DeviceTable.from_csv_bytes(ctx, schema, data, **opts)
    path = _write(tmp_path, data)
    o = datasource.CsvReadOptions(**{k: v for k, v in opts.items() if k in ("has_header", "delimiter", "quote", "escape")})
    try:
        host = datasource.read_csv(path, o, schema, 4096, device=False)
    except Exception as e:
        with pytest.raises(type(e)) as got:
            datasource.read_csv(path, o, schema, 4096, device=True)
        assert str(got.value) == str(e)
        return
    t = datasource.read_csv(path, o, schema, 4096, device=True)
    assert t.decoded_on_device is False and type(t) is type(host)
    _assert_same(t.data, t.schema(), host, decoded=False)


@pytest.mark.parametrize("case", range(len(FIELD_REASONS)))
def test_needs_host_field_spellings(ctx, tmp_path, case):
    t, bad = FIELD_REASONS[case]
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("v", t)])
    good = GOOD[t].encode()
    bad = bad if isinstance(bad, bytes) else bad.encode()
    for where in (0, 9999):                                   # in the first and in the last record of 10 000
        lines = [b"%d,%s" % (k, bad if k == where else good) for k in range(10000)]
        _check_needs_host(ctx, tmp_path, b"k,v\n" + b"\n".join(lines) + b"\n", schema)


STRUCTURE = ["short", "long", "empty_line", "bom", "empty_file", "header_names", "escape", "boolean"]


@pytest.mark.parametrize("what", STRUCTURE)
def test_needs_host_structure(ctx, tmp_path, what):
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("v", pa.string())])
    for where in (0, 9999):
        lines = [b"%d,v%d" % (k, k) for k in range(10000)]
        data, opts = None, {}
        if what == "short":
            lines[where] = b"%d" % where
        elif what == "long":
            lines[where] += b",x"
        elif what == "empty_line":
            lines[where] += b"\n"
        data = b"k,v\n" + b"\n".join(lines) + b"\n"
        if what == "bom":
            data = b"\xef\xbb\xbf" + data
        elif what == "empty_file":
            data = b""
        elif what == "header_names":
            data = b"k,w" + data[3:]
        elif what == "escape":
            opts = {"escape": "\\"}
        elif what == "boolean":
            schema = pa.schema([pa.field("k", pa.int64()), pa.field("v", pa.bool_())])
            data = b"k,v\n" + b"\n".join(b"%d,true" % k for k in range(10000)) + b"\n"
        _check_needs_host(ctx, tmp_path, data, schema, **opts)


def test_bit_exact_values(ctx):
    rng = random.Random(5)
    floats = []
    for _ in range(50000):
        digits = str(rng.randint(0, 2 ** 53))               # m <= 2^53
        frac = rng.randint(0, len(digits) - 1)
        if frac:
            digits = digits[:-frac] + "." + digits[-frac:]
        e = rng.randint(-22, 22)                             # the effective power of ten
        floats.append(("-" if rng.random() < 0.3 else "") + digits + ("" if e + frac == 0 else "e%d" % (e + frac)))
    data = ("f\n" + "\n".join(floats) + "\n").encode()
    dev = DeviceTable.from_csv_bytes(ctx, pa.schema([pa.field("f", pa.float64())]), data)
    got = pa.Table.from_batches(dev.to_batches())["f"].combine_chunks().to_numpy().view(np.uint64)
    assert np.array_equal(got, np.array([float(f) for f in floats]).view(np.uint64))
    # integer limits of every width
    ints = TYPES[:8]
    lim = [((-(1 << (t.bit_width - 1)), (1 << (t.bit_width - 1)) - 1) if pa.types.is_signed_integer(t) else (0, (1 << t.bit_width) - 1)) for t in ints]
    data = (",".join(NAMES[:8]) + "\n" + ",".join(str(a) for a, _ in lim) + "\n" + ",".join(str(b) for _, b in lim) + "\n").encode()
    dev = DeviceTable.from_csv_bytes(ctx, pa.schema([pa.field(n, t) for n, t in zip(NAMES, ints)]), data)
    got = pa.Table.from_batches(dev.to_batches())
    assert [got[k].to_pylist() for k in range(8)] == [[a, b] for a, b in lim]
    # every 97th day of the date range
    days = list(range(1, 3652060, 97))
    data = ("d\n" + "\n".join(datetime.date.fromordinal(o).isoformat() for o in days)).encode()
    dev = DeviceTable.from_csv_bytes(ctx, pa.schema([pa.field("d", pa.date32())]), data)
    got = pa.Table.from_batches(dev.to_batches())["d"].cast(pa.int32()).to_pylist()
    assert got == [o - 719163 for o in days]


def test_past_4_gib_of_text(ctx):
    """the smallest input at which a 32-bit byte offset goes wrong: a 1 MiB block of short records repeated to ~4.3 GB"""
    rng = random.Random(9)
    lines, a, b = [], [], []
    size = 0
    while True:
        x, y = rng.randint(-10 ** 9, 10 ** 9), rng.randint(0, 10 ** 9)
        ln = "%d,%d,%s\n" % (x, y, rng.choice(["ab", "cd", "ef"]))
        if size + len(ln) > (1 << 20) - 40:
            break
        lines.append(ln); a.append(x); b.append(y); size += len(ln)
    pad = (1 << 20) - size                                   # the block is exactly 1 MiB: one last record padded with zeros
    x, y = 7, 11
    ln = "%s,%d,zz\n" % (str(x).rjust(pad - 7, "0"), y)
    assert len(ln) == pad
    lines.append(ln); a.append(x); b.append(y)
    block = "".join(lines).encode()
    assert len(block) == 1 << 20
    reps = 4100
    data = block * reps
    assert len(data) - 1000 * 64 > 1 << 32                   # (the last 1 000 records lie wholly behind byte 2^32)
    schema = pa.schema([pa.field("a", pa.int64()), pa.field("b", pa.int64()), pa.field("s", pa.string())])
    dev = DeviceTable.from_csv_bytes(ctx, schema, data, has_header=False, batch_rows=1 << 24)
    del data
    n = len(lines)
    assert dev.num_rows == n * reps
    assert dev.column_bytes(2) == (n * reps + 1) * 4 + 2 * n * reps
    t = datasource.DeviceCsvTable(schema, dev)
    i64 = pa.int64()
    aggs = [CountAggregateExpr(Column("a", 0)), SumAggregateExpr(Column("a", 0), i64), MinAggregateExpr(Column("a", 0), i64), MaxAggregateExpr(Column("a", 0), i64),
            CountAggregateExpr(Column("b", 1)), SumAggregateExpr(Column("b", 1), i64), MinAggregateExpr(Column("b", 1), i64), MaxAggregateExpr(Column("b", 1), i64),
            CountAggregateExpr(Column("s", 2))]
    out_schema = pa.schema([pa.field("c%d" % k, i64) for k in range(len(aggs))])
    got = NoGroupingAggregate(out_schema, Scan(schema, t, None, None), aggs).execute()
    row = [c.to_pylist()[0] for c in got[0].columns]
    assert row == [n * reps, sum(a) * reps, min(a), max(a), n * reps, sum(b) * reps, min(b), max(b), n * reps]
    tail = Limit(Scan(schema, t, None, None), 1000, n * reps - 1000).execute()
    tail = pa.Table.from_batches(tail)
    assert tail["a"].to_pylist() == a[-1000:] and tail["b"].to_pylist() == b[-1000:]
    assert tail["s"].to_pylist() == [ln.rsplit(",", 1)[1][:-1] for ln in lines[-1000:]]


def test_q1_mini_over_a_device_decoded_lineitem(ctx, oracle, tmp_path):
    tbl = pa.Table.from_batches(synth.lineitem(200_000, 65_536))
    path = str(tmp_path / "lineitem.csv")
    pacsv.write_csv(tbl, path, write_options=pacsv.WriteOptions(quoting_style="none"))
    schema = pa.schema([pa.field(f.name, f.type) for f in synth.LINEITEM_SCHEMA])
    t = datasource.read_csv(path, schema=schema, batch_rows=65_536, device=True)
    assert t.decoded_on_device and t.device_table().num_rows == 200_000
    plan = queries.q1_mini(t)
    got = sorted(tuple(r) for b in plan.execute() for r in zip(*[c.to_pylist() for c in b.columns]))
    assert t._data is None                                     # the query ran on the decoded table; nothing was downloaded
    want = sorted(tuple(r) for b in oracle.execute(plan) for r in zip(*[c.to_pylist() for c in b.columns]))   # (reads t.data)
    assert got == want and len(got) >= 2
    assert pa.Table.from_batches(t.data).equals(tbl.cast(schema))
