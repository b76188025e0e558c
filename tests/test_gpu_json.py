"""The device decoder for newline-delimited JSON (qhip_table_from_json; csrc/json.cpp, k_json_decode, k_json_copy_utf8; DESIGN
§3.10) against the host path — `datasource.read_json(device=False)`, Arrow C++ with the same explicit schema — over the same
bytes, compared exactly: schema, values, validity, no validity buffer without NULLs, batch split. A file outside the grammar answers
UnsupportedError at the low level and comes back from `read_json(device=True)` as the host path's table or the host path's error.
Every input is well formed for the walk; a needs-host input is a normal return."""
import datetime
import decimal
import io
import json
import random

import numpy as np
import pyarrow as pa
import pyarrow.json as pajson
import pytest

from qurious_amd import datasource
from qurious_amd._ffi import DeviceTable, UnsupportedError
from qurious_amd.expr import Column, CountAggregateExpr, MaxAggregateExpr, SumAggregateExpr
from qurious_amd.plan import HashAggregate, Scan

pytestmark = pytest.mark.gpu

DEC = pa.decimal128(15, 2)
TS_US = pa.timestamp("us")


def _write(tmp_path, data, name="t.json"):
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


def _same_as_host(tmp_path, data, schema, batch_rows=None, columns=None):
    path = _write(tmp_path, data)
    host = datasource.read_json(path, batch_rows, schema, columns, device=False)
    dev = datasource.read_json(path, batch_rows, schema, columns, device=True)
    assert dev.decoded_on_device is True and host.decoded_on_device is False
    _assert_same(dev.data, dev.schema(), host)
    return pa.Table.from_batches(dev.data, schema=dev.schema())


def _host_table(data, schema):
    return pajson.read_json(io.BytesIO(data), parse_options=pajson.ParseOptions(explicit_schema=schema)).combine_chunks()


WORDS = ["", "a", "x,y", 'say \\"hi\\"', '\\"', "\\\\", "ä€\U0001f600", "line\\nbreak, tab\\there", "plain words", "{\\/}", "c:\\\\dir\\\\file", "[1,2]"]

SCHEMA = pa.schema([pa.field("k", pa.int64()), pa.field("i", pa.int32()), pa.field("d", pa.date32()), pa.field("m", DEC), pa.field("f", pa.float64()),
                    pa.field("b", pa.bool_()), pa.field("t", TS_US), pa.field("s", pa.string()), pa.field("c", pa.string())])


def _records(n, seed, schema=SCHEMA):
    """n lineitem-like records: every type, NULLs by `null` and by a missing key, shuffled keys, blanks between tokens"""
    rng = random.Random(seed)
    base = datetime.datetime(1995, 1, 1)
    recs = []
    for k in range(n):
        vals = {
            "k": str(k),
            "i": str(rng.randint(-2 ** 31, 2 ** 31 - 1)),
            "d": str(rng.randint(0, 20000)),
            "m": rng.choice(["%d.%02d", '"%d.%02d"']) % (rng.randint(-10 ** 9, 10 ** 9), rng.randint(0, 99)),
            "f": repr(rng.randint(-10 ** 6, 10 ** 6) / 4.0),
            "b": rng.choice(["true", "false"]),
            "t": '"%s"' % (base + datetime.timedelta(microseconds=rng.randint(0, 10 ** 15))).isoformat(sep=rng.choice(" T")),
            "s": '"%s"' % rng.choice(WORDS),
            "c": '"%s"' % ", ".join(rng.choice(WORDS) for _ in range(rng.randint(0, 4))),
        }
        keys = [f.name for f in schema]
        if rng.random() < 0.3:
            rng.shuffle(keys)
        pairs = []
        for name in keys:
            if name != "k" and rng.random() < 0.1:
                if rng.random() < 0.5:
                    continue
                vals[name] = "null"
            pairs.append('"%s":%s%s' % (name, rng.choice(["", "", " ", "\t"]), vals[name]))
        recs.append("{" + rng.choice([",", ", ", " ,"]).join(pairs) + "}")
    return recs


def test_the_library_exports_the_entry_point(ctx):
    assert hasattr(ctx.lib, "qhip_table_from_json") and hasattr(ctx.lib, "qhip_ctx_json_pass_ms")


def test_a_conforming_file_is_decoded_on_the_device(ctx, tmp_path):
    data = ("\n".join(_records(5000, 1)) + "\n").encode()
    path = _write(tmp_path, data)
    dev = datasource.read_json(path, 1024, SCHEMA, device=True)
    assert dev.decoded_on_device is True
    assert ctx.last_stats()["main_kernel_name"] == "k_json_decode" and ctx.last_stats()["rows_out"] == 5000
    host = datasource.read_json(path, 1024, SCHEMA, device=False)
    assert host.decoded_on_device is False
    _assert_same(dev.data, dev.schema(), host)
    assert set(host.data[0].column("s").to_pylist()) >= {'say "hi"', "\\", "line\nbreak, tab\there"}
    # with every new argument left out: the host read of before, unchanged
    path = _write(tmp_path, b'{"a": 1, "b": "x"}\n{"a": 2, "b": null}\n', "plain.json")
    plain = datasource.read_json(path)
    assert plain.decoded_on_device is False
    assert pa.Table.from_batches(plain.data).equals(pajson.read_json(path).combine_chunks())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_edges_of_lanes_wavefronts_and_vectors(ctx, n):
    schema = pa.schema([SCHEMA.field(name) for name in ("k", "s", "b", "t", "m")])
    recs = _records(n, 200 + n, schema)
    for shift in range(0, 18):
        # blanks in front of the first object: every later record begins 0 to 17 bytes later, on every alignment of a 16-byte load
        for final in (False, True):
            data = (" " * shift + "\n".join(recs) + ("\n" if final else "")).encode()
            dev = DeviceTable.from_json_bytes(ctx, schema, data, batch_rows=100)
            assert dev.num_rows == n and dev.batch_offsets() == list(range(0, n, 100)) + [n]
            assert pa.Table.from_batches(dev.to_batches()).equals(_host_table(data, schema)), (n, shift, final)


def test_boolean_and_validity_words_at_the_64_row_edges(ctx, tmp_path):
    n = 300
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("b", pa.bool_()), pa.field("c", pa.bool_()), pa.field("s", pa.string())])
    special = (63, 64, 127, n - 1)
    # (a column with NULLs has them in every batch of 100: an exported batch carries the column's validity buffer or none)
    for null_at, true_at in ((special, ()), ((), special), ((63, 127, 250), (64, 151, n - 1))):
        rows = []
        for k in range(n):
            b = "null" if k in null_at else ("true" if k in true_at else "false")
            c = '"c":true,' if k % 3 == 0 else ("" if k in true_at else '"c":false,')      # (a missing key is NULL)
            rows.append('{"k":%d,"b":%s,%s"s":"r%d"}' % (k, b, c, k))
        got = _same_as_host(tmp_path, ("\n".join(rows) + "\n").encode(), schema, batch_rows=100)   # (batches cut the bits at 100, 200)
        assert got["b"].to_pylist() == [None if k in null_at else k in true_at for k in range(n)]
        assert got["b"].null_count == len(null_at)


def test_records_across_a_scan_chunk_edge(ctx, tmp_path):
    """the 16 KB chunks of the two scan passes: a line end on the last byte of a chunk, on the first of the next, a "\\r\\n" across it"""
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string())])
    for edge in (16384, 32768):
        for at in (-2, -1, 0, 1):
            for end in ("\n", "\r\n"):
                rows, size, k = [], 0, 0
                while size < edge - 200:
                    rows.append('{"k":%d,"s":"v\\t%d"}' % (k, k))
                    size += len(rows[-1]) + len(end)
                    k += 1
                # the next record's line end (its last byte) lands at file offset edge + at
                head = '{"k":%d,"s":"' % k
                fill = edge + at + 1 - size - len(head) - len('"}') - len(end)
                rows.append(head + "z" * fill + '"}')
                rows += ['{"k":%d,"s":"after"}' % j for j in range(k + 1, k + 50)]
                data = (end.join(rows) + end).encode()
                assert data[edge + at] == 10
                got = _same_as_host(tmp_path, data, schema, batch_rows=64)
                assert got.num_rows == k + 50 and got["s"][k].as_py() == "z" * fill


@pytest.mark.parametrize("total", [48 * 1024 - 1, 48 * 1024, 48 * 1024 + 1])
def test_a_string_at_the_edge_of_the_lds_tile(ctx, tmp_path, total):
    """256 records of `total` bytes from byte 0 of the file: one byte below, at, and one byte above the 48 KB tile"""
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string())])
    rows = ['{"k":%d,"s":"v,%d"}' % (k, k) for k in range(256)]
    size = sum(len(r) + 1 for r in rows)
    fill = total - size
    unit = 'p,\\"'
    rows[100] = '{"k":100,"s":"v,100' + unit * (fill // 4) + "q" * (fill % 4) + '"}'
    first = "\n".join(rows) + "\n"
    assert len(first.encode()) == total
    rest = ['{"k":%d,"s":"w\\"%d"}' % (k, k) for k in range(256, 600)]
    got = _same_as_host(tmp_path, (first + "\n".join(rest) + "\n").encode(), schema, batch_rows=256)
    assert got["s"][100].as_py().startswith('v,100p,"p,"') and got["s"][599].as_py() == 'w"599'


def test_the_200_000_byte_string_with_escapes(ctx, tmp_path):
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string()), pa.field("t", pa.string())])
    unit = "ä€\U0001f600" + "x" * 85 + '\\"' + "\\n"                      # 9 + 85 + 2 + 2 = 98 bytes raw, 96 unescaped
    big = unit * 2040 + "ä" * 39 + "\\\\"                                  # 199 920 + 78 + 2: an escaped backslash in front of the closing quote
    assert len(big.encode()) == 200_000
    rows = ['{"k":%d,"s":"w%d","t":"%s"}' % (k, k, "ü" * (k % 23)) for k in range(300)]
    rows[150] = '{"k":150,"s":"%s","t":"after\\tit"}' % big
    got = _same_as_host(tmp_path, "\n".join(rows).encode(), schema, batch_rows=64)     # (larger than the tile: walked in global memory)
    assert got["s"][150].as_py() == json.loads('"%s"' % big) and got["t"][150].as_py() == "after\tit"


def test_escapes_on_the_64_byte_steps(ctx, tmp_path):
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string())])
    inners = []
    for length in (63, 64, 65, 127, 128, 129, 200):
        for where in sorted({0, 1, 61, 62, 63, 64, 65, 126, 127, 128, length - 2}):   # the introducer's raw offset
            if 0 <= where <= length - 2:
                for esc in ('\\"', "\\\\", "\\n", "\\/"):
                    inners.append("a" * where + esc + "b" * (length - 2 - where))
    for run in (2, 3, 4, 5, 64, 65, 129, 130):                                          # runs of backslashes across the steps
        for lead in (0, 1, 61, 62, 63, 64):
            inners.append("b" * lead + "\\\\" * (run // 2) + ("\\t" if run % 2 else "") + "c" * 70)
    rows = ['{"k":%d,"s":"%s"}' % (k, v) for k, v in enumerate(inners)]
    got = _same_as_host(tmp_path, ("\n".join(rows) + "\n").encode(), schema, batch_rows=64)
    assert got["s"].to_pylist() == [json.loads('"%s"' % v) for v in inners]


GOOD = {"k": "1", "i": "2", "d": "9000", "m": "1.50", "f": "2.5", "b": "true", "t": '"1995-03-15 01:02:03.25"', "s": '"ok"', "c": '"fine"'}
NEEDS_HOST = [
    # (what replaces the record, or (key, value) for one pair of it; what the message names)
    ('{"k":1}\r{"k":2}', "a carriage return that is not followed by a line feed"),      # the splitter's verdicts: the host reads across the
    ("", "an empty line"),                                                                # lone '\\r' and skips the empty line
    ('{"k":1}{"k":2}', "not exactly one complete object"),
    ('{"k":1,"s":"cut', "not exactly one complete object"),
    ('{"k":1,}', "not exactly one complete object"),
    ('{"k":1,"zz":2}', "a key that the schema does not hold"),
    ('{"k":1,"\\u0073":"x"}', "a key with a backslash escape"),
    ('{"k":1,"c":"x","k":2}', "a key that occurs twice"),
    (("c", '{"x":1}'), "a nested object or array"),
    (("c", "[1]"), "a nested object or array"),
    (("c", '"\\u0041"'), "a .u escape"),
    (("c", '"\\q"'), "an unknown backslash escape"),
    (("c", '"a\x01b"'), "a control character"),
    (("c", b'"\xff"'), "invalid UTF-8"),
    (("c", "5"), "another JSON kind"),
    (("b", "1"), "another JSON kind"),
    (("d", '"1995-03-15"'), "another JSON kind"),
    (("i", "1.0"), "an integer"),
    (("i", "2147483648"), "an integer"),
    (("d", "1.5"), "a date"),
    (("f", "0.12345678901234567"), "a float"),
    (("f", "1e400"), "a float"),
    (("m", "1e2"), "a decimal"),
    (("m", '"+1.5"'), "a decimal"),
    (("t", '"1995-03-15"'), "a timestamp"),
    (("t", '"1995-03-15 01:02:03Z"'), "a timestamp"),
]


@pytest.mark.parametrize("case", range(len(NEEDS_HOST)))
def test_needs_host_reasons(ctx, tmp_path, case):
    what, names = NEEDS_HOST[case]
    good = ("{" + ",".join('"%s":%s' % kv for kv in GOOD.items()) + "}").encode()
    if isinstance(what, tuple):
        key, value = what
        value = value if isinstance(value, bytes) else value.encode()
        bad = b"{" + b",".join(b'"%s":%s' % (k.encode(), value if k == key else v.encode()) for k, v in GOOD.items()) + b"}"
        unprojected = [SCHEMA.get_field_index(n) for n in SCHEMA.names if n != key][::-1]
    else:
        bad, unprojected = what.encode(), [0]
    for where in (0, 9999):                                   # in the first and in the last record of 10 000
        lines = [bad if k == where else good for k in range(10000)]
        data = b"\n".join(lines) + b"\n"
        for idx in (None, unprojected):                       # the offending field projected, and not
            with pytest.raises(UnsupportedError, match="JSON needs the host path: .*%s.* in record %d$" % (names, where + 1)):
                DeviceTable.from_json_bytes(ctx, SCHEMA, data, columns=idx)
        path = _write(tmp_path, data)
        cols = [SCHEMA.names[k] for k in unprojected]
        for columns in (None, cols):
            try:
                host = datasource.read_json(path, 4096, SCHEMA, columns, device=False)
            except Exception as e:
                with pytest.raises(type(e)) as got:
                    datasource.read_json(path, 4096, SCHEMA, columns, device=True)
                assert str(got.value) == str(e)
                continue
            got = datasource.read_json(path, 4096, SCHEMA, columns, device=True)
            assert got.decoded_on_device is False and type(got) is type(host)
            _assert_same(got.data, got.schema(), host, decoded=False)


def test_structure_outside_the_grammar(ctx):
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("v", pa.string())])
    for data, names in ((b'{"k":1}\n\n{"k":2}\n', "an empty line in record 2$"), (b'{"k":1}\r{"k":2}\n', "carriage return.* in record 1$"),
                        (b'{"k":1}\n   \n{"k":2}\n', "complete object in record 2$"), (b"", "empty"), (b'\xef\xbb\xbf{"k":1}\n', "byte order mark")):
        with pytest.raises(UnsupportedError, match=names):
            DeviceTable.from_json_bytes(ctx, schema, data)
    # refused before anything is uploaded: a type outside the table, projected or not; too many fields; two fields of one name
    for t in (pa.float32(), pa.time32("s"), pa.decimal256(40, 2), pa.timestamp("us", tz="UTC"), pa.null(), pa.list_(pa.int64()), pa.struct([("x", pa.int64())])):
        for cols in (None, [0]):
            with pytest.raises(UnsupportedError):
                DeviceTable.from_json_bytes(ctx, pa.schema([pa.field("k", pa.int64()), pa.field("v", t)]), b'{"k":1}\n', columns=cols)
    with pytest.raises(UnsupportedError, match="more than 64"):
        DeviceTable.from_json_bytes(ctx, pa.schema([pa.field("f%d" % k, pa.int64()) for k in range(65)]), b'{"f0":1}\n')
    with pytest.raises(UnsupportedError, match="key names"):
        DeviceTable.from_json_bytes(ctx, pa.schema([pa.field("f%d" % k + "x" * 100, pa.int64()) for k in range(20)]), b"{}\n")
    dev = DeviceTable.from_json_bytes(ctx, pa.schema([pa.field("f%02d" % k + "x" * 27, pa.int64()) for k in range(64)]), b'{"f63%s":5}\n{}\n' % (b"x" * 27))
    assert pa.Table.from_batches(dev.to_batches()).column(63).to_pylist() == [5, None]


def test_a_schema_with_a_required_field_stays_with_the_host(ctx, tmp_path):
    """the host refuses a record in which a field that is not nullable is absent or null; on the device both would be NULL"""
    schema = pa.schema([pa.field("a", pa.int64(), nullable=False), pa.field("b", pa.string())])
    for cols in (None, [1]):
        with pytest.raises(UnsupportedError, match="JSON needs the host path: schema field 'a' is not nullable"):
            DeviceTable.from_json_bytes(ctx, schema, b'{"a":1,"b":"x"}\n', columns=cols)
    good = ['{"a":%d,"b":"x"}' % k for k in range(1000)]
    path = _write(tmp_path, ("\n".join(good) + "\n").encode())
    host = datasource.read_json(path, 256, schema, device=False)
    got = datasource.read_json(path, 256, schema, device=True)
    assert got.decoded_on_device is False and type(got) is type(host)
    _assert_same(got.data, got.schema(), host, decoded=False)
    for bad, names in (('{"b":"x"}', "absent"), ('{"a":null,"b":"x"}', "null")):
        for where in (0, 999):
            rows = list(good)
            rows[where] = bad
            path = _write(tmp_path, ("\n".join(rows) + "\n").encode(), "bad.json")
            for columns in (None, ["b"]):
                with pytest.raises(pa.ArrowInvalid, match="a required field was " + names) as want:
                    datasource.read_json(path, 256, schema, columns, device=False)
                with pytest.raises(pa.ArrowInvalid) as got:
                    datasource.read_json(path, 256, schema, columns, device=True)
                assert str(got.value) == str(want.value)


def test_a_projection_in_another_order_than_the_schema(ctx, tmp_path):
    data = ("\n".join(_records(700, 5)) + "\n").encode()
    got = _same_as_host(tmp_path, data, SCHEMA, batch_rows=128, columns=["c", "m", "k", "b", "t"])
    assert got.column_names == ["c", "m", "k", "b", "t"] and got["k"].to_pylist() == list(range(700))
    got = _same_as_host(tmp_path, data, SCHEMA, batch_rows=128, columns=["f"])
    assert got.column_names == ["f"]
    # an unprojected value is still validated: the host refuses the file for it
    bad = data + b'{"k":1,"i":1.5}\n'
    with pytest.raises(UnsupportedError, match="an integer.* in record 701$"):
        DeviceTable.from_json_bytes(ctx, SCHEMA, bad, columns=[0])


def test_inferred_schema_on_a_conforming_file(ctx, tmp_path):
    def rows(d):
        return ['{"k":%d,"b":%s,"t":"1995-03-15 01:02:%02d","d":"%s","f":%d.5,"s":"n, \\"%d\\""}' % (k, "true" if k % 2 else "false", k % 60, d % (1 + k % 28), k, k)
                for k in range(300)]

    inferred = [pa.int64(), pa.bool_(), pa.timestamp("s"), pa.timestamp("s"), pa.float64(), pa.string()]
    path = _write(tmp_path, ("\n".join(rows("2001-01-%02dT00:00:00")) + "\n").encode())
    host = datasource.read_json(path, batch_rows=128, device=False)
    assert [f.type for f in host.schema()] == inferred
    dev = datasource.read_json(path, batch_rows=128, device=True)
    assert dev.decoded_on_device is True
    _assert_same(dev.data, dev.schema(), host)
    # a date-shaped column is Timestamp(s) by inference too, but its date-only spelling needs the host
    path = _write(tmp_path, ("\n".join(rows("2001-01-%02d")) + "\n").encode(), "d.json")
    host = datasource.read_json(path, batch_rows=128, device=False)
    assert [f.type for f in host.schema()] == inferred
    dev = datasource.read_json(path, batch_rows=128, device=True)
    assert dev.decoded_on_device is False
    _assert_same(dev.data, dev.schema(), host, decoded=False)
    # a column that is null in every record of the first block has type null: the device path is refused
    path = _write(tmp_path, b'{"k":1,"z":null}\n{"k":2,"z":null}\n', "n.json")
    dev = datasource.read_json(path, device=True)
    assert dev.decoded_on_device is False and dev.schema().field("z").type == pa.null()


def test_inferred_schema_on_a_two_block_file(ctx, tmp_path):
    """60 000 conforming records (more than Arrow's first block of 1 MB), then one whose value changes a column's type and that
    holds a new key: the strict decode fails on it and the result is the host's whole-file result"""
    rows = ['{"k":%d,"b":true,"s":"r"}' % k for k in range(60000)]
    data = ("\n".join(rows) + "\n").encode()
    assert len(data) > (1 << 20) + 200_000
    path = _write(tmp_path, data)
    with pajson.open_json(path) as rd:
        first = rd.schema
    assert [f.type for f in first] == [pa.int64(), pa.bool_(), pa.string()]
    dev = datasource.read_json(path, 1 << 14, device=True)
    assert dev.decoded_on_device is True
    _assert_same(dev.data, dev.schema(), datasource.read_json(path, 1 << 14, device=False))
    path = _write(tmp_path, data + b'{"k":1.5,"b":false,"s":"x","extra":7}\n', "two.json")
    host = datasource.read_json(path, 1 << 14, device=False)
    assert [f.type for f in host.schema()] == [pa.float64(), pa.bool_(), pa.string(), pa.int64()]
    with pytest.raises(UnsupportedError, match="an integer.* in record 60001$"):
        with open(path, "rb") as f:
            DeviceTable.from_json_bytes(ctx, first, f.read())
    dev = datasource.read_json(path, 1 << 14, device=True)
    assert dev.decoded_on_device is False
    _assert_same(dev.data, dev.schema(), host, decoded=False)


def test_a_query_over_a_decoded_file_against_the_oracle(ctx, oracle, tmp_path):
    n = 20000
    rng = random.Random(3)
    base = datetime.datetime(1995, 1, 1)
    schema = pa.schema([pa.field("g", pa.string()), pa.field("m", DEC), pa.field("b", pa.bool_()), pa.field("t", TS_US)])
    rows = []
    for _ in range(n):
        g = rng.choice(["a,b", 'q\\"r', "plain", ""])
        m = "null" if rng.random() < 0.05 else "%d.%02d" % (rng.randint(-10 ** 6, 10 ** 6), rng.randint(0, 99))
        b = rng.choice(["true", "false", "null"])
        t = "null" if rng.random() < 0.05 else '"%s"' % (base + datetime.timedelta(microseconds=rng.randint(1, 10 ** 15))).isoformat(sep=" ")
        rows.append('{"g":"%s","m":%s,"b":%s,"t":%s}' % (g, m, b, t))
    path = _write(tmp_path, ("\n".join(rows) + "\n").encode())
    host = datasource.read_json(path, 4096, schema, device=False)
    dev = datasource.read_json(path, 4096, schema, device=True)
    assert dev.decoded_on_device is True

    def plan(table):
        aggs = [SumAggregateExpr(Column("m", 1), DEC), CountAggregateExpr(Column("m", 1)), MaxAggregateExpr(Column("t", 3), TS_US)]
        return HashAggregate(None, Scan(schema, table, None, Column("b", 2)), [Column("g", 0)], aggs)

    def rows_of(batches):
        return sorted(tuple(r) for b in batches for r in zip(*[c.to_pylist() for c in b.columns]))

    got = rows_of(plan(dev).execute())
    assert dev._data is None                                    # the query ran on the decoded table; nothing was downloaded
    want = rows_of(oracle.execute(plan(host)))
    assert got == want and len(got) == 4
    tbl = pa.Table.from_batches(host.data)
    keep = [i for i, b in enumerate(tbl["b"].to_pylist()) if b]
    assert sum(r[2] for r in got) == sum(1 for i in keep if tbl["m"][i].as_py() is not None)
    assert sum(r[1] for r in got) == sum((tbl["m"][i].as_py() or decimal.Decimal(0)) for i in keep)
    assert max(r[3] for r in got) == max(tbl["t"][i].as_py() for i in keep if tbl["t"][i].as_py() is not None)
