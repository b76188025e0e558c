"""Parquet files decoded on the device (qhip_table_from_parquet) against the host path on the same bytes:
`read_parquet(device=True)` must return what `read_parquet(device=False)` returns — schema, values, validity, NULL counts and
batch split — or fall back to it."""
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from qurious_amd import datasource, queries, synth
from qurious_amd._ffi import DeviceTable, UnsupportedError
from tests.test_parquet_cpu import DEC_PRECISIONS, LAYOUTS, _null_patterns, _pages, _typed_table, damaged_files, hostile_table

pytestmark = pytest.mark.gpu


def _bits(col, width):
    return pa.compute.fill_null(col, 0.0).to_numpy(zero_copy_only=False).view(width)


def _assert_same(dev, host):
    assert dev.decoded_on_device is True and host.decoded_on_device is False
    assert dev.schema() == host.schema()
    assert dev.schema().metadata == host.schema().metadata
    got, want = dev.device_table().to_batches(), host.data
    assert [b.num_rows for b in got] == [b.num_rows for b in want]
    nulls = [sum(b.column(k).null_count for b in want) for k in range(len(host.schema()))]
    for a, b in zip(got, want):
        assert a.schema == b.schema
        for ca, cb, f, column_nulls in zip(a.columns, b.columns, a.schema, nulls):
            assert ca.null_count == cb.null_count, f.name
            if not pa.types.is_floating(f.type):            # (a NaN equals nothing: floats are compared by their bits below)
                assert ca.equals(cb), f.name
            if column_nulls == 0:
                assert ca.buffers()[0] is None, f.name      # no NULLs, no validity buffer — as after an upload
            assert ca.is_valid().equals(cb.is_valid()), f.name
            if pa.types.is_floating(f.type):
                width = np.uint32 if pa.types.is_float32(f.type) else np.uint64
                assert np.array_equal(_bits(ca, width), _bits(cb, width)), f.name


def _both(tmp_path, tbl, batch_rows=1000, columns=None, name="t.parquet", **kw):
    path = str(tmp_path / name)
    kw.setdefault("compression", "NONE")
    pq.write_table(tbl, path, **kw)
    host = datasource.read_parquet(path, columns, batch_rows, device=False)
    dev = datasource.read_parquet(path, columns, batch_rows, device=True)
    return dev, host, path


def _rows_table(n):
    k = np.arange(n)
    nulls = k % 7 == 3
    return pa.table({"i": pa.array(k.astype(np.int32) - 5, mask=nulls), "b": pa.array(k % 3 == 0, mask=k % 11 == 0), "s": pa.array(["s%d" % (v % 50) for v in k], mask=nulls),
                     "r": pa.array(k * 3, pa.int64())})


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 20_000, 20_001, 50_001])
def test_row_counts_at_the_edges_of_words_pages_and_row_groups(ctx, tmp_path, n, layout):
    dev, host, path = _both(tmp_path, _rows_table(n), batch_rows=1000, **LAYOUTS[layout])
    _assert_same(dev, host)
    assert dev.device_table().num_rows == n


@pytest.mark.parametrize("pattern", ["none", "all", "seventh", "random", "runs"])
def test_null_patterns_on_every_kind_of_column(ctx, tmp_path, pattern):
    n = 3000
    tbl = _typed_table(n, _null_patterns(n)[pattern])
    for layout in LAYOUTS:
        for dictionary in (True, False):
            dev, host, _ = _both(tmp_path, tbl, batch_rows=None, use_dictionary=dictionary, **layout)
            _assert_same(dev, host)
            got = dev.device_table().to_batches()[0]
            for name in ("b", "i32"):           # Boolean and validity words at the 64-row edges, bit by bit
                col, want = got.column(name), tbl.column(name).combine_chunks()
                for edge in range(64, n, 64 * 9):
                    assert col.slice(edge - 2, 4).to_pylist() == want.slice(edge - 2, 4).to_pylist(), (name, edge)


@pytest.mark.parametrize("entries", [2, 3, 256, 257, 65537])
def test_dictionary_index_widths(ctx, tmp_path, entries):
    n = entries + 3000
    rng = np.random.default_rng(entries)
    idx = np.concatenate([np.arange(entries), rng.integers(0, entries, n - entries)])
    mask = np.concatenate([np.zeros(entries, dtype=bool), rng.random(n - entries) < 0.1])
    order = rng.permutation(n)
    idx, mask = idx[order], mask[order]
    tbl = pa.table({"k": pa.array(idx * 7 - 3, pa.int64(), mask=mask), "s": pa.array(["v%06d" % i for i in idx], pa.string(), mask=mask)})
    dev, host, path = _both(tmp_path, tbl)
    assert _pages(path, 0)[1][0]["h"][7][1][0] == entries
    _assert_same(dev, host)


def test_the_dictionary_fallback_in_the_middle_of_a_chunk(ctx, tmp_path):
    n = 100_000
    tbl = pa.table({"s": pa.array(["%040d" % (k * 2654435761 % 10 ** 30) for k in range(n)], pa.string(), mask=np.arange(n) % 11 == 0)})
    dev, host, path = _both(tmp_path, tbl, batch_rows=1 << 20)
    assert {pg["h"][5][2][0] for pg in _pages(path, 0)[1] if 5 in pg["h"]} == {0, 8}
    _assert_same(dev, host)


def test_a_long_string_and_a_required_column(ctx, tmp_path):
    big = "".join(chr(97 + k % 26) for k in range(200_000))
    for dictionary in (True, False):
        dev, host, _ = _both(tmp_path, pa.table({"s": ["a", big, None, "b", big[:70000]]}), use_dictionary=dictionary)
        _assert_same(dev, host)
    n = 1500
    k = np.arange(n)
    schema = pa.schema([pa.field("r", pa.int64(), nullable=False), pa.field("o", pa.int64()), pa.field("rs", pa.string(), nullable=False),
                        pa.field("rb", pa.bool_(), nullable=False)])
    tbl = pa.table([pa.array(k * 3), pa.array(k, mask=k % 4 == 0), pa.array(["s%d" % v for v in k]), pa.array(k % 2 == 0)], schema=schema)
    for layout in LAYOUTS:
        dev, host, _ = _both(tmp_path, tbl, **layout)
        _assert_same(dev, host)
        assert not dev.schema().field("r").nullable


def _every_type():
    def ints(t, lo, hi):
        return pa.array([lo, hi, 0, None, 1, -1 if lo < 0 else 2, lo + 1, hi - 1] * 40, t)
    cols = {"i8": ints(pa.int8(), -128, 127), "i16": ints(pa.int16(), -2 ** 15, 2 ** 15 - 1), "i32": ints(pa.int32(), -2 ** 31, 2 ** 31 - 1),
            "i64": ints(pa.int64(), -2 ** 63, 2 ** 63 - 1), "u8": ints(pa.uint8(), 0, 255), "u16": ints(pa.uint16(), 0, 65535),
            "u32": ints(pa.uint32(), 0, 2 ** 32 - 1), "u64": ints(pa.uint64(), 0, 2 ** 64 - 1),
            "f32": pa.array([0.0, -0.0, float("inf"), None, float("nan"), 1.5, -3.4028235e38, 1e-45] * 40, pa.float32()),
            "f64": pa.array([0.0, -0.0, float("-inf"), None, float("nan"), 1.5, 1.7976931348623157e308, 5e-324] * 40, pa.float64()),
            "d": pa.array([-719162, 2932896, 0, None, 1, -1, 9131, 20000] * 40, pa.date32()), "b": pa.array([True, False, None, True, True, False, None, False] * 40),
            "s": pa.array(["", "a", None, "ä€\U0001f600", "x" * 70, "nul\x00byte", "", "tab\t"] * 40),
            "ts_s": pa.array([0, 1, None, -1, 2 ** 40, -2 ** 40, 5, 6] * 40, pa.timestamp("s")), "ts_ms": ints(pa.timestamp("ms"), -2 ** 63, 2 ** 63 - 1),
            "ts_us": ints(pa.timestamp("us"), -2 ** 63, 2 ** 63 - 1), "ts_ns": ints(pa.timestamp("ns"), -2 ** 63, 2 ** 63 - 1)}
    for p in DEC_PRECISIONS:
        top = 10 ** p - 1
        vals = [top, -top, 0, None, 1, -1, top // 7, -(top // 3)] * 40
        cols["dec%d" % p] = pa.array([None if v is None else decimal.Decimal(v).scaleb(-(p // 2), context=decimal.Context(prec=100)) for v in vals],
                                     pa.decimal128(p, p // 2))
    return pa.table(cols)


def test_every_supported_type_in_one_file(ctx, tmp_path):
    tbl = _every_type()
    for kw in ({}, {"use_dictionary": False}, {"data_page_size": 64, "write_batch_size": 7}):
        dev, host, _ = _both(tmp_path, tbl, batch_rows=100, **kw)
        _assert_same(dev, host)
    small = tbl.select(["dec2", "dec9", "dec11", "dec18"])
    for dictionary in (True, False):
        dev, host, path = _both(tmp_path, small, store_decimal_as_integer=True, use_dictionary=dictionary)
        assert [pq.ParquetFile(path).schema.column(k).physical_type for k in range(4)] == ["INT32", "INT32", "INT64", "INT64"]
        _assert_same(dev, host)


def test_projection(ctx, tmp_path):
    n = 5000
    k = np.arange(n)
    tbl = pa.table({"i": pa.array(k, mask=k % 5 == 0), "t": pa.array(k, pa.time64("us")), "s": pa.array(["v%d" % (v % 9) for v in k]), "f": pa.array(k / 3.0),
                    "z": pa.array(k, pa.timestamp("us", tz="UTC"))})
    for columns in (["i", "s"], ["f", "i"], ["s"]):
        dev, host, path = _both(tmp_path, tbl, columns=columns)
        _assert_same(dev, host)                  # the unprojected Time and zoned Timestamp columns are not looked at
        assert dev.schema().names == columns and [f.name for f in dev.device_table().to_batches()[0].schema] == columns
    dev, host, _ = _both(tmp_path, tbl, columns=["i"], compression={"i": "NONE", "t": "snappy", "s": "snappy", "f": "zstd", "z": "snappy"})
    _assert_same(dev, host)                      # ... nor is their codec
    dev, host, _ = _both(tmp_path, tbl)          # all of them: the Time column needs the host
    assert dev.decoded_on_device is False


FALLBACKS = {"snappy": (lambda t: t, {"compression": "snappy"}, "compressed"), "v2": (lambda t: t, {"data_page_version": "2.0"}, "data page V2"),
             "list": (lambda t: t.append_column("l", pa.array([[1, 2]] * t.num_rows)), {}, "group, list or map"),
             "zone": (lambda t: t.append_column("z", pa.array(np.arange(t.num_rows), pa.timestamp("us", tz="UTC"))), {}, "column type")}


@pytest.mark.parametrize("what", list(FALLBACKS))
def test_fallback_to_the_host_path(ctx, tmp_path, what):
    make, kw, reason = FALLBACKS[what]
    tbl = make(_rows_table(1000))
    path = str(tmp_path / "f.parquet")
    if what == "snappy":
        pq.write_table(tbl, path)                # pyarrow's defaults
        assert pq.ParquetFile(path).metadata.row_group(0).column(0).compression == "SNAPPY"
    else:
        pq.write_table(tbl, path, compression="NONE", **kw)
    host = datasource.read_parquet(path, None, 300, device=False)
    dev = datasource.read_parquet(path, None, 300, device=True)
    assert dev.decoded_on_device is False and host.decoded_on_device is False
    assert dev.schema() == host.schema() and [b.num_rows for b in dev.data] == [b.num_rows for b in host.data]
    assert pa.Table.from_batches(dev.data).equals(pa.Table.from_batches(host.data))
    with pytest.raises(UnsupportedError, match=reason):
        DeviceTable.from_parquet_bytes(ctx, pq.read_schema(path).remove_metadata(), open(path, "rb").read())


def test_damaged_files_are_refused_and_the_context_stays_good(ctx, tmp_path):
    """the four damaged files of tests/test_parquet_cpu.py (each has passed the sanitizers there): the bounds checks answer"""
    tbl = hostile_table()
    path = str(tmp_path / "hostile.parquet")
    pq.write_table(tbl, path, compression="NONE", data_page_size=300, write_batch_size=50)
    good = open(path, "rb").read()
    texts = {"a dictionary index past the entries": "dictionary index", "a BYTE_ARRAY length past its page": "BYTE_ARRAY length",
             "a levels length past its page": "levels' length", "a run count past num_values": "run counts past"}
    for what, (data, _) in damaged_files(path).items():
        with pytest.raises(UnsupportedError, match=texts[what]):
            DeviceTable.from_parquet_bytes(ctx, tbl.schema, data)
        dev = DeviceTable.from_parquet_bytes(ctx, tbl.schema, good)
        assert pa.Table.from_batches(dev.to_batches()).equals(tbl), what


def test_q1_aggregates_over_a_device_decoded_lineitem(ctx, tmp_path):
    tbl = pa.Table.from_batches(synth.lineitem(6000, 2048))
    dev, host, _ = _both(tmp_path, tbl, batch_rows=2048, name="lineitem.parquet", data_page_size=4096)
    assert dev.decoded_on_device and dev.device_table().num_rows == 6000
    rows = lambda t: sorted(tuple(r) for b in queries.q1_full(t).execute() for r in zip(*[c.to_pylist() for c in b.columns]))
    got = rows(dev)
    assert dev._data is None                     # the query ran on the decoded table; nothing was downloaded
    assert got == rows(host) and len(got) >= 2
