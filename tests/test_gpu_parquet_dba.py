"""The DELTA_BYTE_ARRAY switch of the device Parquet decoder (qhip_ctx_set_parquet_delta_byte_array(ctx, 1); k_pq_delta_dba,
k_pq_dba_copy, k_pq_dba_fill): Utf8 and FIXED_LEN_BYTE_ARRAY decimal columns written with DELTA_BYTE_ARRAY against
the host path on the same bytes, compared exactly as tests/test_gpu_parquet.py compares — and every positive case must have
been decoded on the device, so that a silent fallback cannot pass. Raw value streams go through qhip_parquet_dba_decode, good
and hostile ones side by side in one call, against the CPU model of tests/test_parquet_dba_cpu.py (each has passed the
sanitizers there). No stream here makes a kernel do what its checks exist to prevent: a hostile one is refused before the access."""
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from qurious_amd import datasource, queries, synth
from qurious_amd._ffi import DeviceTable, UnsupportedError
from tests.test_gpu_parquet import _assert_same
from tests.test_parquet_cpu import FLAGS, _null_patterns
from tests.test_parquet_dba_cpu import (DBA, KEY_WRITE, SOURCE, cpu_model_dba, good_dba_streams, hostile_dba_streams, key_table, null_patterns, shape_columns,
                                        shape_table)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def switched_on(ctx):
    """the switch, encoding set 2 and format level 2 for the test, the defaults behind it: the context is the process's"""
    ctx.set_parquet_delta_byte_array(1)
    ctx.set_parquet_encodings(2)
    ctx.set_parquet_format(2)
    yield ctx
    ctx.set_parquet_delta_byte_array(0)
    ctx.set_parquet_encodings(1)
    ctx.set_parquet_format(1)


def _both(tmp_path, tbl, batch_rows=1000, columns=None, name="t.parquet", **kw):
    path = str(tmp_path / name)
    kw.setdefault("compression", "NONE")
    kw.setdefault("use_dictionary", False)
    pq.write_table(tbl, path, **kw)
    host = datasource.read_parquet(path, columns, batch_rows, device=False)
    dev = datasource.read_parquet(path, columns, batch_rows, device=True)
    return dev, host, path


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 130, 1000, 20_001])
def test_row_counts_and_null_patterns_with_pages_that_end_inside_steps(ctx, tmp_path, n):
    """data_page_size=4096: pages end inside 64-row steps and the prefix restarts; write batches of 50 rows put the first row
    of every page on a multiple of 50, where "first of a page" has its NULLs"""
    patterns = null_patterns(n, page_rows=range(0, n, 50))
    for name in ("none", "first of a page", "seventh", "all but one", "random"):
        for version in ("1.0", "2.0"):
            dev, host, path = _both(tmp_path, key_table(n, patterns[name]), data_page_version=version, data_page_size=4096, write_batch_size=50, **KEY_WRITE)
            _assert_same(dev, host)
            assert dev.decoded_on_device and dev.device_table().num_rows == n, (name, version)
    md = pq.ParquetFile(path).metadata.row_group(0)
    assert all(DBA in md.column(c).encodings for c in range(3))
    if n == 20_001:
        assert md.column(0).total_compressed_size > 3 * 4096           # (more than one page, so a prefix restarted)


@pytest.mark.parametrize("shape", list(shape_columns()))
def test_shapes_of_values(ctx, tmp_path, shape):
    """a constant column (every byte traces back to row 0 across 15 steps), sorted keys, the empty string, equal neighbours,
    strict prefixes, prefixes of exactly 64 and 65 bytes, and two 200 000-byte strings that share 150 000 bytes"""
    for nulls in (None, lambda n: np.arange(n) % 7 == 3, lambda n: np.arange(n) % 64 == 0):
        tbl = shape_table(shape, nulls)
        for kw in (dict(data_page_version="1.0"), dict(data_page_version="2.0", data_page_size=4096), dict(data_page_version="2.0", compression="snappy")):
            dev, host, path = _both(tmp_path, tbl, batch_rows=300, column_encoding={"s": DBA}, **kw)
            _assert_same(dev, host)
            assert dev.decoded_on_device and DBA in pq.ParquetFile(path).metadata.row_group(0).column(0).encodings


def test_decimals_next_to_delta_integers_and_a_dictionary_column_and_projections(ctx, tmp_path):
    n = 3000
    tbl = key_table(n, _null_patterns(n)["random"])
    assert tbl.schema.field("m15").type == pa.decimal128(15, 2) and tbl.schema.field("m38").type == pa.decimal128(38, 4)
    assert min(tbl["m15"].drop_null().to_pylist()) < 0 and min(tbl["m38"].drop_null().to_pylist()) < 0 and tbl["m38"].null_count > 0
    for kw in (dict(data_page_version="1.0"), dict(data_page_version="2.0", data_page_size=4096), dict(data_page_version="2.0", compression="snappy", row_group_size=700)):
        for columns in (None, ["i64", "tag"], ["key"], ["m38"], ["m15", "tag", "key"]):
            dev, host, path = _both(tmp_path, tbl, columns=columns, **dict(KEY_WRITE, **kw))
            _assert_same(dev, host)
            assert dev.decoded_on_device and (columns is None or dev.schema().names == columns)
    md = pq.ParquetFile(path).metadata
    assert md.schema.column(1).physical_type == md.schema.column(2).physical_type == "FIXED_LEN_BYTE_ARRAY"
    assert "RLE_DICTIONARY" in md.row_group(0).column(4).encodings and "DELTA_BINARY_PACKED" in md.row_group(0).column(3).encodings


def test_q1_aggregates_over_a_device_decoded_v2_snappy_delta_byte_array_lineitem(ctx, tmp_path):
    tbl = pa.Table.from_batches(synth.lineitem(6000, 2048))

    def encoding(t):
        if pa.types.is_integer(t) or pa.types.is_date32(t):
            return "DELTA_BINARY_PACKED"
        return DBA if pa.types.is_string(t) or pa.types.is_decimal(t) else None
    enc = {f.name: encoding(f.type) for f in tbl.schema if encoding(f.type)}
    assert DBA in enc.values()
    dev, host, path = _both(tmp_path, tbl, batch_rows=2048, name="lineitem.parquet", data_page_size=4096, data_page_version="2.0", compression="snappy",
                            column_encoding=enc)
    assert dev.decoded_on_device and dev.device_table().num_rows == 6000
    rows = lambda t: sorted(tuple(r) for b in queries.q1_full(t).execute() for r in zip(*[c.to_pylist() for c in b.columns]))     # noqa: E731
    got = rows(dev)
    assert dev._data is None                     # the query ran on the decoded table; nothing was downloaded
    assert got == rows(host) and len(got) >= 2


def test_the_switch_is_a_switch_of_the_context(ctx, tmp_path):
    """the file of test_what_still_needs_the_host_at_set_2: off it answers as it always did, on it is decoded on the device"""
    tbl = pa.table({"s": pa.array(["v%d" % (v % 9) for v in range(1000)])})
    path = str(tmp_path / "f.parquet")
    pq.write_table(tbl, path, compression="NONE", use_dictionary=False, column_encoding={"s": DBA})
    data = open(path, "rb").read()
    host = datasource.read_parquet(path, None, 300, device=False)
    ctx.set_parquet_delta_byte_array(0)
    dev = datasource.read_parquet(path, None, 300, device=True)
    assert dev.decoded_on_device is False and pa.Table.from_batches(dev.data).equals(pa.Table.from_batches(host.data))
    with pytest.raises(UnsupportedError, match="value encoding"):
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, data)
    for bad in (2, -1):
        with pytest.raises(Exception):
            ctx.set_parquet_delta_byte_array(bad)
    with pytest.raises(UnsupportedError, match="value encoding"):        # (a refused value leaves the switch as it was)
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, data)
    ctx.set_parquet_delta_byte_array(1)
    for bad in (2, -1):
        with pytest.raises(Exception):
            ctx.set_parquet_delta_byte_array(bad)
    _assert_same(datasource.read_parquet(path, None, 300, device=True), host)
    assert ctx.last_stats()["rows_out"] == 1000
    # a data page V1 needs nothing but the switch; a data page V2 still needs encoding set 2
    ctx.set_parquet_encodings(1)
    assert pa.Table.from_batches(DeviceTable.from_parquet_bytes(ctx, tbl.schema, data).to_batches()).equals(tbl)
    path2 = str(tmp_path / "f2.parquet")
    pq.write_table(tbl, path2, compression="NONE", use_dictionary=False, column_encoding={"s": DBA}, data_page_version="2.0")
    with pytest.raises(UnsupportedError, match="data page V2"):
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, open(path2, "rb").read())
    ctx.set_parquet_encodings(2)
    assert pa.Table.from_batches(DeviceTable.from_parquet_bytes(ctx, tbl.schema, open(path2, "rb").read()).to_batches()).equals(tbl)


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("dba_model")
    exe = str(d / "parquet_dba_tests")
    subprocess.check_call(["g++"] + FLAGS + ["-O1", "-o", exe, SOURCE])
    return {"plain": exe, "dir": d}


def test_raw_streams_good_and_hostile_side_by_side(ctx, tmp_path, cpu_model):
    good, hostile = good_dba_streams(), hostile_dba_streams()
    names = [("good", k) for k in good] + [("hostile", k) for k in hostile]
    order = np.random.default_rng(1).permutation(len(names))
    names = [names[k] for k in order]                                     # refused streams between decoded ones
    streams = [good[k][:3] if kind == "good" else hostile[k][:3] for kind, k in names]
    want = cpu_model_dba(cpu_model["plain"], cpu_model["dir"], streams)
    values, statuses = ctx.dba_decode([s for s, _, _ in streams], [w for _, w, _ in streams], [c for _, _, c in streams])
    for (kind, name), w, vals, status in zip(names, want, values, statuses):
        if kind == "good":
            assert status == 0 and vals == w == good[name][3], (name, status)
        else:
            assert status == w == hostile[name][3] and vals is None, (name, status, w)
    # afterwards a good file still decodes on the same context
    dev, host, _ = _both(tmp_path, key_table(2000, _null_patterns(2000)["seventh"]), data_page_version="2.0", data_page_size=4096, **KEY_WRITE)
    _assert_same(dev, host)


def test_a_page_damaged_in_place_is_refused_and_the_context_stays_good(ctx, tmp_path):
    """the first prefix length of a page set to 1 (what a writer that does not reset at a page would leave): the host's business"""
    from tests.test_parquet_cpu import _pages
    tbl = pa.table([pa.array(["customer#%09d" % k for k in range(300)])], schema=pa.schema([pa.field("s", pa.string(), nullable=False)]))
    path = str(tmp_path / "first.parquet")
    pq.write_table(tbl, path, compression="NONE", use_dictionary=False, column_encoding={"s": DBA})
    data, pages = _pages(path, 0)
    at = pages[0]["payload"]
    assert data[at:at + 5] == bytes([0x80, 0x01, 0x04, 0xAC, 0x02]) and data[at + 5] == 0       # block 128, 4 miniblocks, 300 values, a first prefix of 0
    with pytest.raises(UnsupportedError, match="DELTA_BYTE_ARRAY prefix"):
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, data[:at + 5] + b"\x02" + data[at + 6:])
    assert pa.Table.from_batches(DeviceTable.from_parquet_bytes(ctx, tbl.schema, data).to_batches()).equals(tbl)
