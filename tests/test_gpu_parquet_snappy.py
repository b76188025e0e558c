"""Format level 2 of the device Parquet decoder (qhip_ctx_set_parquet_format(ctx, 2); k_pq_unsnap): Snappy files
against the host path on the same bytes, compared exactly as tests/test_gpu_parquet.py compares — and every positive case must
have been decoded on the device, so that a silent fallback cannot pass. Raw streams go through qhip_snappy_decode, good and
hostile ones side by side in one call, against the CPU model of tests/test_parquet_snappy_cpu.py (each has passed the sanitizers
there)."""
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from qurious_amd import datasource, queries, synth
from qurious_amd._ffi import DeviceTable, UnsupportedError
from tests.test_gpu_parquet import _assert_same, _rows_table
from tests.test_parquet_cpu import FLAGS, LAYOUTS, _null_patterns, _pages, _typed_table
from tests.test_parquet_snappy_cpu import (MIXED_CODECS, SOURCE, cpu_model_results, damaged_snappy_file, good_streams, hostile_streams, snappy_hostile_table)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def level2(ctx):
    """level 2 for the test, the default level behind it: the context is the process's"""
    ctx.set_parquet_format(2)
    yield ctx
    ctx.set_parquet_format(1)


def _both(tmp_path, tbl, batch_rows=1000, columns=None, name="t.parquet", **kw):
    """pyarrow's defaults unless told otherwise: Snappy"""
    path = str(tmp_path / name)
    pq.write_table(tbl, path, **kw)
    host = datasource.read_parquet(path, columns, batch_rows, device=False)
    dev = datasource.read_parquet(path, columns, batch_rows, device=True)
    return dev, host, path


def _codecs(path):
    meta = pq.ParquetFile(path).metadata.row_group(0)
    return [meta.column(k).compression for k in range(meta.num_columns)]


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 20_000, 20_001, 50_001])
def test_pyarrows_defaults_at_the_edges_of_words_pages_and_row_groups(ctx, tmp_path, n, layout):
    dev, host, path = _both(tmp_path, _rows_table(n), **LAYOUTS[layout])
    assert set(_codecs(path)) == {"SNAPPY"}
    _assert_same(dev, host)
    assert dev.device_table().num_rows == n


@pytest.mark.parametrize("pattern", ["none", "all", "seventh", "random", "runs"])
def test_null_patterns_on_every_kind_of_column(ctx, tmp_path, pattern):
    n = 3000
    tbl = _typed_table(n, _null_patterns(n)[pattern])
    for layout in LAYOUTS:
        for dictionary in (True, False):
            dev, host, _ = _both(tmp_path, tbl, batch_rows=None, compression="snappy", use_dictionary=dictionary, **layout)
            _assert_same(dev, host)


def test_a_page_of_more_than_one_snappy_block(ctx, tmp_path):
    tbl = pa.table({"k": pa.array(np.arange(10_000, dtype=np.int64) * 3)})
    dev, host, path = _both(tmp_path, tbl, use_dictionary=False, data_page_size=1 << 20)
    pages = _pages(path, 0)[1]
    assert len(pages) == 1 and pages[0]["h"][2][0] > 65536 and pages[0]["size"] < pages[0]["h"][2][0]
    _assert_same(dev, host)


def test_literal_only_and_overlapping_copy_columns(ctx, tmp_path):
    n = 30_000
    rng = np.random.default_rng(3)
    k = np.arange(n)
    tbl = pa.table({"r": pa.array(rng.random(n)), "c": pa.array(np.full(n, 7, dtype=np.int64)), "p2": pa.array((k % 2).astype(np.int8)),
                    "p3": pa.array((k % 3).astype(np.int32)), "p5": pa.array(k % 5, pa.int64(), mask=k % 64 == 63), "p63": pa.array(["v%d" % (v % 63) for v in k])})
    for dictionary in (True, False):
        dev, host, path = _both(tmp_path, tbl, batch_rows=7000, use_dictionary=dictionary)
        _assert_same(dev, host)
    r = pq.ParquetFile(path).metadata.row_group(0).column(0)
    assert r.total_compressed_size >= r.total_uncompressed_size          # random doubles: literals only
    c = pq.ParquetFile(path).metadata.row_group(0).column(1)
    assert c.total_compressed_size * 15 < c.total_uncompressed_size      # a constant: chains of overlapping copies


def test_a_long_string(ctx, tmp_path):
    big = "".join(chr(97 + k % 26) for k in range(200_000))
    for dictionary in (True, False):
        dev, host, path = _both(tmp_path, pa.table({"s": ["a", big, None, "b", big[:70000]]}), use_dictionary=dictionary)
        assert _codecs(path) == ["SNAPPY"]
        _assert_same(dev, host)


def test_a_codec_per_column_with_and_without_projection(ctx, tmp_path):
    n = 5000
    tbl = _typed_table(n, _null_patterns(n)["seventh"])
    for layout in LAYOUTS:
        dev, host, path = _both(tmp_path, tbl, compression=MIXED_CODECS, **layout)
        assert _codecs(path) == ["UNCOMPRESSED", "SNAPPY", "SNAPPY", "UNCOMPRESSED", "SNAPPY", "UNCOMPRESSED", "SNAPPY"]
        _assert_same(dev, host)
        for columns in (["s", "i32", "f64"], ["d", "b"], ["m"]):
            dev, host, _ = _both(tmp_path, tbl, columns=columns, compression=MIXED_CODECS, **layout)
            _assert_same(dev, host)
            assert dev.schema().names == columns
    dev, host, _ = _both(tmp_path, tbl, columns=["i64", "s"], compression=dict(MIXED_CODECS, f64="zstd"))     # an unprojected codec is not looked at
    _assert_same(dev, host)


def test_q1_aggregates_over_a_device_decoded_snappy_lineitem(ctx, tmp_path):
    tbl = pa.Table.from_batches(synth.lineitem(6000, 2048))
    dev, host, path = _both(tmp_path, tbl, batch_rows=2048, name="lineitem.parquet", data_page_size=4096)
    assert set(_codecs(path)) == {"SNAPPY"}
    assert dev.decoded_on_device and dev.device_table().num_rows == 6000
    rows = lambda t: sorted(tuple(r) for b in queries.q1_full(t).execute() for r in zip(*[c.to_pylist() for c in b.columns]))     # noqa: E731
    got = rows(dev)
    assert dev._data is None                     # the query ran on the decoded table; nothing was downloaded
    assert got == rows(host) and len(got) >= 2


def test_the_level_is_a_switch_of_the_context(ctx, tmp_path):
    tbl = _rows_table(3000)
    path = str(tmp_path / "s.parquet")
    pq.write_table(tbl, path)
    data, schema = open(path, "rb").read(), pq.read_schema(path).remove_metadata()
    host = datasource.read_parquet(path, None, 700, device=False)
    ctx.set_parquet_format(1)
    first = datasource.read_parquet(path, None, 700, device=True)
    assert first.decoded_on_device is False and pa.Table.from_batches(first.data).equals(pa.Table.from_batches(host.data))
    with pytest.raises(UnsupportedError, match="compressed"):
        DeviceTable.from_parquet_bytes(ctx, schema, data)
    for bad in (0, 3):
        with pytest.raises(Exception):
            ctx.set_parquet_format(bad)
    with pytest.raises(UnsupportedError, match="compressed"):      # (a refused level leaves the level as it was)
        DeviceTable.from_parquet_bytes(ctx, schema, data)
    ctx.set_parquet_format(2)
    for bad in (0, 3):
        with pytest.raises(Exception):
            ctx.set_parquet_format(bad)
    _assert_same(datasource.read_parquet(path, None, 700, device=True), host)
    assert ctx.last_stats()["main_kernel_name"] == "k_pq_values" and ctx.last_stats()["rows_out"] == 3000


FALLBACKS = {"zstd": ({"compression": "zstd"}, "compressed"), "gzip": ({"compression": "gzip"}, "compressed"),
             "one zstd column": ({"compression": {"i": "snappy", "b": "snappy", "s": "zstd", "r": "NONE"}}, "compressed"),
             "v2 snappy": ({"compression": "snappy", "data_page_version": "2.0"}, "data page V2"), "v2": ({"compression": "NONE", "data_page_version": "2.0"}, "data page V2")}


@pytest.mark.parametrize("what", list(FALLBACKS))
def test_fallback_to_the_host_path_at_level_2(ctx, tmp_path, what):
    kw, reason = FALLBACKS[what]
    tbl = _rows_table(1000)
    path = str(tmp_path / "f.parquet")
    pq.write_table(tbl, path, **kw)
    host = datasource.read_parquet(path, None, 300, device=False)
    dev = datasource.read_parquet(path, None, 300, device=True)
    assert dev.decoded_on_device is False and host.decoded_on_device is False
    assert dev.schema() == host.schema() and [b.num_rows for b in dev.data] == [b.num_rows for b in host.data]
    assert pa.Table.from_batches(dev.data).equals(pa.Table.from_batches(host.data))
    with pytest.raises(UnsupportedError, match=reason):
        DeviceTable.from_parquet_bytes(ctx, pq.read_schema(path).remove_metadata(), open(path, "rb").read())


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("snappy_model")
    exe = str(d / "parquet_snappy_tests")
    subprocess.check_call(["g++"] + FLAGS + ["-O1", "-o", exe, SOURCE])
    return {"plain": exe, "dir": d}


def test_raw_streams_good_and_hostile_side_by_side(ctx, tmp_path, cpu_model):
    good, hostile = good_streams(), hostile_streams()
    names = [("good", k) for k in good] + [("hostile", k) for k in hostile]
    order = np.random.default_rng(1).permutation(len(names))
    names = [names[k] for k in order]                                     # refused streams between decoded ones
    streams = [good[k] if kind == "good" else hostile[k][:2] for kind, k in names]
    want = cpu_model_results(cpu_model, streams)
    outs, statuses = ctx.snappy_decode([s for s, _ in streams], [n for _, n in streams])
    codec = pa.Codec("snappy")
    for (kind, name), (s, n), w, out, status in zip(names, streams, want, outs, statuses):
        if kind == "good":
            assert status == 0 and out == w and isinstance(w, bytes), (name, status)
            assert out == codec.decompress(s, decompressed_size=n, asbytes=True), name
        else:
            assert status == w == hostile[name][2] and out is None, (name, status, w)
    # afterwards a good file still decodes on the same context
    dev, host, _ = _both(tmp_path, _rows_table(2000))
    _assert_same(dev, host)


def test_a_snappy_page_damaged_in_place_is_refused_and_the_context_stays_good(ctx, tmp_path):
    tbl = snappy_hostile_table()
    path = str(tmp_path / "snappy_hostile.parquet")
    pq.write_table(tbl, path, compression="snappy", use_dictionary=False, data_page_size=4096)
    good = open(path, "rb").read()
    data, where = damaged_snappy_file(path)
    rg, col, page = where.split()
    with pytest.raises(UnsupportedError, match="Snappy copy offset.*row group %s, column %s, page %s" % (rg, col, page)):
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, data)
    dev = DeviceTable.from_parquet_bytes(ctx, tbl.schema, good)
    assert pa.Table.from_batches(dev.to_batches()).equals(tbl)
