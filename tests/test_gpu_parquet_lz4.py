"""The lz4 switch of the device Parquet decoder (qhip_ctx_set_parquet_lz4(ctx, 1); k_pq_unlz4): LZ4 files — LZ4_RAW as
pyarrow writes them, the legacy id as a bare block and in Hadoop's framing — against the host path on the same bytes, compared
exactly as tests/test_gpu_parquet.py compares — and every positive case must have been decoded on the device, so that a silent
fallback cannot pass. Raw blocks go through qhip_lz4_decode, good, hand-made and hostile ones side by side in one call, against
the CPU model of tests/test_parquet_lz4_cpu.py (each has passed the sanitizers there) and against pa.Codec("lz4_raw")."""
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from qurious_amd import datasource
from qurious_amd._ffi import DeviceTable, UnsupportedError
from tests.test_gpu_parquet import _assert_same, _rows_table
from tests.test_parquet_cpu import FLAGS, LAYOUTS, _null_patterns, _pages, _typed_table
from tests.test_parquet_lz4_cpu import (LZ4, SOURCE, codec_varints, cpu_model_results, damaged_lz4_file, good_blocks, hadoop_file, hadoop_table, handmade_blocks,
                                        hostile_blocks, legacy_id, lz4_hostile_table)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def lz4_on(ctx):
    """the lz4 switch on for the test, the defaults of all five switches behind it: the context is the process's"""
    ctx.set_parquet_lz4(1)
    yield ctx
    ctx.set_parquet_lz4(0)
    ctx.set_parquet_gzip(0)
    ctx.set_parquet_codecs(1)
    ctx.set_parquet_format(1)
    ctx.set_parquet_encodings(1)


def _both(ctx, tmp_path, tbl, batch_rows=1000, columns=None, name="t.parquet", **kw):
    path = str(tmp_path / name)
    pq.write_table(tbl, path, **dict({"compression": "lz4"}, **kw))
    return _read_both(ctx, path, batch_rows, columns) + (path,)


def _read_both(ctx, path, batch_rows=1000, columns=None):
    host = datasource.read_parquet(path, columns, batch_rows, device=False)
    dev = datasource.read_parquet(path, columns, batch_rows, device=True)
    assert dev.decoded_on_device is True and ctx.last_stats()["main_kernel_name"] == "k_pq_values"
    return dev, host


def _codec_ids(path):
    return {v for _, v in codec_varints(open(path, "rb").read())}


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
@pytest.mark.parametrize("n", [1, 64, 65, 20_001])
def test_lz4_files_at_the_edges_of_words_pages_and_row_groups(ctx, tmp_path, n, layout):
    dev, host, path = _both(ctx, tmp_path, _rows_table(n), **LAYOUTS[layout])
    assert _codec_ids(path) == {7}
    _assert_same(dev, host)
    assert dev.device_table().num_rows == n


@pytest.mark.parametrize("pattern", ["none", "all", "random", "runs"])
def test_null_patterns_on_every_kind_of_column(ctx, tmp_path, pattern):
    n = 3000
    tbl = _typed_table(n, _null_patterns(n)[pattern])
    for layout in LAYOUTS:
        for dictionary in (True, False):
            dev, host, _ = _both(ctx, tmp_path, tbl, batch_rows=None, use_dictionary=dictionary, **layout)
            _assert_same(dev, host)


def test_large_pages_long_strings_and_what_does_not_compress(ctx, tmp_path):
    n = 40_000
    rng = np.random.default_rng(3)
    k = np.arange(n)
    tbl = pa.table({"k": pa.array(k.astype(np.int64) * 3), "r": pa.array(np.frombuffer(rng.bytes(8 * n), dtype=np.int64)), "c": pa.array(np.full(n, 7, dtype=np.int64)),
                    "p": pa.array(rng.integers(100, 100_000, n), pa.int64(), mask=k % 64 == 63), "w": pa.array(["v%d" % (v % 63) for v in k])})
    for dictionary in (True, False):
        dev, host, path = _both(ctx, tmp_path, tbl, batch_rows=7000, use_dictionary=dictionary, data_page_size=1 << 20)
        _assert_same(dev, host)
    data, pages = _pages(path, 0)
    assert pages[0]["h"][2][0] > 131072 and pages[0]["size"] < pages[0]["h"][2][0]     # one page of more than 128 KB
    # the random column does not compress: one literal run spans its page
    data, pages = _pages(path, 1)
    at, size, plain = pages[0]["payload"], pages[0]["size"], pages[0]["h"][2][0]
    assert data[at] == 0xF0 and size == 1 + (plain - 15) // 255 + 1 + plain
    # the constant column: long matches that overlap themselves at a small offset
    data, pages = _pages(path, 2)
    assert pages[0]["size"] < pages[0]["h"][2][0] // 200   # (a match's extension adds 255 bytes per byte)
    big = "".join(chr(97 + k % 26) for k in range(200_000))
    for dictionary in (True, False):
        dev, host, path = _both(ctx, tmp_path, pa.table({"s": ["a", big, None, "b", big[:70000]]}), use_dictionary=dictionary)
        _assert_same(dev, host)
    assert _pages(path, 0)[1][0]["h"][2][0] > 2 * 131072


def test_the_other_codecs_stay_with_their_switches_and_v2_pages_with_the_encoding_set(ctx, tmp_path):
    n = 5000
    tbl = _typed_table(n, _null_patterns(n)["seventh"])
    mixed = {"i32": "NONE", "i64": "lz4", "f64": "snappy", "d": "lz4", "m": "zstd", "b": "gzip", "s": "lz4"}
    path = str(tmp_path / "m.parquet")
    pq.write_table(tbl, path, compression=mixed)

    def on_device(level, codecs, gzip, lz4):
        ctx.set_parquet_format(level)
        ctx.set_parquet_codecs(codecs)
        ctx.set_parquet_gzip(gzip)
        ctx.set_parquet_lz4(lz4)
        return datasource.read_parquet(path, None, 1000, device=True).decoded_on_device
    assert on_device(1, 1, 0, 1) is False                  # the Snappy, ZSTD and GZIP columns need the host
    assert on_device(1, 2, 1, 1) is False                  # ... one switch missing: the Snappy column still does
    assert on_device(2, 1, 1, 1) is False                  # ... the ZSTD column
    assert on_device(2, 2, 0, 1) is False                  # ... the GZIP column
    assert on_device(2, 2, 1, 0) is False                  # ... the LZ4 columns
    assert on_device(2, 2, 1, 1) is True
    ctx.set_parquet_format(1)
    ctx.set_parquet_codecs(1)
    ctx.set_parquet_gzip(0)
    dev = datasource.read_parquet(path, ["i64", "s", "i32"], 1000, device=True)                      # ... unless they are not projected
    assert dev.decoded_on_device is True
    _assert_same(dev, datasource.read_parquet(path, ["i64", "s", "i32"], 1000, device=False))
    ctx.set_parquet_format(2)
    ctx.set_parquet_codecs(2)
    ctx.set_parquet_gzip(1)
    for layout in LAYOUTS:
        dev, host, path = _both(ctx, tmp_path, tbl, compression=mixed, **layout)
        meta = pq.ParquetFile(path).metadata.row_group(0)
        assert [meta.column(k).compression for k in (0, 2, 4, 5)] == ["UNCOMPRESSED", "SNAPPY", "ZSTD", "GZIP"]
        assert _codec_ids(path) == {0, 1, 2, 6, 7}
        _assert_same(dev, host)
    ctx.set_parquet_format(1)
    ctx.set_parquet_codecs(1)
    ctx.set_parquet_gzip(0)
    # data pages V2: the levels stay uncompressed in front of the block
    pq.write_table(tbl, path, compression="lz4", data_page_version="2.0")
    assert datasource.read_parquet(path, None, 1000, device=True).decoded_on_device is False
    with pytest.raises(UnsupportedError, match="data page V2"):
        DeviceTable.from_parquet_bytes(ctx, pq.read_schema(path).remove_metadata(), open(path, "rb").read())
    ctx.set_parquet_encodings(2)
    for dictionary in (True, False):
        for layout in LAYOUTS:
            dev, host, _ = _both(ctx, tmp_path, tbl, data_page_version="2.0", use_dictionary=dictionary, **layout)
            _assert_same(dev, host)


def test_the_legacy_id_as_a_bare_block_and_in_hadoop_framing(ctx, tmp_path):
    tbl = _typed_table(3000, _null_patterns(3000)["random"])
    for layout in LAYOUTS:
        path = str(tmp_path / "raw.parquet")
        pq.write_table(tbl, path, compression="lz4", **layout)
        old = str(tmp_path / "legacy.parquet")
        with open(old, "wb") as f:
            f.write(legacy_id(open(path, "rb").read()))
        assert _codec_ids(old) == {5}
        dev, host = _read_both(ctx, old, None)
        _assert_same(dev, host)                            # (the host read of the patched file: Arrow's fallback to the bare block)
        _assert_same(dev, datasource.read_parquet(path, None, None, device=False))
    # Hadoop's frames, one and more per page: the host splits them, the kernel sees bare blocks
    path = str(tmp_path / "hadoop.parquet")
    data, frames = hadoop_file(path)
    with open(path, "wb") as f:
        f.write(data)
    assert _codec_ids(path) == {5}
    dev, host = _read_both(ctx, path, 1000)
    _assert_same(dev, host)
    assert pa.Table.from_batches(host.data).equals(hadoop_table())
    ctx.set_parquet_lz4(0)
    with pytest.raises(UnsupportedError, match="compressed"):
        DeviceTable.from_parquet_bytes(ctx, hadoop_table().schema, data)


def test_lz4_is_a_switch_of_the_context(ctx, tmp_path):
    tbl = _rows_table(3000)
    path = str(tmp_path / "s.parquet")
    pq.write_table(tbl, path, compression="lz4")
    data, schema = open(path, "rb").read(), pq.read_schema(path).remove_metadata()
    host = datasource.read_parquet(path, None, 700, device=False)
    ctx.set_parquet_lz4(0)
    for level in (1, 2):                                   # off is what it was, whatever the other four say
        for encodings in (1, 2):
            for codecs in (1, 2):
                for gzip in (0, 1):
                    ctx.set_parquet_format(level)
                    ctx.set_parquet_encodings(encodings)
                    ctx.set_parquet_codecs(codecs)
                    ctx.set_parquet_gzip(gzip)
                    with pytest.raises(UnsupportedError, match="compressed"):
                        DeviceTable.from_parquet_bytes(ctx, schema, data)
    first = datasource.read_parquet(path, None, 700, device=True)
    assert first.decoded_on_device is False and pa.Table.from_batches(first.data).equals(pa.Table.from_batches(host.data))
    ctx.set_parquet_format(1)
    ctx.set_parquet_encodings(1)
    ctx.set_parquet_codecs(1)
    ctx.set_parquet_gzip(0)
    for bad in (2, -1):
        with pytest.raises(Exception):
            ctx.set_parquet_lz4(bad)
    with pytest.raises(UnsupportedError, match="compressed"):      # (a refused value leaves the switch as it was)
        DeviceTable.from_parquet_bytes(ctx, schema, data)
    ctx.set_parquet_lz4(1)
    for bad in (2, -1):
        with pytest.raises(Exception):
            ctx.set_parquet_lz4(bad)
    ctx.set_timing(True)
    try:
        dev = datasource.read_parquet(path, None, 700, device=True)
        assert dev.decoded_on_device is True and ctx.last_stats()["main_kernel_name"] == "k_pq_values"
        _assert_same(dev, host)
        assert ctx.parquet_unpack_ms() > 0
        pq.write_table(tbl, path, compression="NONE")
        dev = datasource.read_parquet(path, None, 700, device=True)
        assert ctx.last_stats()["main_kernel_name"] == "k_pq_values"
        _assert_same(dev, host)
        assert ctx.parquet_unpack_ms() == 0                # no LZ4 page, no launch
    finally:
        ctx.set_timing(False)
    if pa.Codec.is_available("brotli"):                    # brotli stays on the host
        pq.write_table(tbl, path, compression="brotli")
        with pytest.raises(UnsupportedError, match="compressed"):
            DeviceTable.from_parquet_bytes(ctx, schema, open(path, "rb").read())


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("lz4_model")
    exe = str(d / "parquet_lz4_tests")
    subprocess.check_call(["g++"] + FLAGS + ["-O1", "-o", exe, SOURCE])
    return {"plain": exe, "dir": d}


def test_raw_blocks_good_handmade_and_hostile_side_by_side(ctx, tmp_path, cpu_model):
    good, hostile = dict(good_blocks(), **handmade_blocks()), hostile_blocks()
    good["no input at all"] = (b"", b"")
    names = [("good", k) for k in good] + [("hostile", k) for k in hostile]
    order = np.random.default_rng(1).permutation(len(names))
    names = [names[k] for k in order]                                     # refused blocks between decoded ones
    blocks = [(good[k][0], len(good[k][1])) if kind == "good" else hostile[k][:2] for kind, k in names]
    want = cpu_model_results(cpu_model, blocks)
    outs, statuses = ctx.lz4_decode([s for s, _ in blocks], [n for _, n in blocks])
    for (kind, name), w, out, status in zip(names, want, outs, statuses):
        if kind == "good":
            assert status == 0 and out == w and out == good[name][1], (name, status)
        else:
            assert status == w == hostile[name][2] and out is None, (name, status, w)
    for name, (s, d) in good_blocks().items():
        assert LZ4.decompress(s, decompressed_size=len(d), asbytes=True) == d, name
    # afterwards a good file still decodes on the same context
    dev, host, _ = _both(ctx, tmp_path, _rows_table(2000))
    _assert_same(dev, host)


def test_an_lz4_page_damaged_in_place_is_refused_and_the_context_stays_good(ctx, tmp_path):
    tbl = lz4_hostile_table()
    path = str(tmp_path / "lz4_hostile.parquet")
    pq.write_table(tbl, path, compression="lz4", use_dictionary=False, data_page_size=4096)
    good = open(path, "rb").read()
    data, where = damaged_lz4_file(path)                   # damage only the kernel sees
    rg, col, page = where.split()
    with pytest.raises(UnsupportedError, match="LZ4 match offset.*row group %s, column %s, page %s" % (rg, col, page)):
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, data)
    dev = DeviceTable.from_parquet_bytes(ctx, tbl.schema, good)
    assert pa.Table.from_batches(dev.to_batches()).equals(tbl)
