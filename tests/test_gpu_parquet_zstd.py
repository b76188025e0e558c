"""Codec set 2 of the device Parquet decoder (qhip_ctx_set_parquet_codecs(ctx, 2); k_pq_unzstd): ZSTD files against
the host path on the same bytes, compared exactly as tests/test_gpu_parquet.py compares — and every positive case must have been
decoded on the device, so that a silent fallback cannot pass. Raw frames go through qhip_zstd_decode, good and hostile ones side
by side in one call, against the CPU model of tests/test_parquet_zstd_cpu.py (each has passed the sanitizers there) and against
pyarrow's decoder."""
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from qurious_amd import datasource
from qurious_amd._ffi import DeviceTable, UnsupportedError
from tests.test_gpu_parquet import _assert_same, _rows_table
from tests.test_parquet_cpu import FLAGS, LAYOUTS, _null_patterns, _pages, _typed_table
from tests.test_parquet_zstd_cpu import SOURCE, cpu_model_results, damaged_zstd_file, good_frames, hostile_frames, zstd_hostile_table

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def codecs2(ctx):
    """codec set 2 for the test, the defaults behind it: the context is the process's"""
    ctx.set_parquet_codecs(2)
    yield ctx
    ctx.set_parquet_codecs(1)
    ctx.set_parquet_format(1)
    ctx.set_parquet_encodings(1)


def _both(tmp_path, tbl, batch_rows=1000, columns=None, name="t.parquet", **kw):
    path = str(tmp_path / name)
    pq.write_table(tbl, path, **dict({"compression": "zstd"}, **kw))
    host = datasource.read_parquet(path, columns, batch_rows, device=False)
    dev = datasource.read_parquet(path, columns, batch_rows, device=True)
    return dev, host, path


def _codecs(path):
    meta = pq.ParquetFile(path).metadata.row_group(0)
    return [meta.column(k).compression for k in range(meta.num_columns)]


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
@pytest.mark.parametrize("n", [1, 64, 65, 20_001])
def test_zstd_files_at_the_edges_of_words_pages_and_row_groups(ctx, tmp_path, n, layout):
    dev, host, path = _both(tmp_path, _rows_table(n), **LAYOUTS[layout])
    assert set(_codecs(path)) == {"ZSTD"}
    _assert_same(dev, host)
    assert dev.device_table().num_rows == n
    assert ctx.last_stats()["main_kernel_name"] == "k_pq_values"


@pytest.mark.parametrize("pattern", ["none", "all", "random", "runs"])
def test_null_patterns_on_every_kind_of_column(ctx, tmp_path, pattern):
    n = 3000
    tbl = _typed_table(n, _null_patterns(n)[pattern])
    for layout, level in zip(LAYOUTS, (1, 9, 19)):
        for dictionary in (True, False):
            dev, host, _ = _both(tmp_path, tbl, batch_rows=None, compression_level=level, use_dictionary=dictionary, **layout)
            _assert_same(dev, host)


def test_pages_of_several_blocks_long_strings_and_what_does_not_compress(ctx, tmp_path):
    n = 40_000
    rng = np.random.default_rng(3)
    k = np.arange(n)
    tbl = pa.table({"k": pa.array(k.astype(np.int64) * 3), "r": pa.array(rng.random(n)), "c": pa.array(np.full(n, 7, dtype=np.int64)),
                    "p": pa.array(rng.integers(100, 100_000, n), pa.int64(), mask=k % 64 == 63), "w": pa.array(["v%d" % (v % 63) for v in k])})
    for dictionary in (True, False):
        dev, host, path = _both(tmp_path, tbl, batch_rows=7000, use_dictionary=dictionary, data_page_size=1 << 20)
        _assert_same(dev, host)
    pages = _pages(path, 0)[1]
    assert pages[0]["h"][2][0] > 131072 and pages[0]["size"] < pages[0]["h"][2][0]     # (a writer's page holds 20 000 rows at the most: two blocks)
    big = "".join(chr(97 + k % 26) for k in range(200_000))
    for dictionary in (True, False):
        dev, host, path = _both(tmp_path, pa.table({"s": ["a", big, None, "b", big[:70000]]}), use_dictionary=dictionary)
        _assert_same(dev, host)
    assert _pages(path, 0)[1][0]["h"][2][0] > 2 * 131072                               # one page of three blocks


def test_snappy_stays_with_the_level_and_v2_pages_with_the_encoding_set(ctx, tmp_path):
    n = 5000
    tbl = _typed_table(n, _null_patterns(n)["seventh"])
    mixed = {"i32": "NONE", "i64": "zstd", "f64": "snappy", "d": "zstd", "m": "snappy", "b": "zstd", "s": "zstd"}
    path = str(tmp_path / "m.parquet")
    pq.write_table(tbl, path, compression=mixed)
    assert datasource.read_parquet(path, None, 1000, device=True).decoded_on_device is False          # level 1: the Snappy columns need the host
    dev = datasource.read_parquet(path, ["i64", "s", "i32"], 1000, device=True)                      # ... unless they are not projected
    _assert_same(dev, datasource.read_parquet(path, ["i64", "s", "i32"], 1000, device=False))
    ctx.set_parquet_format(2)
    for layout in LAYOUTS:
        dev, host, path = _both(tmp_path, tbl, compression=mixed, **layout)
        assert _codecs(path) == ["UNCOMPRESSED", "ZSTD", "SNAPPY", "ZSTD", "SNAPPY", "ZSTD", "ZSTD"]
        _assert_same(dev, host)
    ctx.set_parquet_format(1)
    # data pages V2: the levels stay uncompressed in front of the frame
    pq.write_table(tbl, path, compression="zstd", data_page_version="2.0")
    assert datasource.read_parquet(path, None, 1000, device=True).decoded_on_device is False
    with pytest.raises(UnsupportedError, match="data page V2"):
        DeviceTable.from_parquet_bytes(ctx, pq.read_schema(path).remove_metadata(), open(path, "rb").read())
    ctx.set_parquet_encodings(2)
    for dictionary in (True, False):
        for layout in LAYOUTS:
            dev, host, _ = _both(tmp_path, tbl, data_page_version="2.0", use_dictionary=dictionary, **layout)
            _assert_same(dev, host)


def test_the_codec_set_is_a_switch_of_the_context(ctx, tmp_path):
    tbl = _rows_table(3000)
    path = str(tmp_path / "s.parquet")
    pq.write_table(tbl, path, compression="zstd")
    data, schema = open(path, "rb").read(), pq.read_schema(path).remove_metadata()
    host = datasource.read_parquet(path, None, 700, device=False)
    ctx.set_parquet_codecs(1)
    for level in (1, 2):                                   # set 1 is what it was, whatever the level
        ctx.set_parquet_format(level)
        first = datasource.read_parquet(path, None, 700, device=True)
        assert first.decoded_on_device is False and pa.Table.from_batches(first.data).equals(pa.Table.from_batches(host.data))
        with pytest.raises(UnsupportedError, match="compressed"):
            DeviceTable.from_parquet_bytes(ctx, schema, data)
    ctx.set_parquet_format(1)
    for bad in (0, 3, -1):
        with pytest.raises(Exception):
            ctx.set_parquet_codecs(bad)
    with pytest.raises(UnsupportedError, match="compressed"):      # (a refused set leaves the set as it was)
        DeviceTable.from_parquet_bytes(ctx, schema, data)
    ctx.set_parquet_codecs(2)
    for bad in (0, 3):
        with pytest.raises(Exception):
            ctx.set_parquet_codecs(bad)
    ctx.set_timing(True)
    try:
        _assert_same(datasource.read_parquet(path, None, 700, device=True), host)
        assert ctx.parquet_unpack_ms() > 0
        pq.write_table(tbl, path, compression="NONE")
        _assert_same(datasource.read_parquet(path, None, 700, device=True), host)
        assert ctx.parquet_unpack_ms() == 0                # no ZSTD page, no launch
    finally:
        ctx.set_timing(False)
    for codec in ("gzip", "lz4", "brotli"):
        if pa.Codec.is_available(codec):
            pq.write_table(tbl, path, compression=codec)
            with pytest.raises(UnsupportedError, match="compressed"):
                DeviceTable.from_parquet_bytes(ctx, schema, open(path, "rb").read())


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("zstd_model")
    exe = str(d / "parquet_zstd_tests")
    subprocess.check_call(["g++"] + FLAGS + ["-O1", "-o", exe, SOURCE])
    return {"plain": exe, "dir": d}


def test_raw_frames_good_and_hostile_side_by_side(ctx, tmp_path, cpu_model):
    good, hostile = good_frames(), hostile_frames()
    names = [("good", k) for k in good] + [("hostile", k) for k in hostile]
    order = np.random.default_rng(1).permutation(len(names))
    names = [names[k] for k in order]                                     # refused frames between decoded ones
    frames = [(good[k][0], len(good[k][1])) if kind == "good" else hostile[k][:2] for kind, k in names]
    want = cpu_model_results(cpu_model, frames)
    outs, statuses = ctx.zstd_decode([s for s, _ in frames], [n for _, n in frames])
    for (kind, name), w, out, status in zip(names, want, outs, statuses):
        if kind == "good":
            assert status == 0 and out == w and out == good[name][1], (name, status)
        else:
            assert status == w == hostile[name][2] and out is None, (name, status, w)
    # afterwards a good file still decodes on the same context
    dev, host, _ = _both(tmp_path, _rows_table(2000))
    _assert_same(dev, host)


def test_a_zstd_page_damaged_in_place_is_refused_and_the_context_stays_good(ctx, tmp_path):
    tbl = zstd_hostile_table()
    path = str(tmp_path / "zstd_hostile.parquet")
    pq.write_table(tbl, path, compression="zstd", use_dictionary=False, data_page_size=4096)
    good = open(path, "rb").read()
    data, where = damaged_zstd_file(path)
    rg, col, page = where.split()
    with pytest.raises(UnsupportedError, match="Zstd block header.*row group %s, column %s, page %s" % (rg, col, page)):
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, data)
    # damage the host's walk cannot see: the last byte of the first block of page 2, where its sequence stream's end mark lies
    pages = _pages(path, 0)[1]
    at = pages[2]["payload"]
    d = good[at + 4]
    at += 5 + (0 if d & 0x20 else 1) + {0: d >> 5 & 1, 1: 2, 2: 4, 3: 8}[d >> 6]
    head = int.from_bytes(good[at:at + 3], "little")
    assert head >> 1 & 3 == 2                              # (a compressed block)
    end = at + 3 + (head >> 3)
    with pytest.raises(UnsupportedError, match="Zstd bit stream.*row group 0, column 0, page 2"):
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, good[:end - 1] + b"\x00" + good[end:])
    dev = DeviceTable.from_parquet_bytes(ctx, tbl.schema, good)
    assert pa.Table.from_batches(dev.to_batches()).equals(tbl)
