"""The gzip switch of the device Parquet decoder (qhip_ctx_set_parquet_gzip(ctx, 1); k_pq_ungzip): GZIP files against
the host path on the same bytes, compared exactly as tests/test_gpu_parquet.py compares — and every positive case must have been
decoded on the device, so that a silent fallback cannot pass. Raw members go through qhip_gzip_decode, good and hostile ones side
by side in one call, against the CPU model of tests/test_parquet_gzip_cpu.py (each has passed the sanitizers there) and against
zlib."""
import subprocess
import zlib

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from qurious_amd import datasource
from qurious_amd._ffi import DeviceTable, UnsupportedError
from tests.test_gpu_parquet import _assert_same, _rows_table
from tests.test_parquet_cpu import FLAGS, LAYOUTS, _null_patterns, _pages, _typed_table
from tests.test_parquet_gzip_cpu import SOURCE, cpu_model_results, damaged_gzip_file, good_members, gzip_hostile_table, hostile_members

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def gzip_on(ctx):
    """the gzip switch on for the test, the defaults of all four switches behind it: the context is the process's"""
    ctx.set_parquet_gzip(1)
    yield ctx
    ctx.set_parquet_gzip(0)
    ctx.set_parquet_codecs(1)
    ctx.set_parquet_format(1)
    ctx.set_parquet_encodings(1)


def _both(ctx, tmp_path, tbl, batch_rows=1000, columns=None, name="t.parquet", **kw):
    path = str(tmp_path / name)
    pq.write_table(tbl, path, **dict({"compression": "gzip"}, **kw))
    host = datasource.read_parquet(path, columns, batch_rows, device=False)
    dev = datasource.read_parquet(path, columns, batch_rows, device=True)
    assert dev.decoded_on_device is True and ctx.last_stats()["main_kernel_name"] == "k_pq_values"
    return dev, host, path


def _codecs(path):
    meta = pq.ParquetFile(path).metadata.row_group(0)
    return [meta.column(k).compression for k in range(meta.num_columns)]


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
@pytest.mark.parametrize("n", [1, 64, 65, 20_001])
def test_gzip_files_at_the_edges_of_words_pages_and_row_groups(ctx, tmp_path, n, layout):
    dev, host, path = _both(ctx, tmp_path, _rows_table(n), **LAYOUTS[layout])
    assert set(_codecs(path)) == {"GZIP"}
    _assert_same(dev, host)
    assert dev.device_table().num_rows == n


@pytest.mark.parametrize("pattern", ["none", "all", "random", "runs"])
def test_null_patterns_on_every_kind_of_column(ctx, tmp_path, pattern):
    n = 3000
    tbl = _typed_table(n, _null_patterns(n)[pattern])
    for layout, level in zip(LAYOUTS, (1, 6, 9)):
        for dictionary in (True, False):
            dev, host, _ = _both(ctx, tmp_path, tbl, batch_rows=None, compression_level=level, use_dictionary=dictionary, **layout)
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
    # the random column does not compress: its pages come as stored blocks
    data, pages = _pages(path, 1)
    body = data[pages[0]["payload"] + 10:pages[0]["payload"] + pages[0]["size"] - 8]
    assert body[0] & 6 == 0 and len(body) > pages[0]["h"][2][0]
    big = "".join(chr(97 + k % 26) for k in range(200_000))
    for dictionary in (True, False):
        dev, host, path = _both(ctx, tmp_path, pa.table({"s": ["a", big, None, "b", big[:70000]]}), use_dictionary=dictionary)
        _assert_same(dev, host)
    assert _pages(path, 0)[1][0]["h"][2][0] > 2 * 131072


def test_the_other_codecs_stay_with_their_switches_and_v2_pages_with_the_encoding_set(ctx, tmp_path):
    n = 5000
    tbl = _typed_table(n, _null_patterns(n)["seventh"])
    mixed = {"i32": "NONE", "i64": "gzip", "f64": "snappy", "d": "gzip", "m": "zstd", "b": "gzip", "s": "gzip"}
    path = str(tmp_path / "m.parquet")
    pq.write_table(tbl, path, compression=mixed)
    assert datasource.read_parquet(path, None, 1000, device=True).decoded_on_device is False          # the Snappy and ZSTD columns need the host
    ctx.set_parquet_format(2)
    assert datasource.read_parquet(path, None, 1000, device=True).decoded_on_device is False          # ... the ZSTD column still does
    ctx.set_parquet_format(1)
    ctx.set_parquet_codecs(2)
    assert datasource.read_parquet(path, None, 1000, device=True).decoded_on_device is False          # ... the Snappy column still does
    ctx.set_parquet_codecs(1)
    dev = datasource.read_parquet(path, ["i64", "s", "i32"], 1000, device=True)                      # ... unless they are not projected
    _assert_same(dev, datasource.read_parquet(path, ["i64", "s", "i32"], 1000, device=False))
    ctx.set_parquet_format(2)
    ctx.set_parquet_codecs(2)
    for layout in LAYOUTS:
        dev, host, path = _both(ctx, tmp_path, tbl, compression=mixed, **layout)
        assert _codecs(path) == ["UNCOMPRESSED", "GZIP", "SNAPPY", "GZIP", "ZSTD", "GZIP", "GZIP"]
        _assert_same(dev, host)
    ctx.set_parquet_format(1)
    ctx.set_parquet_codecs(1)
    # data pages V2: the levels stay uncompressed in front of the member
    pq.write_table(tbl, path, compression="gzip", data_page_version="2.0")
    assert datasource.read_parquet(path, None, 1000, device=True).decoded_on_device is False
    with pytest.raises(UnsupportedError, match="data page V2"):
        DeviceTable.from_parquet_bytes(ctx, pq.read_schema(path).remove_metadata(), open(path, "rb").read())
    ctx.set_parquet_encodings(2)
    for dictionary in (True, False):
        for layout in LAYOUTS:
            dev, host, _ = _both(ctx, tmp_path, tbl, data_page_version="2.0", use_dictionary=dictionary, **layout)
            _assert_same(dev, host)


def test_gzip_is_a_switch_of_the_context(ctx, tmp_path):
    tbl = _rows_table(3000)
    path = str(tmp_path / "s.parquet")
    pq.write_table(tbl, path, compression="gzip")
    data, schema = open(path, "rb").read(), pq.read_schema(path).remove_metadata()
    host = datasource.read_parquet(path, None, 700, device=False)
    ctx.set_parquet_gzip(0)
    for level, encodings, codecs in ((1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 2)):      # off is what it was, whatever the other three say
        ctx.set_parquet_format(level)
        ctx.set_parquet_encodings(encodings)
        ctx.set_parquet_codecs(codecs)
        first = datasource.read_parquet(path, None, 700, device=True)
        assert first.decoded_on_device is False and pa.Table.from_batches(first.data).equals(pa.Table.from_batches(host.data))
        with pytest.raises(UnsupportedError, match="compressed"):
            DeviceTable.from_parquet_bytes(ctx, schema, data)
    ctx.set_parquet_format(1)
    ctx.set_parquet_encodings(1)
    ctx.set_parquet_codecs(1)
    for bad in (2, -1):
        with pytest.raises(Exception):
            ctx.set_parquet_gzip(bad)
    with pytest.raises(UnsupportedError, match="compressed"):      # (a refused value leaves the switch as it was)
        DeviceTable.from_parquet_bytes(ctx, schema, data)
    ctx.set_parquet_gzip(1)
    for bad in (2, -1):
        with pytest.raises(Exception):
            ctx.set_parquet_gzip(bad)
    ctx.set_timing(True)
    try:
        dev = datasource.read_parquet(path, None, 700, device=True)
        assert ctx.last_stats()["main_kernel_name"] == "k_pq_values"
        _assert_same(dev, host)
        assert ctx.parquet_unpack_ms() > 0
        pq.write_table(tbl, path, compression="NONE")
        dev = datasource.read_parquet(path, None, 700, device=True)
        assert ctx.last_stats()["main_kernel_name"] == "k_pq_values"
        _assert_same(dev, host)
        assert ctx.parquet_unpack_ms() == 0                # no GZIP page, no launch
    finally:
        ctx.set_timing(False)
    for codec in ("lz4", "brotli"):                        # these stay on the host
        if pa.Codec.is_available(codec):
            pq.write_table(tbl, path, compression=codec)
            with pytest.raises(UnsupportedError, match="compressed"):
                DeviceTable.from_parquet_bytes(ctx, schema, open(path, "rb").read())


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_model")
    exe = str(d / "parquet_gzip_tests")
    subprocess.check_call(["g++"] + FLAGS + ["-O1", "-o", exe, SOURCE])
    return {"plain": exe, "dir": d}


def test_raw_members_good_and_hostile_side_by_side(ctx, tmp_path, cpu_model):
    good, hostile = good_members(), hostile_members()
    names = [("good", k) for k in good] + [("hostile", k) for k in hostile]
    order = np.random.default_rng(1).permutation(len(names))
    names = [names[k] for k in order]                                     # refused members between decoded ones
    members = [(good[k][0], len(good[k][1])) if kind == "good" else hostile[k][:2] for kind, k in names]
    want = cpu_model_results(cpu_model, members)
    outs, statuses = ctx.gzip_decode([s for s, _ in members], [n for _, n in members])
    for (kind, name), w, out, status in zip(names, want, outs, statuses):
        if kind == "good":
            assert status == 0 and out == w and out == good[name][1] and out == zlib.decompress(good[name][0], 31), (name, status)
        else:
            assert status == w == hostile[name][2] and out is None, (name, status, w)
    # afterwards a good file still decodes on the same context
    dev, host, _ = _both(ctx, tmp_path, _rows_table(2000))
    _assert_same(dev, host)


def test_a_gzip_page_damaged_in_place_is_refused_and_the_context_stays_good(ctx, tmp_path):
    tbl = gzip_hostile_table()
    path = str(tmp_path / "gzip_hostile.parquet")
    pq.write_table(tbl, path, compression="gzip", use_dictionary=False, data_page_size=4096)
    good = open(path, "rb").read()
    data, where = damaged_gzip_file(path)                  # damage the host's walk sees
    rg, col, page = where.split()
    with pytest.raises(UnsupportedError, match="Gzip page whose ISIZE.*row group %s, column %s, page %s" % (rg, col, page)):
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, data)
    data, where = damaged_gzip_file(path, "btype")         # damage only the kernel sees
    rg, col, page = where.split()
    with pytest.raises(UnsupportedError, match="Gzip block header.*row group %s, column %s, page %s" % (rg, col, page)):
        DeviceTable.from_parquet_bytes(ctx, tbl.schema, data)
    dev = DeviceTable.from_parquet_bytes(ctx, tbl.schema, good)
    assert pa.Table.from_batches(dev.to_batches()).equals(tbl)
