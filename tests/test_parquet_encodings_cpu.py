"""Encoding set 2 of the device Parquet decoder without a GPU (qhip_ctx_set_parquet_encodings): data pages V2, RLE
Boolean values, BYTE_STREAM_SPLIT, DELTA_BINARY_PACKED and DELTA_LENGTH_BYTE_ARRAY. tests/cpp/parquet_encodings_tests.cpp
contains the page walk as it is and the code the kernels share with the host (csrc/device/qhip_parquet.inc, qhip_delta.inc),
driven by loops that stand for the lanes; it decodes whole files into a text dump, compared with `pyarrow.parquet.read_table`
on the same bytes, and raw delta streams, compared with a byte-serial model of this file's own that is first pinned against
pages pyarrow wrote. Built with g++ as a stand-alone program (nothing of it is loaded into Python), once plainly and once with
the address and undefined-behaviour sanitizers; every stream is decoded from and into heap blocks of exactly its size."""
import decimal
import os
import random
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests.test_parquet_cpu import (BOTH, FLAGS, LAYOUTS, ROOT, SAN, R_ENCODING, R_PAGE_V2, _code, _expect, _finish, _max_varint, _null_patterns, _pages,
                                    _patched, _typed_table, _uleb)

SOURCE = os.path.join(ROOT, "tests", "cpp", "parquet_encodings_tests.cpp")

# the reasons of encoding set 2, behind QH_PQ_R_SNAPPY_OFFSET = 33 (csrc/device/qhip_parquet.inc)
(R_V2_UNCOMPRESSED, R_V2_LEVELS, R_V2_REPETITION, R_V2_ROWS, R_V2_NULLS, R_RLE_LENGTH, R_BSS_SIZE, R_DELTA_VARINT, R_DELTA_GEOMETRY, R_DELTA_LARGE, R_DELTA_COUNT,
 R_DELTA_SHORT, R_DELTA_WIDTH, R_DELTA_LENGTH) = range(34, 48)
R_RANGE, R_SNAPPY_PREAMBLE = 27, 29


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_encodings_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("parquet_encodings_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


def _decode(exes, which, path, schema, proj=None, level=1, encodings=2):
    args = [exes[which], "decode", path, ",".join(_code(f.type) for f in schema), ",".join(map(str, proj)) if proj else "-", str(level), str(encodings)]
    return _finish(subprocess.run(args, capture_output=True))


def _check(exes, tbl, which=BOTH, columns=None, level=1, name="t.parquet", **kw):
    path = str(exes["dir"] / name)
    kw.setdefault("compression", "NONE")
    pq.write_table(tbl, path, **kw)
    schema = pq.read_schema(path)
    want = _expect(pq.read_table(path, columns=columns))
    proj = [schema.get_field_index(c) for c in columns] if columns else None
    for w in which:
        got = _decode(exes, w, path, schema, proj, level)
        assert got == want, (got[:3], want[:3])
    return path


def _reason(exes, path, schema, reasons, which=BOTH, level=1, encodings=2):
    for w in which:
        got = _decode(exes, w, path, schema, None, level, encodings)
        assert len(got) == 1 and got[0].startswith("NEEDS_HOST ") and int(got[0].split()[1]) in reasons, (got[:2], reasons)


def _encodings(path, column):
    md = pq.ParquetFile(path).metadata
    return set(md.row_group(0).column(column).encodings)


# ---------------------------------------------------------------- how the files are written
DELTA = {"i32": "DELTA_BINARY_PACKED", "i64": "DELTA_BINARY_PACKED", "d": "DELTA_BINARY_PACKED", "s": "DELTA_LENGTH_BYTE_ARRAY"}
BSS = {"i32": "BYTE_STREAM_SPLIT", "i64": "BYTE_STREAM_SPLIT", "f64": "BYTE_STREAM_SPLIT", "m": "BYTE_STREAM_SPLIT", "f32": "BYTE_STREAM_SPLIT"}
KINDS = {
    "v2": dict(data_page_version="2.0"),
    "v2 plain": dict(data_page_version="2.0", use_dictionary=False),
    "v2 snappy": dict(data_page_version="2.0", compression="snappy", level=2),
    "v2 snappy plain": dict(data_page_version="2.0", compression="snappy", use_dictionary=False, level=2),
    "v1 delta": dict(data_page_version="1.0", use_dictionary=False, column_encoding=DELTA),
    "v2 delta": dict(data_page_version="2.0", use_dictionary=False, column_encoding=DELTA),
    "v2 snappy delta": dict(data_page_version="2.0", use_dictionary=False, column_encoding=DELTA, compression="snappy", level=2),
    "v1 bss": dict(data_page_version="1.0", use_dictionary=False, column_encoding=BSS),
    "v2 bss": dict(data_page_version="2.0", use_dictionary=False, column_encoding=BSS),
    "v1 rle": dict(data_page_version="1.0", use_dictionary=False, column_encoding={"b": "RLE"}),
}


def typed_table(n, nulls):
    """tests.test_parquet_cpu's table and a Float32 column"""
    t = _typed_table(n, nulls)
    return t.append_column("f32", pa.array((np.arange(n) / 3.0).astype(np.float32), mask=nulls))


@pytest.mark.parametrize("kind", list(KINDS))
def test_null_patterns_and_layouts_for_every_way_of_writing(exes, kind):
    n = 1000
    for name, nulls in _null_patterns(n).items():
        for layout in LAYOUTS:
            path = _check(exes, typed_table(n, nulls), **dict(KINDS[kind], **layout))
    if "delta" in kind:
        assert "DELTA_BINARY_PACKED" in _encodings(path, 0) and "DELTA_LENGTH_BYTE_ARRAY" in _encodings(path, 6)
    if "bss" in kind:
        assert all("BYTE_STREAM_SPLIT" in _encodings(path, c) for c in (0, 1, 2, 4, 7))
    if kind.startswith("v2") or kind == "v1 rle":
        assert "RLE" in _encodings(path, 5) and "PLAIN" not in _encodings(path, 5)      # pyarrow: Boolean values as RLE
    if kind.startswith("v2"):
        assert all(pg["type"] in (2, 3) for pg in _pages(path, 0)[1])


@pytest.mark.parametrize("n", [1, 2, 33, 34, 63, 64, 65, 66, 129, 130, 257, 258, 20_001])
def test_row_counts_at_the_edges_of_miniblocks_blocks_words_and_pages(exes, n):
    which = BOTH if n < 1000 else ("plain",)
    for pattern in ("none", "seventh"):
        tbl = typed_table(n, _null_patterns(n)[pattern])
        for kind in ("v2", "v2 snappy plain", "v1 delta", "v2 delta", "v2 bss", "v1 rle"):
            _check(exes, tbl, which=which, **KINDS[kind])
    if n > 1000:
        _check(exes, typed_table(n, _null_patterns(n)["seventh"]), which=("san",), **KINDS["v2 snappy delta"])
    req = pa.table([pa.array(np.arange(n, dtype=np.int32) * 3), pa.array(np.arange(n, dtype=np.int64) * -5), pa.array(["s%d" % k for k in range(n)])],
                   schema=pa.schema([pa.field("i32", pa.int32(), nullable=False), pa.field("i64", pa.int64(), nullable=False), pa.field("s", pa.string(), nullable=False)]))
    for version in ("1.0", "2.0"):
        _check(exes, req, which=which, data_page_version=version, use_dictionary=False, column_encoding={k: DELTA[k] for k in ("i32", "i64", "s")})


def test_full_range_values_wrap_and_constants_have_width_0(exes):
    rng = np.random.default_rng(7)
    n = 700
    tbl = pa.table({"i32": pa.array(rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)),
                    "i64": pa.array(rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64), mask=np.arange(n) % 9 == 0),
                    "edges": pa.array([-2 ** 63, 2 ** 63 - 1] * (n // 2), pa.int64()), "e32": pa.array([2 ** 31 - 1, -2 ** 31] * (n // 2), pa.int32()),
                    "c32": pa.array(np.full(n, 41, dtype=np.int32)), "c64": pa.array(np.full(n, -2 ** 40, dtype=np.int64)),
                    "step": pa.array(np.arange(n, dtype=np.int64) * 1000)})
    enc = {c: "DELTA_BINARY_PACKED" for c in tbl.column_names}
    for version in ("1.0", "2.0"):
        path = _check(exes, tbl, name="wrap.parquet", data_page_version=version, use_dictionary=False, column_encoding=enc)
        _check(exes, tbl, data_page_version=version, use_dictionary=False, column_encoding={c: "BYTE_STREAM_SPLIT" for c in tbl.column_names})
    data, pages = _pages(path, 4)
    assert pages[0]["size"] < 40          # a constant: every width 0


def test_every_annotation_of_the_integer_types_delta_packed_and_split(exes):
    def ints(t, lo, hi):
        return pa.array([lo, hi, 0, None, 1, -1 if lo < 0 else 2, lo + 1, hi - 1] * 20, t)
    cols = {"i8": ints(pa.int8(), -128, 127), "i16": ints(pa.int16(), -2 ** 15, 2 ** 15 - 1), "u8": ints(pa.uint8(), 0, 255), "u16": ints(pa.uint16(), 0, 65535),
            "u32": ints(pa.uint32(), 0, 2 ** 32 - 1), "u64": ints(pa.uint64(), 0, 2 ** 64 - 1), "ts_ms": ints(pa.timestamp("ms"), -2 ** 63, 2 ** 63 - 1),
            "ts_us": ints(pa.timestamp("us"), -2 ** 63, 2 ** 63 - 1), "ts_ns": ints(pa.timestamp("ns"), -2 ** 63, 2 ** 63 - 1), "d": ints(pa.date32(), -719162, 2932896)}
    for p in (2, 9, 11, 18):
        top = 10 ** p - 1
        vals = [top, -top, 0, None, 1, -1, top // 7, -(top // 3)] * 20
        cols["dec%d" % p] = pa.array([None if v is None else decimal.Decimal(v).scaleb(-(p // 2), context=decimal.Context(prec=100)) for v in vals], pa.decimal128(p, p // 2))
    tbl = pa.table(cols)
    for enc in ("DELTA_BINARY_PACKED", "BYTE_STREAM_SPLIT"):
        for version in ("1.0", "2.0"):
            path = _check(exes, tbl, data_page_version=version, use_dictionary=False, store_decimal_as_integer=True, column_encoding={c: enc for c in cols})
            assert all(enc in _encodings(path, c) for c in range(len(cols)))
    # a stored INT32 outside a narrow column's range is still refused: the first delta-packed value, 100 -> 300, in the same two
    # bytes, so that the stream stays whole and the values become 300 .. 303
    tbl = pa.table({"v": pa.array([100, 101, 102, 103], pa.int8())})
    for enc in ("DELTA_BINARY_PACKED", "BYTE_STREAM_SPLIT"):
        path = _check(exes, tbl, use_dictionary=False, column_encoding={"v": enc})
        data, pages = _pages(path, 0)
        if enc == "DELTA_BINARY_PACKED":
            at = data.index(bytes([0x80, 0x01, 0x04, 0x04, 0xC8, 0x01]), pages[0]["payload"]) + 4    # block 128, 4 miniblocks, 4 values, first = zigzag(100)
            new = b"\xd8\x04"                                                                          # zigzag(300)
        else:
            at = data.index(bytes([100, 101, 102, 103, 0, 0, 0, 0]), pages[0]["payload"]) + 4         # the second bytes of the four values
            new = b"\x01"                                                                              # 100 -> 356
        assert pages[0]["payload"] <= at < pages[0]["payload"] + pages[0]["size"]
        _reason(exes, _patched(exes, data, at, new), tbl.schema, {R_RANGE})


def test_strings_the_empty_one_and_a_long_one(exes):
    big = "".join(chr(97 + k % 26) for k in range(200_000))
    tbl = pa.table({"s": ["a", big, None, "", "b", big[:70000], ""]})
    for version in ("1.0", "2.0"):
        _check(exes, tbl, data_page_version=version, use_dictionary=False, column_encoding={"s": "DELTA_LENGTH_BYTE_ARRAY"})
        _check(exes, tbl, data_page_version=version, use_dictionary=False, column_encoding={"s": "DELTA_LENGTH_BYTE_ARRAY"}, compression="snappy", level=2)
    _check(exes, pa.table({"s": pa.array(["", "", ""])}), use_dictionary=False, column_encoding={"s": "DELTA_LENGTH_BYTE_ARRAY"})


def test_a_projection(exes):
    n = 1500
    tbl = typed_table(n, _null_patterns(n)["random"])
    for kind in ("v2 snappy", "v2 delta", "v1 bss"):
        for columns in (["s", "i32", "f64"], ["d", "b"], ["m"], ["i64"]):
            _check(exes, tbl, columns=columns, **KINDS[kind])


# ---------------------------------------------------------------- raw DELTA_BINARY_PACKED streams
def _zigzag(v):
    return ((v << 1) ^ (v >> 63)) & (2 ** 64 - 1)


def _signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def delta_model(data, width, count):
    """a byte-serial reader: (values as unsigned integers of the width, the byte position where the stream ended)"""
    bits, pos = width * 8, 0

    def varint():
        nonlocal pos
        v = shift = 0
        while True:
            c = data[pos]
            pos += 1
            v |= (c & 0x7F) << shift
            shift += 7
            if not c & 0x80:
                return v

    def unzig(z):
        return (z >> 1) ^ -(z & 1)
    block, mpb, total, first = varint(), varint(), varint(), unzig(varint())
    assert total == count
    vpm, mask = block // mpb, (1 << bits) - 1
    out = [first & mask] if total else []
    while len(out) < total:
        min_delta = unzig(varint())
        widths = data[pos:pos + mpb]
        pos += mpb
        for m in range(mpb):
            if len(out) >= total:
                break
            w = widths[m]
            packed = int.from_bytes(data[pos:pos + vpm * w // 8], "little")
            pos += vpm * w // 8
            for k in range(vpm):
                if len(out) < total:
                    out.append((out[-1] + min_delta + ((packed >> (k * w)) & ((1 << w) - 1))) & mask)
    return out, pos


def make_stream(rng, width, count, block, mpb, width_of, garbage=False, total=None):
    """a hand-made stream of `count` values: miniblock m of block b holds deltas of exactly width_of(b, m) bits. Returns
    (bytes, values). garbage: arbitrary width bytes behind the last miniblock that holds a value, arbitrary padding in it."""
    bits = width * 8
    mask, vpm = (1 << bits) - 1, block // mpb
    first = rng.randint(-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    out = bytearray(_uleb(block) + _uleb(mpb) + _uleb(count if total is None else total) + _uleb(_zigzag(first)))
    values = [first & mask] if count else []
    b = 0
    while len(values) < count:
        min_delta = rng.randint(-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
        out += _uleb(_zigzag(min_delta))
        ws, body = [], bytearray()
        for m in range(mpb):
            if len(values) >= count:
                ws.append(rng.randint(0, 255) if garbage else 0)
                continue
            w = width_of(b, m)
            packed = 0
            for k in range(vpm):
                d = (rng.getrandbits(w) | (1 << (w - 1))) if w else 0
                if len(values) < count:
                    values.append((values[-1] + min_delta + d) & mask)
                elif not garbage:
                    d = 0
                packed |= d << (k * w)
            ws.append(w)
            body += packed.to_bytes(vpm * w // 8, "little")
        out += bytes(ws) + body
        b += 1
    return bytes(out), values


GEOMETRIES = [(128, 1), (128, 4), (256, 8), (1024, 32), (65536, 1), (384, 4)]        # (384 / 4: miniblocks of 96, no power of two)


def good_delta_streams():
    """{name: (bytes, width, count, values)}"""
    rng = random.Random(17)
    out = {}
    for width in (4, 8):
        bits = width * 8
        for block, mpb in GEOMETRIES:
            vpm = block // mpb
            counts = sorted({0, 1, 2, vpm, vpm + 1, vpm + 2, 2 * vpm + 1, block, block + 1, block + 2, 2 * block + 1, block + vpm + 1, 63, 64, 65, 66})
            if block == 65536:
                counts = [1, 2, 65, block + 1, block + 2]
            for count in counts:
                s, vals = make_stream(rng, width, count, block, mpb, lambda b, m: rng.randint(0, bits), garbage=count % 2 == 1)
                out["%d/%d x%d n=%d" % (block, mpb, width, count)] = (s, width, count, vals)
        for w in range(bits + 1):                                                    # every width, in one block of 128 / 4 and one of 256 / 8
            for block, mpb in ((128, 4), (256, 8)):
                s, vals = make_stream(rng, width, block + 1 + block // 2, block, mpb, lambda b, m: w if (b + m) % 2 == 0 else rng.randint(0, bits))
                out["w=%d %d/%d x%d" % (w, block, mpb, width)] = (s, width, len(vals), vals)
    return out


def hostile_delta_streams():
    """{name: (bytes, width, count, reason)}"""
    rng = random.Random(23)
    head = lambda block, mpb, total, first=0: _uleb(block) + _uleb(mpb) + _uleb(total) + _uleb(_zigzag(first))     # noqa: E731
    good, vals = make_stream(rng, 4, 300, 128, 4, lambda b, m: 7)
    g64, _ = make_stream(rng, 8, 300, 256, 4, lambda b, m: 13)
    _, end = delta_model(good, 4, 300)
    assert end == len(good)
    first_block = len(head(128, 4, 300)) - 1 + len(_uleb(_zigzag(_signed(vals[0], 32))))      # where the first block's min delta begins
    wb = first_block + 1
    while good[wb - 1] & 0x80:
        wb += 1                                                                                 # ... and its four width bytes
    rest = good[first_block:]
    out = {
        "a varint that does not end": (b"\xff" * 12 + good, 4, 300, R_DELTA_VARINT),
        "a first value of eleven bytes": (_uleb(128) + _uleb(4) + _uleb(300) + b"\x80" * 10 + b"\x01" + rest, 4, 300, R_DELTA_VARINT),
        "an empty stream": (b"", 4, 1, R_DELTA_SHORT),
        "a stream that ends inside its header": (good[:2], 4, 300, R_DELTA_SHORT),
        "block size 0": (head(0, 4, 300) + rest, 4, 300, R_DELTA_GEOMETRY),
        "a block size that is no multiple of 128": (head(192, 2, 300) + rest, 4, 300, R_DELTA_GEOMETRY),
        "no miniblocks": (head(128, 0, 300) + rest, 4, 300, R_DELTA_GEOMETRY),
        "miniblocks that do not divide the block": (head(128, 3, 300) + rest, 4, 300, R_DELTA_GEOMETRY),
        "more miniblocks than values": (head(128, 256, 300) + rest, 4, 300, R_DELTA_GEOMETRY),
        "16 values per miniblock": (head(128, 8, 300) + rest, 4, 300, R_DELTA_GEOMETRY),
        "a block above the cap": (head(131072, 4, 300) + rest, 4, 300, R_DELTA_LARGE),
        "a block of 2^40": (head(1 << 40, 4, 300) + rest, 4, 300, R_DELTA_LARGE),
        "a count below the rows": (good, 4, 301, R_DELTA_COUNT),
        "a count above the rows": (good, 4, 299, R_DELTA_COUNT),
        "a count of 2^33": (head(128, 4, 1 << 33) + rest, 4, 300, R_DELTA_COUNT),
        "the end inside a block header": (good[:first_block], 4, 300, R_DELTA_SHORT),
        "the end inside the width bytes": (good[:wb + 3], 4, 300, R_DELTA_SHORT),
        "the end inside the first miniblock": (good[:wb + 4 + 10], 4, 300, R_DELTA_SHORT),
        "the end inside the last miniblock": (good[:-1], 4, 300, R_DELTA_SHORT),
        "the end in front of the second block": (good[:wb + 4 + 4 * 28], 4, 300, R_DELTA_SHORT),
        "a width of 33 bits for INT32": (good[:wb] + b"\x21" + good[wb + 1:], 4, 300, R_DELTA_WIDTH),
        "a width of 255": (good[:wb + 2] + b"\xff" + good[wb + 3:], 4, 300, R_DELTA_WIDTH),
        "a width of 65 bits for INT64": (g64[:g64.index(b"\x0d\x0d\x0d\x0d")] + b"\x41" + g64[g64.index(b"\x0d\x0d\x0d\x0d") + 1:], 8, 300, R_DELTA_WIDTH),
        "widths of 64 bits in a stream of 4 bytes": (head(65536, 1, 65537) + b"\x00\x40", 8, 65537, R_DELTA_SHORT),
    }
    assert good[wb:wb + 4] == b"\x07\x07\x07\x07"
    return out


def cpu_model_delta(exe, workdir, streams):
    """[(bytes, width, count)] through the C++ loops: per stream (values, end) or the reason"""
    path = str(workdir / "delta_streams.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(streams)))
        for s, width, count in streams:
            f.write(struct.pack("<III", len(s), width, count) + s)
    out = []
    for line in _finish(subprocess.run([exe, "delta", path], capture_output=True)):
        parts = line.split()
        out.append(int(parts[1]) if parts[0] == "REASON" else ([int(v) for v in parts[2:]], int(parts[1])))
    assert len(out) == len(streams)
    return out


def test_the_model_reads_what_pyarrow_writes(exes):
    """pyarrow's two geometries (128 / 4 for INT32, 256 / 4 for INT64), its padded last miniblock and omitted ones"""
    rng = np.random.default_rng(3)
    streams, want = [], []
    for t, width, geometry in ((pa.int32(), 4, (128, 4)), (pa.int64(), 8, (256, 4))):
        for n in (1, 2, 33, 34, 65, 66, 129, 130, 257, 258, 1000):
            vals = rng.integers(-1000, 1000, n).astype(t.to_pandas_dtype())
            tbl = pa.table([pa.array(vals, t)], schema=pa.schema([pa.field("v", t, nullable=False)]))
            path = str(exes["dir"] / "pin.parquet")
            pq.write_table(tbl, path, compression="NONE", use_dictionary=False, column_encoding={"v": "DELTA_BINARY_PACKED"}, data_page_version="1.0")
            data, pages = _pages(path, 0)
            assert len(pages) == 1
            page = data[pages[0]["payload"]:pages[0]["payload"] + pages[0]["size"]]
            got, end = delta_model(page, width, n)
            assert end == len(page) and [_signed(v, width * 8) for v in got] == vals.tolist()
            assert ((page[0] & 0x7F) | (page[1] & 0x7F) << 7, page[2]) == geometry
            streams.append((page, width, n))
            want.append((got, end))
    for which in BOTH:
        assert cpu_model_delta(exes[which], exes["dir"], streams) == want


def test_hand_made_streams_of_every_geometry_and_width(exes):
    good = good_delta_streams()
    for name, (s, width, count, vals) in good.items():
        assert delta_model(s, width, count) == (vals, len(s)), name
    names = list(good)
    for which in BOTH:
        got = cpu_model_delta(exes[which], exes["dir"], [good[k][:3] for k in names])
        for name, g in zip(names, got):
            assert g == (good[name][3], len(good[name][0])), name
    # bytes behind the stream are not its own: the end position says where it stopped
    s, width, count, vals = good["256/8 x8 n=65"]
    for which in BOTH:
        assert cpu_model_delta(exes[which], exes["dir"], [(s + b"\xff" * 9, width, count)]) == [(vals, len(s))]


def test_hostile_streams_each_with_its_reason(exes):
    hostile = hostile_delta_streams()
    names = list(hostile)
    for which in BOTH:
        got = cpu_model_delta(exes[which], exes["dir"], [hostile[k][:3] for k in names])
        for name, g in zip(names, got):
            assert g == hostile[name][3], (name, g)
    # a good stream cut at every byte, and damaged at every byte: a reason or values, never a report
    rng = random.Random(5)
    s, width, count, _ = good_delta_streams()["256/8 x4 n=289"]
    cuts = [(s[:k], width, count) for k in range(len(s))]
    got = cpu_model_delta(exes["san"], exes["dir"], cuts)
    assert all(isinstance(g, int) for g in got)
    flips = [(s[:k] + bytes([rng.choice([0, 0xFF, 0x80, s[k] ^ 1])]) + s[k + 1:], width, count) for k in range(len(s))]
    cpu_model_delta(exes["san"], exes["dir"], flips)


# ---------------------------------------------------------------- hostile files
def hostile_table():
    k = np.arange(200)
    return pa.table({"i": pa.array(k % 3 * 1000, pa.int64(), mask=k % 5 == 0), "s": pa.array(["str%d" % (v % 3) for v in k], mask=k % 7 == 0),
                     "b": pa.array(k % 2 == 0), "f": pa.array(k / 3.0, mask=k % 2 == 1)})


HOSTILE_ENC = {"i": "DELTA_BINARY_PACKED", "s": "DELTA_LENGTH_BYTE_ARRAY", "f": "BYTE_STREAM_SPLIT"}


def _shorter(field, new_value):
    """the zigzag varint of new_value in exactly the bytes the field has"""
    _, at, n = field
    z = _uleb((new_value << 1) ^ (new_value >> 63))
    assert len(z) == n, (len(z), n)
    return at, z


def damaged_files(path):
    """{what: (the file's bytes, the reasons that may answer)} for a file of hostile_table() written V2 with HOSTILE_ENC, no
    dictionary, data_page_size=600, write_batch_size=50"""
    data, pages = _pages(path, 0)
    _, spages = _pages(path, 1)
    _, bpages = _pages(path, 2)
    _, fpages = _pages(path, 3)
    pg, h = pages[0], pages[0]["h"][8]
    assert pg["type"] == 3 and h[4][0] == 5 and spages[0]["h"][8][4][0] == 6 and bpages[0]["h"][8][4][0] == 3 and fpages[0]["h"][8][4][0] == 9

    def put(at, new):
        return data[:at] + new + data[at + len(new):]
    n, nulls, lev = h[1][0], h[2][0], h[5][0]
    stream = pg["payload"] + lev
    fh = fpages[0]["h"][8]
    fl = fpages[0]["payload"]                       # the first byte of f's levels: a bit-packed run header, then the bits
    assert data[fl] & 1 and data[fl + 1] == 0x55
    sp = spages[0]["payload"] + spages[0]["h"][8][5][0]
    assert data[sp:sp + 4] == bytes([0x80, 0x01, 0x04]) + _uleb(spages[0]["h"][8][1][0] - spages[0]["h"][8][2][0])[:1]
    first_len = sp + 3 + len(_uleb(spages[0]["h"][8][1][0] - spages[0]["h"][8][2][0]))
    assert data[first_len] == 0x08                  # "str1" (row 0 is NULL): zigzag(4)
    bp = bpages[0]["payload"] + bpages[0]["h"][8][5][0]
    out = {"repetition levels present": (put(*_shorter(h[6], 1)), {R_V2_REPETITION}),
           "num_rows that is not num_values": (put(*_shorter(h[3], n - 1)), {R_V2_ROWS}),
           "num_nulls that is not what the levels say": (put(*_shorter(h[2], nulls - 1)), {R_V2_NULLS}),
           "num_nulls above num_values": (put(h[2][1], _max_varint(h[2][2])), {R_V2_NULLS, 3}),
           "a delta count that is not the non-NULL rows": (put(stream + 3, bytes([data[stream + 3] ^ 1])), {R_DELTA_COUNT}),
           "a delta block size of 0": (put(stream, b"\x80\x00"), {R_DELTA_GEOMETRY}),
           "a negative DELTA_LENGTH_BYTE_ARRAY length": (put(first_len, b"\x07"), {R_DELTA_LENGTH}),
           "lengths that pass the page": (put(first_len, b"\x7e"), {R_DELTA_LENGTH}),
           "a BYTE_STREAM_SPLIT region of the wrong size": (put(fl + 1, b"\x57"), {R_BSS_SIZE, R_V2_NULLS}),
           "an RLE Boolean length past the page": (put(bp, struct.pack("<I", bpages[0]["size"] - bpages[0]["h"][8][5][0] - 3)), {R_RLE_LENGTH}),
           "an RLE Boolean length of 2^31": (put(bp, struct.pack("<I", 0x80000000)), {R_RLE_LENGTH})}
    assert fh[5][0] > 0
    return out


def _hostile_file(exes, version="2.0"):
    tbl = hostile_table()
    path = _check(exes, tbl, name="hostile2.parquet", data_page_version=version, use_dictionary=False, column_encoding=HOSTILE_ENC, data_page_size=600,
                  write_batch_size=50)
    return tbl, path


def test_fields_that_point_outside_their_page_each_with_its_reason(exes):
    tbl, path = _hostile_file(exes)
    for what, (data, reasons) in damaged_files(path).items():
        _reason(exes, _patched(exes, data, 0, b""), tbl.schema, reasons)
        _reason(exes, _patched(exes, data, 0, b""), tbl.schema, {R_PAGE_V2}, encodings=1)
    # V2 level lengths past the page: 250 bytes of levels, so that the varint has room for more than the page holds
    k = np.arange(2000)
    lv = pa.table({"x": pa.array(k.astype(np.int32), mask=k % 2 == 1)})
    lpath = _check(exes, lv, name="lev.parquet", data_page_version="2.0", use_dictionary=False)
    data, pages = _pages(lpath, 0)
    h = pages[0]["h"][8]
    assert len(pages) == 1 and h[5][2] == 2 and pages[0]["size"] < 8191
    _reason(exes, _patched(exes, data, h[5][1], _max_varint(2)), lv.schema, {R_V2_LEVELS})
    _reason(exes, _patched(exes, data, h[5][1], _uleb((pages[0]["size"] + 1) << 1)), lv.schema, {R_V2_LEVELS})
    # the BYTE_STREAM_SPLIT region on a V1 page, where no num_nulls stands in the way: one more level bit set
    tbl1, path1 = _hostile_file(exes, "1.0")
    data, pages = _pages(path1, 3)
    p = pages[0]["payload"]
    assert data[p + 4] & 1 and data[p + 5] == 0x55
    _reason(exes, _patched(exes, data, p + 5, b"\x57"), tbl1.schema, {R_BSS_SIZE})
    # the RLE Boolean length on a V1 page of a required column: the values begin the page
    req = pa.table([pa.array(np.arange(100) % 3 == 0)], schema=pa.schema([pa.field("b", pa.bool_(), nullable=False)]))
    rpath = _check(exes, req, name="rle.parquet", use_dictionary=False, column_encoding={"b": "RLE"})
    data, pages = _pages(rpath, 0)
    for v in (pages[0]["size"] - 3, 0xFFFFFFFF):
        _reason(exes, _patched(exes, data, pages[0]["payload"], struct.pack("<I", v)), req.schema, {R_RLE_LENGTH})


def test_a_page_marked_uncompressed_in_a_snappy_chunk(exes):
    """is_compressed = false: pyarrow writes such pages where Snappy does not help, and they are decoded where they lie; one so
    marked whose two sizes differ is refused. The field is a Boolean of the compact protocol, its value in the field header's
    type nibble (1 true, 2 false) right behind repetition_levels_byte_length, so it is overwritten in place."""
    n = 1000
    tbl = typed_table(n, _null_patterns(n)["seventh"])
    path = _check(exes, tbl, name="marked.parquet", **KINDS["v2 snappy"])
    marked = {name: [pg["h"][8][7] for pg in _pages(path, c)[1] if pg["type"] == 3] for c, name in enumerate(tbl.column_names)}
    assert not any(marked["i32"]) and all(marked["b"]), marked        # (both kinds are in the file that was just decoded)
    data, pages = _pages(path, tbl.column_names.index("b"))
    h = pages[0]["h"]
    assert h[2][0] != h[3][0]
    at = h[8][6][1] + h[8][6][2]
    assert data[at] == 0x11
    bad = _patched(exes, data, at, b"\x12")
    assert _pages(bad, tbl.column_names.index("b"))[1][0]["h"][8][7] is False
    _reason(exes, bad, tbl.schema, {R_V2_UNCOMPRESSED}, level=2)
    _reason(exes, bad, tbl.schema, {R_PAGE_V2}, level=2, encodings=1)
    # the other way round, a page that lies there uncompressed and is marked compressed: its first bytes (the index width, a run
    # header) are no Snappy preamble of the size the header states, which the page walk checks before anything is unpacked
    data, pages = _pages(path, 0)
    at = pages[-1]["h"][8][6][1] + pages[-1]["h"][8][6][2]
    assert data[at] == 0x12
    _reason(exes, _patched(exes, data, at, b"\x11"), tbl.schema, {R_SNAPPY_PREAMBLE}, level=2)


def test_a_v1_page_that_also_carries_a_v2_header_is_read_as_v1(exes):
    """PageHeader by hand: type, the two sizes, data_page_header {10 values, PLAIN, RLE, RLE} and data_page_header_v2 {7 values, 0
    NULLs, 7 rows, DELTA_BINARY_PACKED, 0, 0}. num_values and encoding are the struct's that the page's type names, at either set"""
    zz = lambda v: _uleb(v << 1)                                                                             # noqa: E731
    v1 = b"\x2c" + b"\x15" + zz(10) + b"\x15" + zz(0) + b"\x15" + zz(3) + b"\x15" + zz(3) + b"\x00"
    v2 = b"\x3c" + b"\x15" + zz(7) + b"\x15" + zz(0) + b"\x15" + zz(7) + b"\x15" + zz(5) + b"\x15" + zz(0) + b"\x15" + zz(0) + b"\x00"
    for which in BOTH:
        for ptype, set2, want in ((0, 0, "0 10 0 0"), (0, 1, "0 10 0 1"), (3, 1, "3 7 5 1"), (3, 0, "3 10 0 0")):
            head = b"\x15" + zz(ptype) + b"\x15" + zz(40) + b"\x15" + zz(40) + v1 + v2 + b"\x00"
            got = _finish(subprocess.run([exes[which], "header", head.hex(), str(set2)], capture_output=True))
            assert got == ["%s %d" % (want, len(head))], (ptype, set2, got)


def test_at_set_1_every_file_answers_as_before(exes):
    n = 300
    tbl = typed_table(n, _null_patterns(n)["seventh"])
    for kind, kw in KINDS.items():
        kw = dict(kw)
        level = kw.pop("level", 1)
        path = str(exes["dir"] / "set1.parquet")
        pq.write_table(tbl, path, **dict({"compression": "NONE"}, **kw))
        _reason(exes, path, pq.read_schema(path), {R_PAGE_V2 if kind.startswith("v2") else R_ENCODING}, level=level, encodings=1)
    # what still needs the host at set 2
    base = pa.table({"s": pa.array(["v%d" % (v % 9) for v in range(n)])})
    for version in ("1.0", "2.0"):
        path = str(exes["dir"] / "dba.parquet")
        pq.write_table(base, path, compression="NONE", use_dictionary=False, column_encoding={"s": "DELTA_BYTE_ARRAY"}, data_page_version=version)
        _reason(exes, path, base.schema, {R_ENCODING})
    path = str(exes["dir"] / "v2snappy.parquet")
    pq.write_table(base, path, compression="snappy", data_page_version="2.0")
    _reason(exes, path, base.schema, {7}, level=1)                       # (the codec is the format level's business)


def test_truncation_and_random_damage_never_read_outside(exes):
    tbl, path = _hostile_file(exes)
    data = open(path, "rb").read()
    flen = struct.unpack("<I", data[-8:-4])[0]
    footer = len(data) - 8 - flen
    tail = data[footer:]
    cuts = set()
    for col in range(4):
        for pg in _pages(path, col)[1]:
            lev = pg["h"][8][5][0]
            cuts |= {pg["header"], pg["header"] + 1, pg["payload"] - 1, pg["payload"], pg["payload"] + 1, pg["payload"] + lev - 1, pg["payload"] + lev,
                     pg["payload"] + lev + 1, pg["payload"] + lev + 4, pg["payload"] + lev + 6, pg["payload"] + (pg["size"] + lev) // 2, pg["payload"] + pg["size"] - 1}
    for cut in sorted(c for c in cuts if 4 < c < footer):
        got = _decode(exes, "san", _patched(exes, data[:cut] + tail, 0, b""), tbl.schema)
        assert len(got) == 1 and got[0].startswith("NEEDS_HOST "), (cut, got[:2])
    rng = random.Random(3)
    for at in range(4, footer, 3):
        got = _decode(exes, "san", _patched(exes, data, at, bytes([rng.choice([0x00, 0xFF, 0x7F, 0x80, data[at] ^ 1])])), tbl.schema)
        assert got[0].startswith("NEEDS_HOST ") or got[0].startswith("ROWS "), (at, got[:1])
    # the same with Snappy around the values
    spath = _check(exes, tbl, name="hostile2s.parquet", level=2, data_page_version="2.0", use_dictionary=False, column_encoding=HOSTILE_ENC, data_page_size=600,
                   write_batch_size=50, compression="snappy")
    sdata = open(spath, "rb").read()
    sfooter = len(sdata) - 8 - struct.unpack("<I", sdata[-8:-4])[0]
    for at in range(4, sfooter, 5):
        got = _decode(exes, "san", _patched(exes, sdata, at, bytes([rng.choice([0x00, 0xFF, 0x7F, 0x80, sdata[at] ^ 1])])), tbl.schema, level=2)
        assert got[0].startswith("NEEDS_HOST ") or got[0].startswith("ROWS "), (at, got[:1])
