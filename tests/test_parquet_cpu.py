"""The device Parquet decoder without a GPU: tests/cpp/parquet_tests.cpp contains the host half as it is
(csrc/parquet_meta.hpp: the Thrift reader, the footer and the page walk) and the per-run and per-value code of the kernels
(csrc/device/qhip_parquet.inc), and decodes whole files page by page into a text dump, which is compared with
`pyarrow.parquet.read_table` on the same bytes. Built with g++ as a stand-alone program (nothing of it is loaded into Python),
once plainly and once with the address and undefined-behaviour sanitizers; every buffer is a heap allocation of exactly the
size of its data, so a read outside the file, a page or a column is a report, and every hostile file must end in a reason."""
import datetime
import decimal
import os
import random
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qurious_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "cpp", "parquet_tests.cpp")
FLAGS = ["-std=c++17", "-g", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
SAN = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
BOTH = ("plain", "san")

(R_MAGIC, R_ENCRYPTED, R_CORRUPT, R_NESTED, R_SCHEMA, R_TYPE, R_CODEC, R_FILE_PATH, R_PAGE_V2, R_INDEX_PAGE, R_PAGE_ORDER, R_ENCODING, R_LEVEL_ENCODING,
 R_REPEATED, R_NO_ROWS, R_TOO_MANY_COLUMNS, R_TOO_MANY_ROWS, R_NUM_VALUES, R_LEVELS_LENGTH, R_RUN, R_RUN_COUNT, R_LEVEL_VALUE, R_BIT_WIDTH, R_VALUES_SHORT,
 R_DICT_INDEX, R_BYTE_ARRAY, R_RANGE, R_UTF8_LONG) = range(1, 29)

TYPE_CODE = {pa.int8(): "i8", pa.int16(): "i16", pa.int32(): "i32", pa.int64(): "i64", pa.uint8(): "u8", pa.uint16(): "u16", pa.uint32(): "u32",
             pa.uint64(): "u64", pa.float32(): "f32", pa.float64(): "f64", pa.date32(): "date", pa.string(): "utf8", pa.bool_(): "bool",
             pa.timestamp("ms"): "ts3", pa.timestamp("us"): "ts6", pa.timestamp("ns"): "ts9"}


def _code(t):
    if pa.types.is_decimal128(t):
        return f"dec:{t.precision}:{t.scale}"
    return TYPE_CODE.get(t, "x")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("parquet_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


def _finish(r):
    assert r.returncode == 0, r.stderr.decode()
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()
    return r.stdout.decode().split("\n")[:-1]


def _decode(exes, which, path, schema, proj=None):
    args = [exes[which], "decode", path, ",".join(_code(f.type) for f in schema), ",".join(map(str, proj)) if proj else "-"]
    return _finish(subprocess.run(args, capture_output=True))


def _cell(v, t):
    if v is None:
        return "N"
    if pa.types.is_float64(t):
        return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]
    if pa.types.is_float32(t):
        return "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]
    if pa.types.is_date32(t):
        return str((v - datetime.date(1970, 1, 1)).days)
    if pa.types.is_decimal(t):
        return str(int(v.scaleb(t.scale, context=decimal.Context(prec=100))))
    if pa.types.is_string(t):
        return "s" + v.encode().hex()
    if pa.types.is_boolean(t):
        return "1" if v else "0"
    return str(v)


def _expect(tbl):
    cols = []
    for c, f in zip(tbl.columns, tbl.schema):
        if pa.types.is_timestamp(f.type):
            c = c.cast(pa.int64())
        if pa.types.is_floating(f.type):     # (bit patterns: a NaN's payload and -0.0 count)
            width = "<u4" if pa.types.is_float32(f.type) else "<u8"
            fmt = "%08x" if pa.types.is_float32(f.type) else "%016x"
            bits = c.combine_chunks().fill_null(0).to_numpy(zero_copy_only=False).view(width)
            valid = c.combine_chunks().is_valid().to_pylist()
            cols.append([fmt % b if ok else "N" for b, ok in zip(bits.tolist(), valid)])
        else:
            cols.append([_cell(v, f.type) for v in c.to_pylist()])
    return ["ROWS %d" % tbl.num_rows, "NULLS " + " ".join(str(c.null_count) for c in tbl.columns)] + ["\t".join(r) for r in zip(*cols)]


def _write(exes, tbl, name="t.parquet", **kw):
    path = str(exes["dir"] / name)
    kw.setdefault("compression", "NONE")
    pq.write_table(tbl, path, **kw)
    return path


def _check(exes, tbl, which=BOTH, columns=None, **kw):
    path = _write(exes, tbl, **kw)
    schema = pq.read_schema(path)
    want = _expect(pq.read_table(path, columns=columns))
    proj = [schema.get_field_index(c) for c in columns] if columns else None
    for w in which:
        got = _decode(exes, w, path, schema, proj)
        assert got == want, (got[:3], want[:3])
    return path


def _needs_host(exes, path, schema, reason, proj=None, which=BOTH):
    for w in which:
        got = _decode(exes, w, path, schema, proj)
        assert len(got) == 1 and got[0].startswith("NEEDS_HOST %d " % reason), (got[:2], reason)


# ---------------------------------------------------------------- a page walk of the test's own (Thrift compact protocol)
def _varint(b, p):
    v = shift = 0
    while True:
        c = b[p]
        p += 1
        v |= (c & 0x7F) << shift
        shift += 7
        if not c & 0x80:
            return v, p


def _struct(b, p):
    """{field id: value} of the struct at b[p:]; an integer field is (value, offset, length), a struct field a dict"""
    out, last = {}, 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return out, p
        ty, delta = h & 15, h >> 4
        if delta:
            fid = last + delta
        else:
            z, p = _varint(b, p)
            fid = (z >> 1) ^ -(z & 1)
        last = fid
        if ty in (1, 2):
            out[fid] = ty == 1
        elif ty == 3:
            out[fid] = (b[p], p, 1)
            p += 1
        elif ty in (4, 5, 6):
            z, q = _varint(b, p)
            out[fid] = ((z >> 1) ^ -(z & 1), p, q - p)
            p = q
        elif ty == 7:
            p += 8
        elif ty == 8:
            n, p = _varint(b, p)
            p += n
        elif ty == 12:
            out[fid], p = _struct(b, p)
        elif ty in (9, 10):
            h2 = b[p]
            p += 1
            n, et = h2 >> 4, h2 & 15
            if n == 15:
                n, p = _varint(b, p)
            for _ in range(n):
                if et == 12:
                    _, p = _struct(b, p)
                elif et == 8:
                    m, p = _varint(b, p)
                    p += m
                elif et in (4, 5, 6):
                    _, p = _varint(b, p)
                else:
                    p += 1
        else:
            raise AssertionError("thrift type %d" % ty)


def _pages(path, column=0, row_group=0):
    """the pages of one chunk: dicts with the header's fields (value, offset, length) and `payload`, `size`, `header`"""
    data = open(path, "rb").read()
    cm = pq.ParquetFile(path).metadata.row_group(row_group).column(column)
    pos = cm.dictionary_page_offset if cm.has_dictionary_page and cm.dictionary_page_offset else cm.data_page_offset
    end, rows, out = pos + cm.total_compressed_size, 0, []
    while pos < end and rows < cm.num_values:
        h, q = _struct(data, pos)
        pg = {"header": pos, "payload": q, "size": h[3][0], "type": h[1][0], "h": h}
        if 5 in h:
            rows += h[5][1][0]
        out.append(pg)
        pos = q + h[3][0]
    return data, out


def _max_varint(length):
    """the largest zigzag value a varint of `length` bytes holds"""
    return bytes([0xFE] + [0xFF] * (length - 2) + [0x7F]) if length > 1 else bytes([0x7E])


def _patched(exes, data, at, new, name="bad.parquet"):
    path = str(exes["dir"] / name)
    with open(path, "wb") as f:
        f.write(data[:at] + new + data[at + len(new):])
    return path


# ---------------------------------------------------------------- types
DEC_PRECISIONS = [2, 4, 6, 9, 11, 14, 16, 18, 21, 23, 26, 28, 31, 33, 35, 38]    # FIXED_LEN_BYTE_ARRAY lengths 1 .. 16


def test_every_type_at_its_limits(exes):
    def ints(t, lo, hi):
        return pa.array([lo, hi, 0, None, 1, -1 if lo < 0 else 2, lo + 1, hi - 1], t)
    cols = {
        "i8": ints(pa.int8(), -128, 127), "i16": ints(pa.int16(), -2 ** 15, 2 ** 15 - 1), "i32": ints(pa.int32(), -2 ** 31, 2 ** 31 - 1),
        "i64": ints(pa.int64(), -2 ** 63, 2 ** 63 - 1), "u8": ints(pa.uint8(), 0, 255), "u16": ints(pa.uint16(), 0, 65535),
        "u32": ints(pa.uint32(), 0, 2 ** 32 - 1), "u64": ints(pa.uint64(), 0, 2 ** 64 - 1),
        "f32": pa.array([0.0, -0.0, float("inf"), None, float("nan"), 1.5, -3.4028235e38, 1e-45], pa.float32()),
        "f64": pa.array([0.0, -0.0, float("-inf"), None, float("nan"), 1.5, 1.7976931348623157e308, 5e-324], pa.float64()),
        "d": pa.array([-719162, 2932896, 0, None, 1, -1, 9131, 20000], pa.date32()),
        "b": pa.array([True, False, None, True, True, False, None, False]),
        "s": pa.array(["", "a", None, "ä€\U0001f600", "x" * 70, "nul\x00byte", "", "tab\t"]),
        "ts_s": pa.array([0, 1, None, -1, 2 ** 40, -2 ** 40, 5, 6], pa.timestamp("s")),
        "ts_ms": ints(pa.timestamp("ms"), -2 ** 63, 2 ** 63 - 1), "ts_us": ints(pa.timestamp("us"), -2 ** 63, 2 ** 63 - 1),
        "ts_ns": ints(pa.timestamp("ns"), -2 ** 63, 2 ** 63 - 1),
    }
    for p in DEC_PRECISIONS:
        top = 10 ** p - 1
        vals = [top, -top, 0, None, 1, -1, top // 7, -(top // 3)]
        cols["dec%d" % p] = pa.array([None if v is None else decimal.Decimal(v).scaleb(-(p // 2), context=decimal.Context(prec=100)) for v in vals], pa.decimal128(p, p // 2))
    tbl = pa.table(cols)
    path = _check(exes, tbl)
    lengths = [pq.ParquetFile(path).schema.column(tbl.schema.get_field_index("dec%d" % p)).length for p in DEC_PRECISIONS]
    assert lengths == list(range(1, 17))
    _check(exes, tbl, use_dictionary=False)     # the same values PLAIN
    # decimals stored as INT32 / INT64
    small = tbl.select(["dec2", "dec9", "dec11", "dec18"])
    path = _check(exes, small, store_decimal_as_integer=True)
    assert [pq.ParquetFile(path).schema.column(k).physical_type for k in range(4)] == ["INT32", "INT32", "INT64", "INT64"]
    _check(exes, small, store_decimal_as_integer=True, use_dictionary=False)


@pytest.mark.parametrize("entries", [1, 2, 3, 255, 256, 257, 65537])
def test_dictionaries_of_every_index_width(exes, entries):
    n = max(3 * entries, 1000) if entries < 1000 else entries + 5000
    rng = np.random.default_rng(entries)
    idx = np.concatenate([np.arange(entries), rng.integers(0, entries, n - entries)])
    mask = np.concatenate([np.zeros(entries, dtype=bool), rng.random(n - entries) < 0.1])     # (every distinct value is stored at least once)
    order = rng.permutation(n)
    idx, mask = idx[order], mask[order]
    tbl = pa.table({"k": pa.array(idx * 7 - 3, pa.int64(), mask=mask), "s": pa.array(["v%06d" % i for i in idx], pa.string(), mask=mask),
                    "m": pa.array([decimal.Decimal(int(i)) / 100 for i in idx], pa.decimal128(15, 2))})
    path = _check(exes, tbl, which=("plain",) if entries > 1000 else BOTH)
    data, pages = _pages(path, 0)
    assert pages[0]["type"] == 2 and pages[0]["h"][7][1][0] == entries
    if entries > 1000:
        _check(exes, tbl.slice(0, 70000), which=("san",))


# ---------------------------------------------------------------- hand-made hybrid streams
def _uleb(v):
    out = bytearray()
    while True:
        out.append((v & 0x7F) | (0x80 if v > 0x7F else 0))
        v >>= 7
        if not v:
            return bytes(out)


def _rle(count, value, w):
    return _uleb(count << 1) + value.to_bytes((w + 7) // 8, "little")


def _packed(values, w):
    """a bit-packed run: whole groups of 8 (the caller pads)"""
    assert len(values) % 8 == 0
    bits = 0
    for k, v in enumerate(values):
        bits |= v << (k * w)
    return _uleb((len(values) // 8 << 1) | 1) + bits.to_bytes(len(values) * w // 8, "little")


def _stream(exes, which, w, n, data):
    path = str(exes["dir"] / "stream.bin")
    with open(path, "wb") as f:
        f.write(data)
    return _finish(subprocess.run([exes[which], "stream", str(w), str(n), path], capture_output=True))


@pytest.mark.parametrize("w", range(33))
def test_hand_made_streams_at_every_bit_width(exes, w):
    """RLE and bit-packed runs of 1 .. 130 values in every order (RLE-packed, packed-packed, packed-RLE, RLE-RLE), a last
    bit-packed group padded past the number of values; at width 0 an RLE run's value occupies 0 bytes"""
    rng = random.Random(w)
    top = (1 << w) - 1
    out, want = bytearray(), []
    for n in range(1, 131):
        for kind in ("rle", "packed", "packed", "rle", "rle"):
            if kind == "rle":
                v = rng.randint(0, top)
                out += _rle(n, v, w)
                want += [v] * n
            else:
                vals = [rng.choice([0, top, rng.randint(0, top)]) for _ in range((n + 7) // 8 * 8)]
                out += _packed(vals, w)
                want += vals
    tail = [rng.randint(0, top) for _ in range(24)]
    out += _packed(tail, w)
    want += tail[:19]                       # 5 values of padding behind the last one
    if w == 0:
        assert len(_rle(5, 0, 0)) == 1      # (count > 1, no value byte)
    for which in BOTH:
        got = _stream(exes, which, w, len(want), bytes(out))
        assert got == [str(v) for v in want]
    # a stream that ends early, a run of no values, a bit-packed run whose bytes are cut: reasons, not reads
    for which in BOTH:
        assert _stream(exes, which, w, len(want) + 6, bytes(out)) == ["REASON %d" % R_RUN]
        assert _stream(exes, which, w, 5, _rle(0, 0, w)) == ["REASON %d" % R_RUN]
        if w:
            assert _stream(exes, which, w, 8, _packed([top] * 8, w)[:-1]) == ["REASON %d" % R_RUN]
            assert _stream(exes, which, w, 8, _rle(8, top, w)[:-1]) == ["REASON %d" % R_RUN]
        assert _stream(exes, which, w, 8, b"\xff\xff\xff\xff\xff\x01") == ["REASON %d" % R_RUN]     # a header of more than 32 bits


def _levels(exes, which, first, n, data):
    path = str(exes["dir"] / "levels.bin")
    with open(path, "wb") as f:
        f.write(data)
    return _finish(subprocess.run([exes[which], "levels", str(first), str(n), path], capture_output=True))


def _null_patterns(n, seed=5):
    rng = np.random.default_rng(seed)
    runs = np.zeros(n, dtype=bool)       # NULL runs that cross the 64-row edges
    for edge in range(64, n, 64):
        runs[max(0, edge - 3):edge + 5] = True
    return {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "seventh": np.arange(n) % 7 == 0, "random": rng.random(n) < 0.1, "runs": runs}


def test_level_streams_into_words_shared_with_the_neighbours(exes):
    rng = random.Random(11)
    for first in (0, 1, 63, 64, 65, 100, 127):
        for n in (1, 7, 63, 64, 65, 200, 1000):
            for name, nulls in _null_patterns(n).items():
                valid = [0 if x else 1 for x in nulls]
                out, k = bytearray(), 0
                while k < n:                # a random mix of RLE and bit-packed runs that spells `valid`
                    run = 1
                    while k + run < n and valid[k + run] == valid[k]:
                        run += 1
                    if run >= 8 and rng.random() < 0.8:
                        take = rng.randint(1, run)
                        out += _rle(take, valid[k], 1)
                    else:
                        take = min(n - k, 8 * rng.randint(1, 3))
                        vals = valid[k:k + take]
                        vals += [rng.randint(0, 1) for _ in range(-len(vals) % 8)]     # (padding: only ever behind the last value)
                        if len(vals) != take and k + take < n:
                            take = take // 8 * 8
                            vals = valid[k:k + take]
                        out += _packed(vals, 1)
                    k += take
                for which in BOTH:
                    got = _levels(exes, which, first, n, bytes(out))
                    assert got == ["".join(map(str, valid)), "NONNULL %d NULLS %d" % (sum(valid), n - sum(valid))], (first, n, name)
    for which in BOTH:
        assert _levels(exes, which, 3, 10, _rle(11, 1, 1)) == ["REASON %d" % R_RUN_COUNT]
        assert _levels(exes, which, 3, 10, _packed([1] * 24, 1)) == ["REASON %d" % R_RUN_COUNT]
        assert _levels(exes, which, 3, 10, _rle(10, 2, 1)) == ["REASON %d" % R_LEVEL_VALUE]
        assert _levels(exes, which, 3, 10, _rle(4, 1, 1)) == ["REASON %d" % R_RUN]            # the stream ends before the page's rows do
        assert _levels(exes, which, 3, 10, _packed([1] * 16, 1))[0] == "1" * 10               # one padded group is what writers emit


# ---------------------------------------------------------------- NULL patterns, pages, row groups
LAYOUTS = ({}, {"data_page_size": 64, "write_batch_size": 7}, {"row_group_size": 333})


def _typed_table(n, nulls):
    k = np.arange(n)
    return pa.table({
        "i32": pa.array((k * 7919 % 100003 - 50000).astype(np.int32), mask=nulls), "i64": pa.array(k.astype(np.int64) * 10 ** 10 - 17, mask=nulls),
        "f64": pa.array(k / 7.0, mask=nulls), "d": pa.array((k % 20000).astype(np.int32), pa.int32(), mask=nulls).cast(pa.date32()),
        "m": pa.array([None if x else decimal.Decimal(int(v) - 500) / 100 for v, x in zip(k, nulls)], pa.decimal128(15, 2)),
        "b": pa.array(k % 3 == 0, mask=nulls), "s": pa.array(["row %d" % v if v % 5 else "" for v in k], pa.string(), mask=nulls)})


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_null_patterns_across_page_and_row_group_edges(exes, layout):
    n = 2000
    for name, nulls in _null_patterns(n).items():
        for dictionary in (True, False):
            _check(exes, _typed_table(n, nulls), use_dictionary=dictionary, **LAYOUTS[layout])
    path = _write(exes, _typed_table(n, _null_patterns(n)["seventh"]), **LAYOUTS[layout])
    if layout == 1:
        assert len(_pages(path, 0)[1]) > 50
    if layout == 2:
        assert pq.ParquetFile(path).metadata.num_row_groups == 7


def test_a_required_column_and_a_projection(exes):
    n = 1500
    k = np.arange(n)
    schema = pa.schema([pa.field("r", pa.int64(), nullable=False), pa.field("o", pa.int64()), pa.field("rs", pa.string(), nullable=False),
                        pa.field("rb", pa.bool_(), nullable=False)])
    tbl = pa.table([pa.array(k * 3), pa.array(k, mask=k % 4 == 0), pa.array(["s%d" % v for v in k]), pa.array(k % 2 == 0)], schema=schema)
    for layout in LAYOUTS:
        _check(exes, tbl, **layout)
        _check(exes, tbl, columns=["rs", "r"], **layout)
        _check(exes, tbl, use_dictionary=False, **layout)


def test_the_dictionary_fallback_in_the_middle_of_a_chunk(exes):
    n = 100_000
    tbl = pa.table({"s": pa.array(["%040d" % (k * 2654435761 % 10 ** 30) for k in range(n)], pa.string(), mask=np.arange(n) % 11 == 0)})
    path = _check(exes, tbl)
    encodings = {pg["h"][5][2][0] for pg in _pages(path, 0)[1] if 5 in pg["h"]}
    assert encodings == {0, 8}, encodings     # RLE_DICTIONARY first, PLAIN behind: only the page headers say where


def test_a_long_string(exes):
    big = "".join(chr(97 + k % 26) for k in range(200_000))
    for dictionary in (True, False):
        _check(exes, pa.table({"s": ["a", big, None, "b", big[:70000]]}), use_dictionary=dictionary)


# ---------------------------------------------------------------- what needs the host, each with its own reason
def test_files_outside_the_coverage(exes):
    n = 300
    k = np.arange(n)
    base = pa.table({"i": pa.array(k, pa.int64()), "f": pa.array(k / 3.0), "s": pa.array(["v%d" % (v % 9) for v in k]), "b": pa.array(k % 2 == 0)})

    def case(tbl, reason, proj=None, **kw):
        path = _write(exes, tbl, name="host.parquet", **kw)
        _needs_host(exes, path, pq.read_schema(path), reason, proj)
        return path

    case(base, R_CODEC, compression="snappy")
    case(base, R_CODEC, compression="zstd")
    case(base, R_PAGE_V2, data_page_version="2.0")
    case(base, R_ENCODING, use_dictionary=False, use_byte_stream_split=["f"])
    for col, enc in (("i", "DELTA_BINARY_PACKED"), ("s", "DELTA_LENGTH_BYTE_ARRAY"), ("s", "DELTA_BYTE_ARRAY"), ("b", "RLE")):
        case(base, R_ENCODING, use_dictionary=False, column_encoding={col: enc})
    case(pa.table({"t": pa.array(k, pa.timestamp("ns"))}), R_TYPE, use_deprecated_int96_timestamps=True)
    case(pa.table({"i": k, "l": [[1, 2]] * n}), R_NESTED)
    case(pa.table({"i": k, "l": [[1, 2]] * n}), R_NESTED, proj=[0])               # leaf index != field index: even unprojected
    case(pa.table({"i": k, "st": [{"a": 1}] * n}), R_NESTED)
    case(pa.table({"t": pa.array(k, pa.timestamp("us", tz="UTC"))}), R_TYPE)
    case(pa.table({"t": pa.array(k, pa.timestamp("ms", tz="Europe/Berlin"))}), R_TYPE)
    case(pa.table({"t": pa.array(k, pa.time64("us"))}), R_TYPE)
    case(pa.table({"t": pa.array(k.astype(np.int32), pa.time32("ms"))}), R_TYPE)
    case(pa.table({"t": pa.array(k.astype(np.float16))}), R_TYPE)
    case(pa.table({"t": pa.array([decimal.Decimal(int(v)) for v in k], pa.decimal256(50, 0))}), R_TYPE)
    case(pa.table({"t": pa.array(["x"] * n, pa.large_string())}), R_TYPE)
    case(pa.table({"t": pa.array([b"x"] * n, pa.binary())}), R_TYPE)
    case(pa.table({"t": pa.array(["x"] * n).dictionary_encode()}), R_TYPE)
    case(pa.table({"i": pa.array([], pa.int64())}), R_NO_ROWS)
    case(pa.table({"c%d" % c: k for c in range(65)}), R_TOO_MANY_COLUMNS)
    path = _check(exes, pa.table({"c%d" % c: k for c in range(65)}), columns=["c64", "c0"])          # 64 or fewer of them: fine
    # unprojected columns are not looked at beyond the footer: their codec, encodings and types are irrelevant
    mixed = pa.table({"i": k, "t": pa.array(k, pa.time64("us")), "z": pa.array(k, pa.timestamp("us", tz="UTC")), "s": base["s"]})
    _check(exes, mixed, columns=["s", "i"])
    _check(exes, mixed, columns=["i"], compression={"i": "NONE", "t": "snappy", "z": "zstd", "s": "snappy"})
    # the wrong schema for the file
    path = _write(exes, base)
    for w in BOTH:
        assert _decode(exes, w, path, pa.schema([("i", pa.int64())]))[0].startswith("NEEDS_HOST %d " % R_SCHEMA)
        assert _decode(exes, w, path, pa.schema([("i", pa.int32()), ("f", pa.float64()), ("s", pa.string()), ("b", pa.bool_())]))[0].startswith("NEEDS_HOST %d " % R_TYPE)
    # magic
    data = open(path, "rb").read()
    _needs_host(exes, _patched(exes, data, 0, b"PARE"), base.schema, R_ENCRYPTED)
    _needs_host(exes, _patched(exes, data, len(data) - 4, b"PARE"), base.schema, R_ENCRYPTED)
    _needs_host(exes, _patched(exes, data, 0, b"PAR2"), base.schema, R_MAGIC)
    for cut in (0, 3, 4, 8, 11):
        _needs_host(exes, _patched(exes, data[:cut], 0, b""), base.schema, R_MAGIC)


def test_a_stored_value_outside_a_narrow_column(exes):
    for t, bad in ((pa.int8(), 128), (pa.int8(), -129), (pa.int16(), 40000), (pa.uint8(), 256), (pa.uint8(), -1), (pa.uint16(), 65536)):
        tbl = pa.table({"v": pa.array([1, 2, 3, 4], t)})
        for dictionary in (True, False):
            path = _check(exes, tbl, use_dictionary=dictionary)
            data, pages = _pages(path, 0)
            pg = pages[0]                        # the dictionary page, or the PLAIN data page behind its 6 bytes of levels
            at = pg["payload"] + (0 if dictionary else 6) + 8
            assert data[at:at + 4] == struct.pack("<i", 3)
            _needs_host(exes, _patched(exes, data, at, struct.pack("<i", bad)), tbl.schema, R_RANGE)


# ---------------------------------------------------------------- hostile bytes
def _hostile_base(exes, dictionary=True):
    n = 200
    k = np.arange(n)
    tbl = pa.table({"i": pa.array(k % 3 * 1000, pa.int64(), mask=k % 5 == 0), "s": pa.array(["str%d" % (v % 3) for v in k], mask=k % 7 == 0)})
    path = _check(exes, tbl, name="hostile.parquet", use_dictionary=dictionary, data_page_size=300, write_batch_size=50)
    return tbl, path


def test_truncation_at_every_structural_edge(exes):
    tbl, path = _hostile_base(exes)
    data = open(path, "rb").read()
    flen = struct.unpack("<I", data[-8:-4])[0]
    footer = len(data) - 8 - flen
    tail = data[footer:]
    cuts = {footer + 1, footer + flen // 2, len(data) - 9, len(data) - 5, len(data) - 1}          # inside the footer and its length
    for col in (0, 1):
        for pg in _pages(path, col)[1]:
            cuts |= {pg["header"], pg["header"] + 1, pg["payload"] - 1, pg["payload"], pg["payload"] + 2, pg["payload"] + 4, pg["payload"] + 5,
                     pg["payload"] + pg["size"] // 2, pg["payload"] + pg["size"] - 1}             # inside a header, the levels, the values
    for cut in sorted(cuts):
        _needs_host(exes, _patched(exes, data[:cut], 0, b""), tbl.schema, R_MAGIC, which=("san",))
        if cut < footer:
            # the same cut with the footer put back behind it: the chunk now reaches into the footer or past the data
            got = _decode(exes, "san", _patched(exes, data[:cut] + tail, 0, b""), tbl.schema)
            assert len(got) == 1 and got[0].startswith("NEEDS_HOST "), (cut, got[:2])
    # a footer whose bytes end early (the length still points at its start)
    for keep in (1, flen // 3, flen - 1):
        short = data[:footer] + data[footer:footer + keep] + struct.pack("<I", keep) + b"PAR1"
        _needs_host(exes, _patched(exes, short, 0, b""), tbl.schema, R_CORRUPT)


def test_fields_that_point_outside_their_page(exes):
    tbl, path = _hostile_base(exes)
    data, pages = _pages(path, 0)
    _, spages = _pages(path, 1)
    dict_pg, data_pg = pages[0], pages[1]
    assert dict_pg["type"] == 2 and data_pg["type"] == 0 and spages[0]["type"] == 2

    def bad(at, new, *reasons):
        for w in BOTH:
            got = _decode(exes, w, _patched(exes, data, at, new), tbl.schema)
            assert len(got) == 1 and got[0].startswith("NEEDS_HOST "), got[:2]
            assert int(got[0].split()[1]) in reasons, (got[0], reasons)

    # the footer length
    for v in (0xFFFFFFFF, len(data), len(data) - 11, 0, 1):
        bad(len(data) - 8, struct.pack("<I", v), R_CORRUPT, R_NESTED, R_SCHEMA)
    # a page's two sizes (together, as an uncompressed page has them, and each alone)
    for pg in (dict_pg, data_pg, pages[-1]):
        (_, at2, n2), (_, at3, n3) = pg["h"][2], pg["h"][3]
        assert at3 == at2 + n2 + 1              # (one field header byte in between)
        bad(at2, _max_varint(n2) + data[at2 + n2:at3] + _max_varint(n3), R_CORRUPT)
        bad(at2, _max_varint(n2), R_CORRUPT)
        bad(at3, _max_varint(n3), R_CORRUPT)
        bad(at3, b"\x01" + b"\x00" * (n3 - 1) if n3 == 1 else b"\x81" + b"\x80" * (n3 - 2) + b"\x00", R_CORRUPT)     # a negative size
    # num_values: of a data page (more rows than the row group has left, and a negative count) and of the dictionary
    for pg in (data_pg, pages[-1]):
        _, at, n = pg["h"][5][1]
        bad(at, _max_varint(n), R_NUM_VALUES)
        bad(at, b"\x01" if n == 1 else b"\x81" + b"\x80" * (n - 2) + b"\x00", R_CORRUPT)
    _, at, n = dict_pg["h"][7][1]
    bad(at, _max_varint(n), R_CORRUPT)                     # more entries than the page has bytes for
    _, at, n = spages[0]["h"][7][1]
    for w in BOTH:                                         # (the string dictionary lives in column 1's chunk)
        got = _decode(exes, w, _patched(exes, data, at, _max_varint(n)), tbl.schema)
        assert got[0].split()[:2] in (["NEEDS_HOST", str(R_CORRUPT)], ["NEEDS_HOST", str(R_BYTE_ARRAY)]), got[:2]
    # the levels' length prefix
    p = data_pg["payload"]
    for v in (0xFFFFFFFF, data_pg["size"] - 3, data_pg["size"], 0x7FFFFFFF):
        bad(p, struct.pack("<I", v), R_LEVELS_LENGTH)
    # a level run's count: the first header of the level stream
    lv_len = struct.unpack("<I", data[p:p + 4])[0]
    assert lv_len < 128
    bad(p + 4, b"\x7e", R_RUN_COUNT, R_RUN, R_LEVEL_VALUE)          # an RLE run of 63 ...
    bad(p + 4, b"\x7f", R_RUN, R_RUN_COUNT)                         # ... and 63 bit-packed groups, past the stream
    bad(p + 4, b"\x00", R_RUN)                                       # a run of no values
    # a dictionary index: 3 entries at width 2, every index bit set
    v = p + 4 + lv_len
    assert data[v] == 2
    for at in range(v + 2, p + data_pg["size"]):
        if data[at] != 0xFF:
            got = _decode(exes, "san", _patched(exes, data, at, b"\xff"), tbl.schema)
            assert got[0].split()[1] in (str(R_DICT_INDEX), str(R_RUN)) or got[0].startswith("ROWS"), got[0]
    bad(v + 2, b"\xff", R_DICT_INDEX, R_RUN)
    bad(v, b"\x21", R_BIT_WIDTH)
    bad(v, b"\x20", R_RUN, R_DICT_INDEX)                             # width 32: the runs no longer fit, or the indices are huge
    # a BYTE_ARRAY length: in the dictionary page and in a PLAIN data page
    sp = spages[0]["payload"]
    for at in (sp, sp + 4 + 4):
        for val in (0x7FFFFFFF, 0xFFFFFFFF, spages[0]["size"]):
            for w in BOTH:
                got = _decode(exes, w, _patched(exes, data, at, struct.pack("<I", val)), tbl.schema)
                assert got == ["NEEDS_HOST %d 0 1 0" % R_BYTE_ARRAY], got[:2]
    ptbl, ppath = _hostile_base(exes, dictionary=False)
    pdata, ppages = _pages(ppath, 1)
    pp = ppages[0]["payload"]
    first = pp + 4 + struct.unpack("<I", pdata[pp:pp + 4])[0]
    assert pdata[first:first + 8] == struct.pack("<I", 4) + b"str1"
    for val in (0x7FFFFFFF, 0xFFFFFFFF, ppages[0]["size"]):
        for w in BOTH:
            got = _decode(exes, w, _patched(exes, pdata, first, struct.pack("<I", val)), ptbl.schema)
            assert got == ["NEEDS_HOST %d 0 1 0" % R_BYTE_ARRAY], got[:2]


def test_random_byte_damage_never_reads_outside(exes):
    """every single-byte change of the footer and of the first pages ends in a reason or in a table, never in a report"""
    tbl, path = _hostile_base(exes)
    data = open(path, "rb").read()
    rng = random.Random(3)
    flen = struct.unpack("<I", data[-8:-4])[0]
    spots = list(range(len(data) - 8 - flen, len(data) - 8, 7)) + list(range(4, 400, 3))
    for at in spots:
        path = _patched(exes, data, at, bytes([rng.choice([0x00, 0xFF, 0x7F, 0x80, data[at] ^ 1])]))
        got = _decode(exes, "san", path, tbl.schema)
        assert got[0].startswith("NEEDS_HOST ") or got[0].startswith("ROWS "), (at, got[:1])


# ---------------------------------------------------------------- the damaged files tests/test_gpu_parquet.py runs on the device
def hostile_table():
    k = np.arange(200)
    return pa.table({"i": pa.array(k % 3 * 1000, pa.int64(), mask=k % 5 == 0), "s": pa.array(["str%d" % (v % 3) for v in k], mask=k % 7 == 0)})


def damaged_files(path):
    """{what: (the file's bytes, the reason)} for a file of hostile_table() written with data_page_size=300, write_batch_size=50"""
    data, pages = _pages(path, 0)
    _, spages = _pages(path, 1)
    p = pages[1]["payload"]
    v = p + 4 + struct.unpack("<I", data[p:p + 4])[0]
    assert pages[0]["type"] == 2 and pages[1]["type"] == 0 and data[v] == 2 and spages[0]["type"] == 2

    def put(at, new):
        return data[:at] + new + data[at + len(new):]
    return {"a dictionary index past the entries": (put(v + 2, b"\xff"), R_DICT_INDEX),
            "a BYTE_ARRAY length past its page": (put(spages[0]["payload"] + 8, struct.pack("<I", 0x7FFFFFFF)), R_BYTE_ARRAY),
            "a levels length past its page": (put(p, struct.pack("<I", pages[1]["size"] - 3)), R_LEVELS_LENGTH),
            "a run count past num_values": (put(p + 4, b"\xfe\x7f"), R_RUN_COUNT)}      # an RLE run of 8191 levels


def test_the_damaged_files_of_the_gpu_test(exes):
    tbl = hostile_table()
    path = _check(exes, tbl, name="hostile.parquet", data_page_size=300, write_batch_size=50)
    for what, (data, reason) in damaged_files(path).items():
        _needs_host(exes, _patched(exes, data, 0, b""), tbl.schema, reason)
