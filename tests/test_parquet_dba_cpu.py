"""The DELTA_BYTE_ARRAY switch of the device Parquet decoder without a GPU: tests/cpp/parquet_dba_tests.cpp contains
the page walk with the switch (csrc/parquet_meta.hpp), the checks k_pq_delta_dba makes (csrc/device/qhip_dba.inc, the same text
with loops that stand for the lanes) and a model of k_pq_dba_fill that emulates the 64 lanes of a step. Files that pyarrow
writes are compared with `pq.read_table`, hand-made streams with a value-by-value model below. Built with g++ as a stand-alone
program (nothing of it is loaded into Python), plainly and with the address and undefined-behaviour sanitizers; every stream is
decoded from a heap block of exactly its size, so a hostile stream must end in its reason and never in a report. All
comparisons are exact.

The tables and stream lists below are also what tests/test_gpu_parquet_dba.py sends through the device."""
import decimal
import os
import random
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests.test_parquet_cpu import BOTH, FLAGS, ROOT, SAN, R_ENCODING, R_PAGE_V2, _code, _expect, _finish, _null_patterns, _pages, _patched, _uleb
from tests.test_parquet_encodings_cpu import R_DELTA_COUNT, R_DELTA_SHORT, _zigzag, delta_model

SOURCE = os.path.join(ROOT, "tests", "cpp", "parquet_dba_tests.cpp")
R_DBA_PREFIX, R_DBA_SUFFIX, R_DBA_WIDTH = 75, 76, 77        # behind QH_PQ_R_LZ4_END = 74 (csrc/device/qhip_parquet.inc)
DBA = "DELTA_BYTE_ARRAY"


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_dba_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("parquet_dba_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


def _decode(exes, which, path, schema, proj=None, level=1, encodings=1, dba=1):
    args = [exes[which], "decode", path, ",".join(_code(f.type) for f in schema), ",".join(map(str, proj)) if proj else "-", str(level), str(encodings), str(dba)]
    return _finish(subprocess.run(args, capture_output=True))


def _check(exes, tbl, which=BOTH, columns=None, level=1, encodings=1, name="t.parquet", **kw):
    path = str(exes["dir"] / name)
    kw.setdefault("compression", "NONE")
    kw.setdefault("use_dictionary", False)
    pq.write_table(tbl, path, **kw)
    schema = pq.read_schema(path)
    want = _expect(pq.read_table(path, columns=columns))
    proj = [schema.get_field_index(c) for c in columns] if columns else None
    for w in which:
        got = _decode(exes, w, path, schema, proj, level, encodings)
        assert got == want, (got[:3], want[:3])
    return path


def _reason(exes, path, schema, reasons, which=BOTH, level=1, encodings=1, dba=1):
    for w in which:
        got = _decode(exes, w, path, schema, None, level, encodings, dba)
        assert len(got) == 1 and got[0].startswith("NEEDS_HOST ") and int(got[0].split()[1]) in reasons, (got[:2], reasons)


# ---------------------------------------------------------------- the tables (also the GPU tests')
def null_patterns(n, page_rows=()):
    """tests.test_parquet_cpu's patterns, the first row of every page NULL, and all NULL but one"""
    out = dict(_null_patterns(n))
    first = np.zeros(n, dtype=bool)
    first[[r for r in page_rows if r < n] or [0]] = True
    one = np.ones(n, dtype=bool)
    one[n * 2 // 3] = False
    out["first of a page"] = first
    out["all but one"] = one
    return out


def key_table(n, nulls):
    """sorted keys with a shared head next to decimals of two widths, an Int64 and a Utf8 column of few values"""
    k = np.arange(n)
    dec = lambda p, s, v: pa.array([decimal.Decimal(int(x)).scaleb(-s, context=decimal.Context(prec=100)) for x in v], pa.decimal128(p, s), mask=nulls)     # noqa: E731
    return pa.table({"key": pa.array(["customer#%09d" % (v * 7) for v in k], pa.string(), mask=nulls),
                     "m15": dec(15, 2, (k * 1234567 % 99991 - 50000) * 100003),
                     "m38": dec(38, 4, [(-1) ** int(v) * (10 ** 30 + int(v) * 10 ** 17 + int(v) % 13) for v in k]),
                     "i64": pa.array(k * 5 - 100, pa.int64(), mask=nulls),
                     "tag": pa.array(["tag%d" % (v % 5) for v in k])})


KEY_ENC = {"key": DBA, "m15": DBA, "m38": DBA, "i64": "DELTA_BINARY_PACKED"}
KEY_WRITE = dict(use_dictionary=["tag"], column_encoding=KEY_ENC)


def shape_columns():
    """{name: values}: the shapes of values the fill has to get right"""
    a64, a65 = "p" * 64, "q" * 65
    big = "".join(chr(97 + k % 26) for k in range(200_000))
    return {
        "constant": ["the same value in every row"] * 1000,                                      # every row's bytes come from row 0, across 15 steps
        "empty and equal": ["", "", "abc", "abc", "abc", "", "abd", "abd", ""] * 30,
        "strict prefixes": ["abcdefgh", "abcdef", "abcd", "ab", "", "abcdefgh", "abcdefg"] * 40,
        "prefix 64 and 65": [a64 + "x", a64 + "y", a65 + "x", a65 + "y", a64, a65, a65 + "zz", a64 + "1"] * 20,
        "long": ["short", big, big[:150_000] + "X" * 50_000, "s", big[:150_000] + "Y", "", "tail"],  # the long-prefix path
        "growing": ["x" * k for k in range(200)] + ["x" * (200 - k) for k in range(200)],
        "random words": None,
    }


def shape_table(name, nulls=None):
    vals = shape_columns()[name]
    if vals is None:
        rng = random.Random(9)
        words = ["alpha", "alphabet", "alpine", "beta", "betray", "", "gamma", "gam"]
        vals = sorted(rng.choice(words) + rng.choice(words) + str(rng.randint(0, 30)) for _ in range(3000))
    return pa.table({"s": pa.array(vals, pa.string(), mask=None if nulls is None else nulls(len(vals)))})


# ---------------------------------------------------------------- hand-made DELTA_BYTE_ARRAY streams
def dbp(values, block=128, mpb=4, total=None):
    """a DELTA_BINARY_PACKED stream of exactly these (signed 32-bit) values: every miniblock at the width its deltas need,
    the miniblocks behind the last value not stored"""
    vpm = block // mpb
    out = bytearray(_uleb(block) + _uleb(mpb) + _uleb(len(values) if total is None else total) + _uleb(_zigzag(values[0] if values else 0)))
    deltas = [b - a for a, b in zip(values, values[1:])]
    for b0 in range(0, len(deltas), block):
        chunk = deltas[b0:b0 + block]
        lo = min(chunk)
        out += _uleb(_zigzag(lo))
        ws, body = [], bytearray()
        for m in range(mpb):
            part = [d - lo for d in chunk[m * vpm:(m + 1) * vpm]]
            if not part:
                ws.append(0)
                continue
            w = max(v.bit_length() for v in part)
            packed = 0
            for k, v in enumerate(part):
                packed |= v << (k * w)
            ws.append(w)
            body += packed.to_bytes(vpm * w // 8, "little")
        out += bytes(ws) + body
    return bytes(out)


def dba_stream(values, block=128, mpb=4):
    """the value stream of a DELTA_BYTE_ARRAY page for these bytes objects, with the longest prefixes"""
    prefixes, suffixes, prev = [], [], b""
    for v in values:
        p = 0
        while p < min(len(v), len(prev)) and v[p] == prev[p]:
            p += 1
        prefixes.append(p)
        suffixes.append(v[p:])
        prev = v
    return dbp(prefixes, block, mpb) + dbp([len(s) for s in suffixes], block, mpb) + b"".join(suffixes)


def dba_parts(prefixes, suffix_lengths, tail, total2=None):
    return dbp(prefixes) + dbp(suffix_lengths, total=total2) + tail


def dba_model(data, count):
    """a value-by-value reader of a good stream"""
    pre, end1 = delta_model(data, 4, count)
    suf, end2 = delta_model(data[end1:], 4, count)
    at, prev, out = end1 + end2, b"", []
    for p, s in zip(pre, suf):
        prev = prev[:p] + data[at:at + s]
        at += s
        out.append(prev)
    return out


def good_dba_streams():
    """{name: (bytes, width, count, values)}"""
    rng = random.Random(31)
    out = {}

    def add(name, values, width=0, **kw):
        out[name] = (dba_stream(values, **kw), width, len(values), values)
    for n in (0, 1, 2, 63, 64, 65, 66, 128, 129, 130, 257, 1000):
        add("keys n=%d" % n, [b"customer#%09d" % (k * 3) for k in range(n)])
    add("constant across 15 steps", [b"one value"] * 1000)
    add("empty, equal and strict prefixes", [b"", b"", b"abc", b"abc", b"ab", b"a", b"", b"abcd", b"abcd"] * 29)
    add("prefix 64 and 65", [b"p" * 64 + b"x", b"p" * 64 + b"y", b"p" * 65, b"p" * 65 + b"zz", b"p" * 64] * 30)
    big = bytes(97 + k % 26 for k in range(70_000))
    add("long prefixes between short ones", [b"s", big, big[:50_000] + b"X" * 900, b"t", big[:50_000], b"", b"tail"] + [b"k%d" % k for k in range(70)])
    add("growing and shrinking", [b"x" * k for k in range(150)] + [b"x" * (150 - k) for k in range(150)], block=256, mpb=8)
    words = [b"alpha", b"alphabet", b"alpine", b"beta", b"", b"gam"]
    add("random words", sorted(rng.choice(words) + rng.choice(words) + b"%d" % rng.randint(0, 30) for _ in range(700)), block=384, mpb=4)
    for width in (1, 5, 7, 16):
        add("decimals of %d bytes" % width, [rng.randint(-2 ** (8 * width - 1) // 1000, 2 ** (8 * width - 1) // 1000).to_bytes(width, "big", signed=True) for _ in range(300)], width)
    return out


def hostile_dba_streams():
    """{name: (bytes, width, count, reason)}: one per reason, each refused before the access it would make"""
    keys = [b"key%05d" % k for k in range(200)]
    pre = [0] + [next(p for p in range(9) if p == 8 or a[p] != b[p]) for a, b in zip(keys, keys[1:])]
    suf = [len(k) - p for k, p in zip(keys, pre)]
    tail = b"".join(k[p:] for k, p in zip(keys, pre))
    assert dba_model(dba_parts(pre, suf, tail), 200) == keys

    def with_(lst, at, v):
        return lst[:at] + [v] + lst[at + 1:]
    return {
        "a first prefix that is not 0": (dba_parts(with_(pre, 0, 1), suf, tail), 0, 200, R_DBA_PREFIX),
        "a prefix longer than the value before it": (dba_parts(with_(pre, 100, 9), suf, tail), 0, 200, R_DBA_PREFIX),
        "a prefix longer than the value before it, at the head of a step": (dba_parts(with_(pre, 65, 9), suf, tail), 0, 200, R_DBA_PREFIX),
        "a negative prefix": (dba_parts(with_(pre, 70, -1), suf, tail), 0, 200, R_DBA_PREFIX),
        "a negative suffix length": (dba_parts(pre, with_(suf, 130, -2), tail), 0, 200, R_DBA_SUFFIX),
        "a negative first suffix length": (dba_parts(pre, with_(suf, 0, -1), tail), 0, 200, R_DBA_SUFFIX),
        "suffix bytes past the page": (dba_parts(pre, with_(suf, 199, suf[199] + 1), tail), 0, 200, R_DBA_SUFFIX),
        "suffix bytes far past the page": (dba_parts(pre, with_(suf, 3, 2 ** 30), tail), 0, 200, R_DBA_SUFFIX),
        "a value above 2^31 - 1": (dba_parts(with_(with_(pre, 1, 8), 2, 8), with_(with_(suf, 1, 2 ** 31 - 9), 2, 2 ** 31 - 8), tail), 0, 200, R_DBA_SUFFIX),
        "a suffix count that is not the prefix count": (dba_parts(pre, suf[:199], tail), 0, 200, R_DELTA_COUNT),
        "a suffix count above the prefix count": (dba_parts(pre, suf, tail, total2=201), 0, 200, R_DELTA_COUNT),
        "a prefix count that is not the rows": (dba_parts(pre, suf, tail), 0, 199, R_DELTA_COUNT),
        "the end inside the suffix lengths": (dbp(pre) + dbp(suf)[:-3], 0, 200, R_DELTA_SHORT),
        "the end behind the prefix lengths": (dbp(pre), 0, 200, R_DELTA_SHORT),
        "a fixed-length value of the wrong width": (dba_parts(pre, with_(suf, 150, suf[150] + 1), tail + b"x"), 8, 200, R_DBA_WIDTH),
        "fixed-length values of another width": (dba_parts(pre, suf, tail), 7, 200, R_DBA_WIDTH),
    }


def cpu_model_dba(exe, workdir, streams):
    """[(bytes, width, count)] through the C++ loops: per stream the list of values or the reason"""
    path = str(workdir / "dba_streams.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(streams)))
        for s, width, count in streams:
            f.write(struct.pack("<III", len(s), width, count) + s)
    out = []
    for line in _finish(subprocess.run([exe, "dba", path], capture_output=True)):
        parts = line.split()
        out.append(int(parts[1]) if parts[0] == "REASON" else [b"" if v == "-" else bytes.fromhex(v) for v in parts[1:]])
    assert len(out) == len(streams)
    return out


# ---------------------------------------------------------------- what pyarrow writes
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_null_patterns_of_keys_and_decimals(exes, version):
    n = 1000
    for name, nulls in null_patterns(n, page_rows=range(0, n, 50)).items():      # (pages end with a write batch: every 50 rows here)
        tbl = key_table(n, nulls)
        path = _check(exes, tbl, encodings=2, data_page_version=version, data_page_size=256, write_batch_size=50, **KEY_WRITE)
        md = pq.ParquetFile(path).metadata.row_group(0)
        assert all(DBA in md.column(c).encodings for c in range(3)) and md.num_rows == n, name


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 130, 1000, 20_001])
def test_row_counts_with_pages_that_end_inside_steps(exes, n):
    for version in ("1.0", "2.0"):
        which = BOTH if n < 5000 else ("plain",)
        _check(exes, key_table(n, _null_patterns(n)["seventh"]), which=which, encodings=2, data_page_version=version, data_page_size=4096, **KEY_WRITE)
        _check(exes, key_table(n, None), which=which, encodings=2, data_page_version=version, data_page_size=4096, write_batch_size=50, **KEY_WRITE)


@pytest.mark.parametrize("shape", list(shape_columns()))
def test_shapes_of_values(exes, shape):
    for nulls in (None, lambda n: np.arange(n) % 7 == 3, lambda n: np.arange(n) % 64 == 0):
        tbl = shape_table(shape, nulls)
        for kw in (dict(data_page_version="1.0"), dict(data_page_version="2.0", data_page_size=4096)):
            path = _check(exes, tbl, encodings=2, column_encoding={"s": DBA}, **kw)
            assert DBA in pq.ParquetFile(path).metadata.row_group(0).column(0).encodings


def test_projections_with_and_without_the_column(exes):
    n = 1500
    tbl = key_table(n, _null_patterns(n)["random"])
    for columns in (["i64", "tag"], ["key"], ["m38"], ["tag", "m15", "key"]):
        _check(exes, tbl, columns=columns, encodings=2, data_page_version="2.0", data_page_size=4096, **KEY_WRITE)


def test_snappy_around_the_values(exes):
    n = 2000
    _check(exes, key_table(n, _null_patterns(n)["seventh"]), level=2, encodings=2, data_page_version="2.0", data_page_size=4096, compression="snappy", **KEY_WRITE)
    _check(exes, key_table(n, _null_patterns(n)["seventh"]), level=2, data_page_version="1.0", data_page_size=4096, compression="snappy",
           use_dictionary=["tag"], column_encoding={k: DBA for k in ("key", "m15", "m38")})       # (V1 pages: the switch and the level, no encoding set)


# ---------------------------------------------------------------- the switch in the page walk
def test_off_every_file_answers_as_before_and_on_the_page_is_planned(exes):
    n = 300
    for tbl, enc in ((pa.table({"s": pa.array(["v%d" % (v % 9) for v in range(n)])}), {"s": DBA}), (key_table(n, _null_patterns(n)["seventh"]).select(["m15"]), {"m15": DBA})):
        for version, reasons in (("1.0", {R_ENCODING}), ("2.0", {R_ENCODING, R_PAGE_V2})):
            path = str(exes["dir"] / "switch.parquet")
            pq.write_table(tbl, path, compression="NONE", use_dictionary=False, column_encoding=enc, data_page_version=version)
            schema = pq.read_schema(path)
            _reason(exes, path, schema, {R_ENCODING}, encodings=2, dba=0)
            _reason(exes, path, schema, reasons, encodings=1, dba=0)
            want = _expect(pq.read_table(path))
            for w in BOTH:
                assert _decode(exes, w, path, schema, None, 1, 2, 1) == want
            if version == "1.0":                                                 # a V1 page needs nothing but the switch
                assert _decode(exes, "plain", path, schema, None, 1, 1, 1) == want
            else:                                                                # a V2 page still needs encoding set 2
                _reason(exes, path, schema, {R_PAGE_V2}, encodings=1, dba=1)
    # with the switch on, a file without such pages answers as it did, and the older programs' calls answer through this one
    tbl = key_table(n, _null_patterns(n)["seventh"])
    path = str(exes["dir"] / "plain.parquet")
    pq.write_table(tbl, path, compression="NONE")
    schema = pq.read_schema(path)
    types = ",".join(_code(f.type) for f in schema)
    for w in BOTH:
        on = _decode(exes, w, path, schema, None, 1, 1, 1)
        assert on == _decode(exes, w, path, schema, None, 1, 1, 0) == _expect(tbl)
        assert _finish(subprocess.run([exes[w], "decode", path, types, "-"], capture_output=True)) == on
    # a DELTA_BYTE_ARRAY page of a type the switch does not cover still needs the host
    other = pa.table({"b": pa.array([b"ab", b"abc"], pa.binary())})
    path = str(exes["dir"] / "binary.parquet")
    pq.write_table(other, path, compression="NONE", use_dictionary=False, column_encoding={"b": DBA})
    _reason(exes, path, other.schema, {6})


# ---------------------------------------------------------------- raw streams
def test_the_model_reads_what_pyarrow_writes(exes):
    """the value streams of real pages, V1 behind their levels, through the raw entry's model"""
    vals = ["customer#%09d" % (k * 11) for k in range(500)] + ["", "a", "ab", "ab", "a"]
    tbl = pa.table([pa.array(vals)], schema=pa.schema([pa.field("s", pa.string(), nullable=False)]))
    path = str(exes["dir"] / "raw.parquet")
    pq.write_table(tbl, path, compression="NONE", use_dictionary=False, column_encoding={"s": DBA}, data_page_size=256, write_batch_size=70)
    data, pages = _pages(path, 0)
    assert len(pages) > 2
    streams, want, at = [], [], 0
    for pg in pages:
        n = pg["h"][5][1][0]
        assert pg["h"][5][2][0] == 7
        streams.append((data[pg["payload"]:pg["payload"] + pg["size"]], 0, n))
        want.append([v.encode() for v in vals[at:at + n]])
        at += n
    for w in BOTH:
        assert cpu_model_dba(exes[w], exes["dir"], streams) == want
    assert [dba_model(s, n) for s, _, n in streams] == want


def test_hand_made_streams_against_the_value_by_value_model(exes):
    good = good_dba_streams()
    for name, (s, width, count, values) in good.items():
        assert dba_model(s, count) == values, name
    for w in BOTH:
        got = cpu_model_dba(exes[w], exes["dir"], [v[:3] for v in good.values()])
        for (name, v), g in zip(good.items(), got):
            assert g == v[3], name


def test_hostile_streams_each_with_its_reason(exes):
    hostile = hostile_dba_streams()
    for w in BOTH:
        got = cpu_model_dba(exes[w], exes["dir"], [v[:3] for v in hostile.values()])
        for (name, v), g in zip(hostile.items(), got):
            assert g == v[3], (name, g if isinstance(g, int) else "decoded")


def test_truncation_and_random_damage_never_read_outside(exes):
    rng = random.Random(5)
    s, width, count, values = good_dba_streams()["random words"]
    got = cpu_model_dba(exes["san"], exes["dir"], [(s[:cut], 0, count) for cut in range(0, len(s), 7)])
    assert all(isinstance(g, int) for g in got)
    head = len(s) - sum(len(v) for v in values) + 40          # (both length streams and the first suffix bytes)
    flips = [(s[:k] + bytes([rng.choice([0, 0xFF, 0x80, s[k] ^ 1])]) + s[k + 1:], 0, count) for k in range(head)]
    cpu_model_dba(exes["san"], exes["dir"], flips)
    d, dw, dc, _ = good_dba_streams()["decimals of 7 bytes"]
    cpu_model_dba(exes["san"], exes["dir"], [(d[:k] + bytes([rng.choice([0, 0xFF, 0x80, d[k] ^ 1])]) + d[k + 1:], dw, dc) for k in range(0, len(d), 2)])
    # ... and whole files, damaged in place and cut off
    n = 400
    tbl = key_table(n, _null_patterns(n)["seventh"])
    path = _check(exes, tbl, name="hostile_dba.parquet", encodings=2, data_page_version="2.0", data_page_size=1024, **KEY_WRITE)
    data = open(path, "rb").read()
    footer = len(data) - 8 - struct.unpack("<I", data[-8:-4])[0]
    tail = data[footer:]
    for at in range(4, footer, 11):
        got = _decode(exes, "san", _patched(exes, data, at, bytes([rng.choice([0x00, 0xFF, 0x7F, 0x80, data[at] ^ 1])])), tbl.schema, encodings=2)
        assert got[0].startswith("NEEDS_HOST ") or got[0].startswith("ROWS "), (at, got[:1])
    cuts = set()
    for col in range(3):
        for pg in _pages(path, col)[1]:
            lev = pg["h"][8][5][0]
            cuts |= {pg["payload"] + lev, pg["payload"] + lev + 5, pg["payload"] + (pg["size"] + lev) // 2, pg["payload"] + pg["size"] - 1}
    for cut in sorted(c for c in cuts if 4 < c < footer):
        got = _decode(exes, "san", _patched(exes, data[:cut] + tail, 0, b""), tbl.schema, encodings=2)
        assert len(got) == 1 and got[0].startswith("NEEDS_HOST "), (cut, got[:2])
