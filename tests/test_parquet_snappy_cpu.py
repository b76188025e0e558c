"""Format level 2 of the device Parquet decoder without a GPU: tests/cpp/parquet_snappy_tests.cpp contains the
page walk at level 2 (csrc/parquet_meta.hpp) and the token code of k_pq_unsnap (csrc/device/qhip_snappy.inc), with loops that
stand for the lanes. Whole files are compared with `pyarrow.parquet.read_table`, raw streams with
`pyarrow.Codec("snappy").decompress`. Built with g++ as a stand-alone program (nothing of it is loaded into Python), plainly and
with the address and undefined-behaviour sanitizers; every stream is decoded from and into heap blocks of exactly its sizes, so a
hostile stream must end in its reason and never in a report.

The stream lists below are also what tests/test_gpu_parquet_snappy.py sends through the device."""
import os
import random
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests.test_parquet_cpu import (BOTH, FLAGS, LAYOUTS, R_CODEC, R_PAGE_V2, SAN, _code, _expect, _finish, _null_patterns, _pages, _typed_table, _uleb)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "parquet_snappy_tests.cpp")
R_SNAPPY_PREAMBLE, R_SNAPPY_SIZE, R_SNAPPY_INPUT, R_SNAPPY_OUTPUT, R_SNAPPY_OFFSET = range(29, 34)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_snappy_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("parquet_snappy_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


# ---------------------------------------------------------------- Snappy elements by hand
def lit(data, field=None):
    """a literal; field: the number of length bytes behind the tag (0: in the tag), None: the smallest that holds it"""
    n = len(data) - 1
    if field is None:
        field = 0 if n < 60 else 1 if n < 1 << 8 else 2 if n < 1 << 16 else 3 if n < 1 << 24 else 4
    if field == 0:
        assert n < 60
        return bytes([n << 2]) + data
    return bytes([(59 + field) << 2]) + n.to_bytes(field, "little") + data


def copy1(length, offset):
    assert 4 <= length <= 11 and 0 <= offset < 2048
    return bytes([1 | (length - 4) << 2 | (offset >> 8) << 5, offset & 255])


def copy2(length, offset):
    assert 1 <= length <= 64
    return bytes([2 | (length - 1) << 2]) + offset.to_bytes(2, "little")


def copy4(length, offset):
    assert 1 <= length <= 64
    return bytes([3 | (length - 1) << 2]) + offset.to_bytes(4, "little")


def stream(n, *elements):
    return _uleb(n) + b"".join(elements)


def model(elements_stream):
    """what a well-formed stream spells, by a byte-serial walk of the test's own: (declared size, output)"""
    b, p, n, shift = elements_stream, 0, 0, 0
    while True:
        n |= (b[p] & 0x7F) << shift
        shift += 7
        p += 1
        if not b[p - 1] & 0x80:
            break
    out = bytearray()
    while p < len(b):
        tag = b[p]
        kind, top = tag & 3, tag >> 2
        if kind == 0:
            extra = 0 if top < 60 else top - 59
            length = (top if top < 60 else int.from_bytes(b[p + 1:p + 1 + extra], "little")) + 1
            p += 1 + extra
            out += b[p:p + length]
            p += length
            continue
        if kind == 1:
            length, offset, p = 4 + (top & 7), (tag >> 5) << 8 | b[p + 1], p + 2
        else:
            width = 2 if kind == 2 else 4
            length, offset, p = top + 1, int.from_bytes(b[p + 1:p + 1 + width], "little"), p + 1 + width
        for _ in range(length):
            out.append(out[-offset])
    return n, bytes(out)


def good_streams():
    """{name: (stream, uncompressed size)}: the compressor's outputs and the legal elements it never emits"""
    codec = pa.Codec("snappy")
    rng = random.Random(7)
    rnd = lambda n: bytes(rng.getrandbits(8) for _ in range(n))     # noqa: E731
    text = ("".join("row %d of the lineitem table, shipped by %s|" % (k, ("AIR", "RAIL", "TRUCK")[k % 3]) for k in range(4000))).encode()
    out = {}
    inputs = {"empty": b"", "one byte": b"q", "64 KB - 1": text[:65535], "64 KB": text[:65536], "64 KB + 1": text[:65537], "constant": b"\x07" * 100_000,
              "random": rnd(50_000), "text": text}
    for p in (2, 3, 5, 63, 64, 65):
        inputs["period %d" % p] = (rnd(p) * (20_000 // p + 1))[:20_000]
    for name, data in inputs.items():
        out["compress: " + name] = (codec.compress(data, asbytes=True), len(data))
    # literals at the edges of the length fields, with every field size that holds them
    for length in (1, 60, 61, 256, 257, 65536):
        data = rnd(length)
        least = 0 if length <= 60 else 1 if length <= 256 else 2
        for field in range(least, 5):
            out["literal %d, %d length bytes" % (length, field)] = (stream(length + 3, lit(b"ab"), lit(data, field), lit(b"z")), length + 3)
    # copies: every offset form, lengths and offsets around the length and around the wavefront's width
    for length in (1, 4, 11, 12, 64):
        for offset in sorted({1, length - 1, length, length + 1, 63, 64, 65} - {0}):
            forms = [("2", copy2), ("4", copy4)] + ([("1", copy1)] if 4 <= length <= 11 else [])
            for form, make in forms:
                out["copy%s length %d offset %d" % (form, length, offset)] = (stream(100 + length + 2, lit(rnd(100)), make(length, offset), lit(b"zz")), 100 + length + 2)
    far = rnd(70_000)
    out["offsets above 65535"] = (stream(70_000 + 64 + 10 + 1, lit(far[:65536]), lit(far[65536:]), copy4(64, 66_000), copy4(10, 70_063), lit(b"!")), 70_075)
    # long chains of overlapping copies: each reads what the one before it stored
    out["chain of offset-1 copies"] = (stream(1 + 64 * 300, lit(b"x"), *[copy2(64, 1)] * 300), 1 + 64 * 300)
    out["chain of offset-2 copies"] = (stream(2 + 64 * 300, lit(b"ab"), *[copy2(64, 2)] * 300), 2 + 64 * 300)
    out["chain of offset-3 copies of 5"] = (stream(3 + 5 * 999, lit(b"abc"), *[copy1(5, 3)] * 999), 3 + 5 * 999)
    elements, produced = [lit(rnd(9))], 9
    for _ in range(3000):
        what = rng.random()
        if what < 0.25:
            n = rng.randint(1, 70)
            elements.append(lit(rnd(n)))
        else:
            n, offset = rng.randint(1, 64), rng.randint(1, min(produced, rng.choice([3, 64, 70, 3000])))
            elements.append(copy1(n, offset) if 4 <= n <= 11 and offset < 2048 and what < 0.5 else copy2(n, offset) if what < 0.9 else copy4(n, offset))
        produced += n
    out["a random walk of 3000 elements"] = (stream(produced, *elements), produced)
    return out


def hostile_streams():
    """{name: (stream, declared size, reason)}"""
    return {
        "no bytes at all": (b"", 0, R_SNAPPY_PREAMBLE),
        "preamble unterminated": (b"\x80\x80", 5, R_SNAPPY_PREAMBLE),
        "preamble of five continued bytes": (b"\x80\x80\x80\x80\x80\x00" + lit(b"a"), 1, R_SNAPPY_PREAMBLE),
        "preamble over 32 bits": (b"\xff\xff\xff\xff\x1f" + lit(b"a"), 100, R_SNAPPY_PREAMBLE),
        "preamble below the declared size": (stream(10, lit(b"0123456789")), 11, R_SNAPPY_PREAMBLE),
        "preamble above the declared size": (stream(10, lit(b"0123456789")), 9, R_SNAPPY_PREAMBLE),
        "declared size above 64/3 x compressed": (stream(10_000, lit(b"a"), copy2(64, 1)), 10_000, R_SNAPPY_SIZE),
        "declared size one above 64/3 x 6 bytes": (stream(129, lit(b"a"), copy1(11, 1)), 129, R_SNAPPY_SIZE),
        "declared size at 64/3 x 6 bytes, output short": (stream(128, lit(b"a"), copy1(11, 1)), 128, R_SNAPPY_INPUT),
        "literal tag without its length byte": (stream(20, lit(b"abc")) + bytes([60 << 2]), 20, R_SNAPPY_INPUT),
        "literal tag with 3 of 4 length bytes": (stream(20, lit(b"abc")) + bytes([63 << 2, 1, 0, 0]), 20, R_SNAPPY_INPUT),
        "copy1 tag without its offset byte": (stream(20, lit(b"abc")) + copy1(4, 1)[:1], 20, R_SNAPPY_INPUT),
        "copy2 tag with 1 of 2 offset bytes": (stream(20, lit(b"abc")) + copy2(4, 1)[:2], 20, R_SNAPPY_INPUT),
        "copy4 tag with 3 of 4 offset bytes": (stream(20, lit(b"abc")) + copy4(4, 1)[:4], 20, R_SNAPPY_INPUT),
        "literal past the input": (_uleb(20) + bytes([19 << 2]) + b"abc", 20, R_SNAPPY_INPUT),
        "literal of 2^32 bytes": (_uleb(20) + bytes([63 << 2]) + b"\xff\xff\xff\xff" + b"abc", 20, R_SNAPPY_INPUT),
        "literal past the output": (stream(3, lit(b"abcdef")), 3, R_SNAPPY_OUTPUT),
        "copy past the output": (stream(10, lit(b"abcd"), copy2(10, 2)), 10, R_SNAPPY_OUTPUT),
        "copy2 offset 0": (stream(20, lit(b"abcd"), copy2(8, 0), lit(b"12345678")), 20, R_SNAPPY_OFFSET),
        "copy1 offset 0": (stream(20, lit(b"abcd"), copy1(8, 0), lit(b"12345678")), 20, R_SNAPPY_OFFSET),
        "copy4 offset 0": (stream(20, lit(b"abcd"), copy4(8, 0), lit(b"12345678")), 20, R_SNAPPY_OFFSET),
        "offset one beyond the bytes produced": (stream(8, lit(b"abcd"), copy2(4, 5)), 8, R_SNAPPY_OFFSET),
        "offset 2^32 - 1": (stream(8, lit(b"abcd"), copy4(4, 0xFFFFFFFF)), 8, R_SNAPPY_OFFSET),
        "a copy as the first element": (stream(8, copy2(8, 1)), 8, R_SNAPPY_OFFSET),
        "input left after the output is full": (stream(4, lit(b"abcd"), lit(b"e")), 4, R_SNAPPY_INPUT),
        "input exhausted with output short": (stream(10, lit(b"abcd")), 10, R_SNAPPY_INPUT),
    }


def _run_streams(exes, which, streams):
    """streams: [(bytes, declared size)] -> per stream its output bytes or its reason (an int)"""
    path = str(exes["dir"] / "streams.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(streams)))
        for data, declared in streams:
            f.write(struct.pack("<II", len(data), declared) + data)
    lines = _finish(subprocess.run([exes[which], "streams", path], capture_output=True))
    assert len(lines) == len(streams)
    return [bytes.fromhex(ln[3:]) if ln.startswith("OK ") else int(ln.split()[1]) for ln in lines]


def cpu_model_results(exes, streams, which="plain"):
    return _run_streams(exes, which, streams)


def test_good_streams_equal_the_reference_decoder(exes):
    codec = pa.Codec("snappy")
    good = good_streams()
    want = [codec.decompress(s, decompressed_size=n, asbytes=True) for s, n in good.values()]
    for (name, (s, n)), w in zip(good.items(), want):
        if not name.startswith("compress"):
            assert model(s) == (n, w), name        # (the hand-made stream says what its name says)
    assert sum(name.startswith("literal 1,") for name in good) == 5 and "literal 65536, 4 length bytes" in good
    for which in BOTH:
        got = _run_streams(exes, which, list(good.values()))
        for name, g, w in zip(good, got, want):
            assert g == w, (name, g if isinstance(g, int) else len(g))


def test_hostile_streams_are_refused_each_with_its_reason(exes):
    codec = pa.Codec("snappy")
    hostile = hostile_streams()
    for name, (s, declared, _) in hostile.items():
        if name == "preamble below the declared size":
            continue                                # (a sound stream in a buffer larger than it needs: only the page header is wrong)
        with pytest.raises(Exception):              # the reference refuses every other one of them too
            codec.decompress(s, decompressed_size=declared, asbytes=True)
    for which in BOTH:
        got = _run_streams(exes, which, [(s, declared) for s, declared, _ in hostile.values()])
        for (name, (_, _, reason)), g in zip(hostile.items(), got):
            assert g == reason, (name, g if isinstance(g, int) else "decoded")
    # every truncation of good streams: a reason, never a report, and never the whole output
    good = good_streams()
    cuts = []
    for name in ("compress: text", "copy4 length 64 offset 65", "literal 257, 4 length bytes", "a random walk of 3000 elements"):
        s, n = good[name]
        cuts += [(s[:k], n) for k in list(range(0, min(len(s), 40))) + [len(s) // 2, len(s) - 1]]
    for g in _run_streams(exes, "san", cuts):
        assert g in (R_SNAPPY_PREAMBLE, R_SNAPPY_SIZE, R_SNAPPY_INPUT), g


def test_random_damage_to_streams_never_reads_or_writes_outside(exes):
    rng = random.Random(13)
    good = good_streams()
    cases = []
    for name in ("compress: text", "compress: period 3", "a random walk of 3000 elements", "copy2 length 12 offset 11"):
        s, n = good[name]
        for _ in range(60):
            at = rng.randrange(len(s)) if rng.random() < 0.5 else rng.randrange(min(len(s), 64))
            cases.append((s[:at] + bytes([rng.choice([0x00, 0xFF, 0xFE, 0xF0, 0x01, s[at] ^ 0x04])]) + s[at + 1:], n))
    for g in _run_streams(exes, "san", cases):
        assert isinstance(g, bytes) or g in range(R_SNAPPY_PREAMBLE, R_SNAPPY_OFFSET + 1)


# ---------------------------------------------------------------- whole files
def _decode(exes, which, path, schema, proj=None, level=2):
    args = [exes[which], "decode", path, ",".join(_code(f.type) for f in schema), ",".join(map(str, proj)) if proj else "-", str(level)]
    return _finish(subprocess.run(args, capture_output=True))


def _check(exes, tbl, which=BOTH, columns=None, name="t.parquet", **kw):
    path = str(exes["dir"] / name)
    pq.write_table(tbl, path, **kw)
    schema = pq.read_schema(path)
    want = _expect(pq.read_table(path, columns=columns))
    proj = [schema.get_field_index(c) for c in columns] if columns else None
    for w in which:
        got = _decode(exes, w, path, schema, proj)
        assert got == want, (got[:3], want[:3])
    return path


MIXED_CODECS = {"i32": "NONE", "i64": "snappy", "f64": "snappy", "d": "NONE", "m": "snappy", "b": "NONE", "s": "snappy"}


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_snappy_files_of_every_layout(exes, layout):
    n = 2000
    for name, nulls in _null_patterns(n).items():
        tbl = _typed_table(n, nulls)
        for dictionary in (True, False):
            path = _check(exes, tbl, compression="snappy", use_dictionary=dictionary, **LAYOUTS[layout])
        assert pq.ParquetFile(path).metadata.row_group(0).column(0).compression == "SNAPPY"
    tbl = _typed_table(n, _null_patterns(n)["seventh"])
    path = _check(exes, tbl, **LAYOUTS[layout])                                   # pyarrow's defaults
    assert pq.ParquetFile(path).metadata.row_group(0).column(1).compression == "SNAPPY"
    # a codec per column: the pages of the uncompressed chunks stay in the upload, the others go through the unpack area
    path = _check(exes, tbl, compression=MIXED_CODECS, **LAYOUTS[layout])
    meta = pq.ParquetFile(path).metadata.row_group(0)
    assert [meta.column(k).compression for k in range(7)] == ["UNCOMPRESSED", "SNAPPY", "SNAPPY", "UNCOMPRESSED", "SNAPPY", "UNCOMPRESSED", "SNAPPY"]
    _check(exes, tbl, columns=["s", "i32", "f64"], compression=MIXED_CODECS, **LAYOUTS[layout])
    _check(exes, tbl, columns=["d", "b"], compression=dict(MIXED_CODECS, i64="zstd"), **LAYOUTS[layout])     # (an unprojected codec is not looked at)


def test_pages_of_more_than_one_snappy_block_and_literal_only_pages(exes):
    rng = np.random.default_rng(3)
    tbl = pa.table({"k": pa.array(np.arange(10_000, dtype=np.int64) * 3), "r": pa.array(rng.random(10_000)), "c": pa.array(np.full(10_000, 7, dtype=np.int64)),
                    "p": pa.array(np.arange(10_000, dtype=np.int32) % 3)})
    path = _check(exes, tbl, compression="snappy", use_dictionary=False, data_page_size=1 << 20)
    data, pages = _pages(path, 0)
    assert len(pages) == 1 and pages[0]["h"][2][0] > 65536 and pages[0]["size"] < pages[0]["h"][2][0]     # one page, 80 KB unpacked
    big = "".join(chr(97 + k % 26) for k in range(200_000))
    for dictionary in (True, False):
        _check(exes, pa.table({"s": ["a", big, None, "b", big[:70000]]}), compression="snappy", use_dictionary=dictionary)


def test_what_still_needs_the_host_at_level_2(exes):
    n = 300
    k = np.arange(n)
    base = pa.table({"i": pa.array(k, pa.int64()), "f": pa.array(k / 3.0), "s": pa.array(["v%d" % (v % 9) for v in k]), "b": pa.array(k % 2 == 0)})

    def answer(level, **kw):
        path = str(exes["dir"] / "host.parquet")
        pq.write_table(base, path, **kw)
        return [_decode(exes, w, path, base.schema, level=level) for w in BOTH]

    for got in answer(1, compression="snappy"):
        assert len(got) == 1 and got[0].startswith("NEEDS_HOST %d " % R_CODEC)              # level 1 is what it was
    for got in answer(2, compression="snappy"):
        assert got[0] == "ROWS 300"
    for codec in ("zstd", "gzip", "lz4", "brotli"):
        if pa.Codec.is_available(codec):
            for got in answer(2, compression=codec):
                assert len(got) == 1 and got[0].startswith("NEEDS_HOST %d " % R_CODEC), codec
    for got in answer(2, compression={"i": "snappy", "f": "zstd", "s": "snappy", "b": "NONE"}):
        assert got == ["NEEDS_HOST %d 0 1 -1" % R_CODEC]
    for got in answer(2, compression="snappy", data_page_version="2.0"):
        assert len(got) == 1 and got[0].startswith("NEEDS_HOST %d " % R_PAGE_V2)
    for got in answer(2, compression="NONE", data_page_version="2.0"):
        assert len(got) == 1 and got[0].startswith("NEEDS_HOST %d " % R_PAGE_V2)


def snappy_hostile_table():
    k = np.arange(3000)
    return pa.table({"i": pa.array(k * 7 % 1000, pa.int64(), mask=k % 5 == 0), "s": pa.array(["str%d" % (v % 17) for v in k], mask=k % 7 == 0)})


def damaged_snappy_file(path):
    """the file of snappy_hostile_table() (compression="snappy", use_dictionary=False, data_page_size=4096) with the first tag of
    column 0's second page overwritten in place by a copy tag: a copy as the first element. -> (bytes, where: "0 0 1")"""
    data, pages = _pages(path, 0)
    assert len(pages) >= 3 and all(pg["type"] == 0 for pg in pages)
    pg = pages[1]
    assert pg["h"][2][0] > pg["size"]                     # (compressed)
    at = pg["payload"]
    while data[at] & 0x80:
        at += 1
    at += 1                                               # behind the preamble: the first tag
    assert data[at] & 3 == 0                              # (a literal, as every stream begins)
    return data[:at] + b"\xfe" + data[at + 1:], "0 0 1"


def test_a_snappy_page_damaged_in_place(exes):
    tbl = snappy_hostile_table()
    path = _check(exes, tbl, name="snappy_hostile.parquet", compression="snappy", use_dictionary=False, data_page_size=4096)
    data, where = damaged_snappy_file(path)
    bad = str(exes["dir"] / "snappy_bad.parquet")
    with open(bad, "wb") as f:
        f.write(data)
    for w in BOTH:
        assert _decode(exes, w, bad, tbl.schema) == ["NEEDS_HOST %d %s" % (R_SNAPPY_OFFSET, where)]
    # the sizes in a page header are claims: each alone and both together, at their largest and one off
    good = open(path, "rb").read()
    pg = _pages(path, 0)[1][1]
    (unc, at2, n2), (comp, at3, n3) = pg["h"][2], pg["h"][3]

    def zz(v, length):
        out = bytearray(_uleb(v << 1))
        assert len(out) <= length
        while len(out) < length:                          # (pad the varint to the field's length)
            out[-1] |= 0x80
            out.append(0)
        return bytes(out)
    for at, new in ((at2, zz(unc + 1, n2)), (at2, zz(unc - 1, n2)), (at2, zz((1 << (7 * n2 - 1)) - 1, n2)), (at3, zz(comp - 1, n3)), (at3, zz(1, n3)), (at3, zz(0, n3))):
        with open(bad, "wb") as f:
            f.write(good[:at] + new + good[at + len(new):])
        got = _decode(exes, "san", bad, tbl.schema)
        assert len(got) == 1 and got[0].startswith("NEEDS_HOST "), got[:2]
    # random single-byte damage inside the compressed pages: a reason or a table, never a report
    rng = random.Random(5)
    first, last = _pages(path, 0)[1][0]["payload"], pg["payload"] + pg["size"]
    for _ in range(60):
        at = rng.randrange(first, last)
        with open(bad, "wb") as f:
            f.write(good[:at] + bytes([rng.choice([0x00, 0xFF, 0xFE, good[at] ^ 0x10])]) + good[at + 1:])
        got = _decode(exes, "san", bad, tbl.schema)
        assert got[0].startswith("NEEDS_HOST ") or got[0].startswith("ROWS "), (at, got[:1])
