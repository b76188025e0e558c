"""The lz4 switch of the device Parquet decoder without a GPU: tests/cpp/parquet_lz4_tests.cpp contains the page walk
with the switch (csrc/parquet_meta.hpp) and the LZ4 block decoder k_pq_unlz4 runs (csrc/device/qhip_lz4.inc, the same text with
loops that stand for the lanes). Raw blocks are compared with `pa.Codec("lz4_raw")`, hand-made ones with a byte-by-byte model
below, the pages of whole files with the codec over each page's payload. Built with g++ as a stand-alone program (nothing of it
is loaded into Python), plainly and with the address and undefined-behaviour sanitizers; every block is decoded from and into
heap blocks of exactly its sizes, so a hostile block must end in its reason and never in a report. All comparisons are exact.

The block lists below are also what tests/test_gpu_parquet_lz4.py sends through the device."""
import os
import random
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests.test_parquet_cpu import BOTH, FLAGS, LAYOUTS, R_CODEC, R_PAGE_V2, SAN, _code, _finish, _pages, _struct, _varint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "parquet_lz4_tests.cpp")
R_LZ4_SIZE, R_LZ4_FRAME, R_LZ4_CUT, R_LZ4_LITERAL, R_LZ4_OUTPUT, R_LZ4_OFFSET, R_LZ4_END = range(68, 75)

# what of the format a block used (QH_LZ4F_* of qhip_lz4.inc)
F_LITEXT, F_MATCHEXT, F_OVERLAP, F_FAR, F_LONG, F_LAST, F_EMPTY = range(7)
ALL_FORMS = set(range(7))
LZ4 = pa.Codec("lz4_raw")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_lz4_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("parquet_lz4_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


# ---------------------------------------------------------------- LZ4 blocks by hand, and a model that reads them byte by byte
def _ext(v):
    """the bytes that extend a nibble of 15 by v"""
    return b"\xff" * (v // 255) + bytes([v % 255])


def seq(lit=b"", offset=None, mlen=None):
    """one sequence: `lit` literals and, unless it is the last one, a match of mlen (4 or more) bytes at `offset`"""
    ln, mn = min(len(lit), 15), 0 if mlen is None else min(mlen - 4, 15)
    out = bytes([ln << 4 | mn]) + (_ext(len(lit) - 15) if ln == 15 else b"") + lit
    if mlen is not None:
        out += struct.pack("<H", offset) + (_ext(mlen - 19) if mn == 15 else b"")
    return out


def model(block):
    """what a block spells, read byte by byte with no limits but the block's own (IndexError where it is cut off)"""
    out, p = bytearray(), 0
    if not block:
        return b""
    while True:
        token = block[p]
        p += 1
        n = token >> 4
        if n == 15:
            while True:
                b = block[p]
                p += 1
                n += b
                if b != 255:
                    break
        assert p + n <= len(block)
        out += block[p:p + n]
        p += n
        if p == len(block):
            return bytes(out)
        offset = block[p] | block[p + 1] << 8
        p += 2
        m = (token & 15) + 4
        if m == 19:
            while True:
                b = block[p]
                p += 1
                m += b
                if b != 255:
                    break
        assert 0 < offset <= len(out)
        for _ in range(m):
            out.append(out[-offset])


def _text(n):
    words = ["wave", "front", "lane", "block", "offset", "literal", "match", "token", "parquet", "page"]
    rng = random.Random(3)
    s = " ".join(rng.choice(words) for _ in range(n // 5 + 2))
    return s.encode()[:n]


def good_blocks():
    """{name: (block, data)}: what the compressor makes of data that exercises the format"""
    rng = np.random.default_rng(7)
    data = {"the empty string": b"", "1 byte": b"q", "text": _text(20_000), "random bytes": rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
            "int64 prices": (rng.integers(0, 1000, 4000) * 25).astype(np.int64).tobytes()}
    for n in (5, 13, 64, 65, 1000, 70_000):
        data["a run of one byte, %d" % n] = b"z" * n
    for period in (2, 3, 63, 64, 65):
        unit = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
        data["period %d" % period] = (unit * (3000 // period + 1))[:3000]
    for n in (14, 15, 16, 18, 19, 20, 269, 270, 271, 273, 274, 275, 65_534, 65_535, 65_536, 65_537, 65_536 + 300):
        data["%d random bytes" % n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()                  # (one literal run of n)
        data["1 + %d equal bytes and a tail" % n] = b"k" * (n + 1) + b"tail of 12.."                     # (a match of n at offset 1)
        data["%d random bytes, twice" % n] = data["%d random bytes" % n] * 2 + b"tail of 12.."           # (a match of n at offset n)
    return {name: (LZ4.compress(d, asbytes=True), d) for name, d in data.items()}


def handmade_blocks():
    """{name: (block, what it spells)}: what the compressor does not emit"""
    rng = np.random.default_rng(9)
    far = rng.integers(0, 256, 65_535, dtype=np.uint8).tobytes()
    lits = {n: rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (15, 269, 270)}
    made = {
        "offset 65535": (seq(far, 65_535, 8) + seq(b"-end-"), far + far[:8] + b"-end-"),
        "offset 1, a match of 4": (seq(b"a", 1, 4) + seq(b"-end-"), b"aaaaa-end-"),
        "offset 1, a match of 1000": (seq(b"a", 1, 1000) + seq(b"-end-"), b"a" * 1001 + b"-end-"),
        "offset 3, a match of 200": (seq(b"abc", 3, 200) + seq(b"-end-"), (b"abc" * 68)[:203] + b"-end-"),
        "offset 70, a match of 300": (seq(far[:70], 70, 300) + seq(b"-end-"), (far[:70] * 6)[:370] + b"-end-"),
        "a match of exactly 19": (seq(b"abcd", 4, 19) + seq(b"-end-"), (b"abcd" * 6)[:23] + b"-end-"),
        "a match of exactly 19 + 255": (seq(b"abcd", 4, 274) + seq(b"-end-"), (b"abcd" * 70)[:278] + b"-end-"),
        "ends behind a match and an empty literal run": (seq(b"abcd", 4, 4) + seq(b""), b"abcdabcd"),          # (against the encoder's end rules)
        "a last match 1 byte before the end": (seq(b"abcd", 2, 6) + seq(b"!"), b"abcdcdcdcd!"),                # (the same)
        "two empty literal runs": (seq(b"ab", 2, 4) + seq(b"", 6, 5) + seq(b""), b"abababababa"),
    }
    for n, lit in lits.items():
        made["a literal run of exactly %d" % n] = (seq(lit, n, 4) + seq(b"-end-"), lit + lit[:4] + b"-end-")
        made["a last literal run of exactly %d" % n] = (seq(lit), lit)
    return made


def hostile_blocks():
    """{name: (block, declared size, reason)}"""
    text = _text(600)
    good = LZ4.compress(text, asbytes=True)
    return {
        "offset 0": (seq(b"abcd", 0, 4) + seq(b"-end-"), 13, R_LZ4_OFFSET),
        "an offset one beyond the bytes produced": (seq(b"abcd", 5, 4) + seq(b"-end-"), 13, R_LZ4_OFFSET),
        "a far offset one beyond the bytes produced": (seq(b"x" * 300, 301, 4) + seq(b"-end-"), 309, R_LZ4_OFFSET),
        "a literal run one byte past the input": (b"\x50abcd", 5, R_LZ4_LITERAL),
        "an extended literal run one byte past the input": (b"\xf0\x05" + b"a" * 19, 20, R_LZ4_LITERAL),
        "a literal run one byte past the output": (seq(b"abcde"), 4, R_LZ4_OUTPUT),
        "a match one byte past the output": (seq(b"abcd", 4, 8) + seq(b"-end-"), 11, R_LZ4_OUTPUT),
        "a long match one byte past the output": (seq(b"abcd", 4, 500) + seq(b"-end-"), 503, R_LZ4_OUTPUT),
        "a literal extension cut off": (b"\xf0\xff", 300, R_LZ4_CUT),
        "a literal extension cut off behind the token": (b"\x10a\x01\x00\xf0", 20, R_LZ4_CUT),
        "a match extension cut off": (b"\x4fabcd\x04\x00\xff", 300, R_LZ4_CUT),
        "an offset cut off": (b"\x40abcd\x04", 8, R_LZ4_CUT),
        "input left over": (good + b"\x00", len(text), R_LZ4_END),
        "a sequence left over": (good + seq(b"-end-"), len(text), R_LZ4_END),
        "output one byte short": (good, len(text) + 1, R_LZ4_END),
        "a block that ends behind a match": (seq(b"abcd", 4, 4), 8, R_LZ4_END),
        "a literal run of 255s that would overflow 32 bits": (b"\xf0" + b"\xff" * 16_843_010 + b"\x00", 1000, R_LZ4_LITERAL),
        "a match run of 255s that would overflow 32 bits": (b"\x4fabcd\x04\x00" + b"\xff" * 16_843_010 + b"\x00" + seq(b"-end-"), 1000, R_LZ4_OUTPUT),
        "a declared size of 255 x + 1": (seq(b"a", 1, 19 + 255) + seq(b"-end-"), 255 * len(seq(b"a", 1, 19 + 255) + seq(b"-end-")) + 1, R_LZ4_SIZE),
        "no input, a declared size of 1": (b"", 1, R_LZ4_SIZE),
    }


def run_blocks(exes, which, blocks, mode="streams"):
    """blocks: [(bytes, declared size)] -> per block (its output bytes or its reason, the forms it used as a set)"""
    path, out_path = str(exes["dir"] / "blocks.bin"), str(exes["dir"] / "blocks.out")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blocks)))
        for data, declared in blocks:
            f.write(struct.pack("<II", len(data), declared) + data)
    assert _finish(subprocess.run([exes[which], mode, path, out_path], capture_output=True)) == []
    raw = open(out_path, "rb").read()
    if mode == "frames":
        return raw
    at, res = 0, []
    for _ in blocks:
        reason, forms, n = struct.unpack_from("<III", raw, at)
        at += 12
        res.append((reason if reason else raw[at:at + n], {b for b in range(16) if forms >> b & 1}))
        at += n
    assert at == len(raw)
    return res


def cpu_model_results(exes, blocks, which="plain"):
    return [r for r, _ in run_blocks(exes, which, blocks)]


def test_compressed_blocks_decode_to_their_input(exes):
    good = good_blocks()
    assert good["the empty string"][0] == b"\x00"
    for name, (s, d) in good.items():
        assert model(s) == d, name
    seen = {}
    for which in BOTH:
        got = run_blocks(exes, which, [(s, len(d)) for s, d in good.values()])
        for (name, (_, data)), (g, forms) in zip(good.items(), got):
            assert g == data, (name, g if isinstance(g, int) else len(g))
            seen[name] = forms
    assert seen["the empty string"] == {F_LAST, F_EMPTY}
    assert seen["1 byte"] == {F_LAST}
    assert F_LITEXT in seen["15 random bytes"] and F_LITEXT not in seen["14 random bytes"]
    assert F_MATCHEXT in seen["1 + 274 equal bytes and a tail"] and F_OVERLAP in seen["a run of one byte, 1000"]
    assert {F_FAR, F_LONG} <= seen["65535 random bytes, twice"]
    # the empty input is accepted as well as the compressor's 00
    for which in BOTH:
        assert run_blocks(exes, which, [(b"", 0)]) == [(b"", {F_EMPTY})]


def test_handmade_blocks_cover_what_the_compressor_does_not_emit(exes):
    made = handmade_blocks()
    for name, (s, want) in made.items():
        assert model(s) == want, name                                               # (the block says what its name says)
    seen = set()
    for which in BOTH:
        got = run_blocks(exes, which, [(s, len(w)) for s, w in made.values()])
        for (name, (_, want)), (g, forms) in zip(made.items(), got):
            assert g == want, (name, g if isinstance(g, int) else len(g))
            seen |= forms
    assert {F_LITEXT, F_MATCHEXT, F_OVERLAP, F_FAR, F_LONG, F_LAST} <= seen


def test_the_two_sets_use_every_form_of_the_format(exes):
    both = [(s, len(d)) for s, d in list(good_blocks().values()) + list(handmade_blocks().values())]
    seen = set()
    for _, forms in run_blocks(exes, "plain", both):
        seen |= forms
    assert seen == ALL_FORMS


def test_hostile_blocks_are_refused_each_with_its_reason(exes):
    hostile = hostile_blocks()
    assert {r for _, _, r in hostile.values()} == {R_LZ4_SIZE, R_LZ4_CUT, R_LZ4_LITERAL, R_LZ4_OUTPUT, R_LZ4_OFFSET, R_LZ4_END}
    for name, (s, declared, reason) in hostile.items():
        if len(s) < 1 << 20 and reason != R_LZ4_SIZE and "short" not in name:      # the reference refuses them as well
            with pytest.raises(OSError):
                LZ4.decompress(s, decompressed_size=declared)
    for which in BOTH:
        got = run_blocks(exes, which, [(s, declared) for s, declared, _ in hostile.values()])
        for (name, (_, _, reason)), (g, _) in zip(hostile.items(), got):
            assert g == reason, (name, g if isinstance(g, int) else "decoded %d bytes" % len(g))
    # every truncation of good blocks: a reason, never a report, and never an output
    good = good_blocks()
    cuts = []
    for name in ("text", "period 3", "a run of one byte, 1000", "270 random bytes, twice"):
        s, data = good[name]
        cuts += [(s[:k], len(data)) for k in list(range(0, min(len(s), 120))) + [len(s) // 2, len(s) - 1]]
    for g, _ in run_blocks(exes, "san", cuts):
        assert isinstance(g, int) and R_LZ4_SIZE <= g <= R_LZ4_END, g


def damaged_blocks():
    """[(block, declared size)]: a few hundred blocks with random damage: byte flips and truncations"""
    rng = random.Random(13)
    good = good_blocks()
    cases = []
    for name in ("text", "int64 prices", "period 3", "period 65", "a run of one byte, 1000", "270 random bytes, twice", "1 + 274 equal bytes and a tail", "19 random bytes"):
        s, data = good[name]
        for k in range(60):
            b = bytearray(s)
            kind = rng.randrange(4)
            p = rng.randrange(len(b)) if rng.random() < 0.5 else rng.randrange(min(len(b), 24))
            if kind == 0:
                b[p] ^= 1 << rng.randrange(8)
            elif kind == 1:
                b[p] = rng.choice([0x00, 0xFF, 0xF0, 0x0F, b[p] ^ 0x80])
            elif kind == 2:
                del b[p:]
            else:
                del b[p:p + rng.choice([1, 2])]
            cases.append((bytes(b), len(data)))
    return cases


def test_random_damage_to_blocks_never_reads_or_writes_outside(exes):
    cases = damaged_blocks()
    assert len(cases) >= 400
    got = run_blocks(exes, "san", cases)
    assert [g for g, _ in run_blocks(exes, "plain", cases)] == [g for g, _ in got]
    for k, ((s, declared), (g, _)) in enumerate(zip(cases, got)):
        assert (isinstance(g, bytes) and len(g) == declared) or R_LZ4_SIZE <= g <= R_LZ4_END, k
        if isinstance(g, bytes):
            assert g == model(s), k
            try:
                want = LZ4.decompress(s, decompressed_size=declared, asbytes=True)
            except OSError:
                continue                                   # (the reference also holds a block to the encoder's end rules)
            assert g == want, k


# ---------------------------------------------------------------- Hadoop's framing of the legacy id
def frame(data, block=None):
    block = LZ4.compress(data, asbytes=True) if block is None else block
    return struct.pack(">II", len(data), len(block)) + block


def run_frames(exes, which, payloads):
    """payloads: [(bytes, declared size)] -> per payload (verdict, reason, [(where, bytes, uncompressed size)])"""
    raw, at, res = run_blocks(exes, which, payloads, "frames"), 0, []
    for _ in payloads:
        verdict, reason, n = struct.unpack_from("<III", raw, at)
        at += 12
        res.append((verdict, reason, [struct.unpack_from("<III", raw, at + 12 * k) for k in range(n)]))
        at += 12 * n
    assert at == len(raw)
    return res


def framed_payloads():
    """{name: (payload, the data it holds in its frames)}"""
    a, b, c = _text(3000), b"z" * 700, np.arange(500, dtype=np.int64).tobytes()
    return {"one frame": (frame(a), [a]), "three frames": (frame(a) + frame(b) + frame(c), [a, b, c]),
            "a frame of size 0 in the middle": (frame(a) + frame(b"") + frame(c), [a, b"", c]),
            "a frame of size 0 without a block": (frame(a) + frame(b"", b""), [a, b""])}


def test_hadoop_frames_that_tile_become_entries_and_others_one_bare_block(exes):
    payloads = framed_payloads()
    for which in BOTH:
        got = run_frames(exes, which, [(p, sum(map(len, parts))) for p, parts in payloads.values()])
        for (name, (p, parts)), (verdict, reason, frames) in zip(payloads.items(), got):
            assert (verdict, reason, len(frames)) == (1, 0, len(parts)), name
            at = 0
            for part, (where, csize, usize) in zip(parts, frames):
                assert where == at + 8 and usize == len(part) and (csize, usize) == struct.unpack_from(">II", p, at)[::-1], name
                at = where + csize
            assert at == len(p)
            # each frame's block, decoded as the kernel decodes it: from its own range into its own slice
            out = run_blocks(exes, which, [(p[w:w + cs], us) for w, cs, us in frames])
            assert [g for g, _ in out] == parts, name
    a = _text(3000)
    block = LZ4.compress(a, asbytes=True)
    n, m = len(a), len(block)
    off = {"the compressed size one more": struct.pack(">II", n, m + 1) + block, "the compressed size one less": struct.pack(">II", n, m - 1) + block,
           "the uncompressed size one more": struct.pack(">II", n + 1, m) + block, "the uncompressed size one less": struct.pack(">II", n - 1, m) + block,
           "a second frame one byte short": frame(a) + frame(a)[:-1], "7 bytes behind the frame": frame(a) + b"\x00" * 7,
           "a bare block": block, "nothing": b""}
    for which in BOTH:
        got = run_frames(exes, which, [(p, 2 * n if "second" in name else 0 if name == "nothing" else n) for name, p in off.items()])
        assert got == [(0, 0, [])] * len(off), dict(zip(off, got))
    # frames the host refuses before anything is reserved
    bad = {"no bytes for the output a frame declares": (frame(a) + struct.pack(">II", 5, 0), n + 5, R_LZ4_FRAME),
           "a frame above the 255 x bound": (frame(a) + struct.pack(">II", 511, 2) + b"\x1f\x00", n + 511, R_LZ4_SIZE)}
    for which in BOTH:
        got = run_frames(exes, which, [(p, d) for p, d, _ in bad.values()])
        assert [(v, r) for v, r, _ in got] == [(1, r) for _, _, r in bad.values()]


def test_a_bare_block_whose_first_bytes_tile_is_taken_for_frames_and_refused(exes):
    # 00 00 00 28 00 00 00 11 ... : as a bare block a token of 0 (no literals, a match at the very beginning: no block at all); as
    # Hadoop's framing one frame of 17 bytes that declares 40. Arithmetic says frames; the decoder says what the 17 bytes are.
    inner = seq(b"abcd", 9, 30) + seq(b"-end-+")
    payload = struct.pack(">II", 40, len(inner)) + inner
    for which in BOTH:
        (verdict, reason, frames), = run_frames(exes, which, [(payload, 40)])
        assert (verdict, reason, frames) == (1, 0, [(8, len(inner), 40)])
        (g, _), = run_blocks(exes, which, [(inner, 40)])
        assert g == R_LZ4_OFFSET                          # (the device's refusal is what sends such a page to the host)
        (g, _), = run_blocks(exes, which, [(payload, 40)])
        assert isinstance(g, int)                          # (nor is it a bare block)


# ---------------------------------------------------------------- whole files: the page walk with the lz4 switch
def run_pages(exes, which, path, schema, proj=None, level=1, encodings=1, codecs=1, gzip=0, lz4=1):
    """-> (the answer's first line, [(page, reason, where in the page, bytes)])"""
    out_path = str(exes["dir"] / "pages.out")
    args = [exes[which], "pages", path, ",".join(_code(f.type) for f in schema), ",".join(map(str, proj)) if proj else "-", str(level), str(encodings), str(codecs),
            str(gzip), str(lz4), out_path]
    lines = _finish(subprocess.run(args, capture_output=True))
    if lines[0].startswith("NEEDS_HOST"):
        return lines[0], []
    raw, at, res = open(out_path, "rb").read(), 0, []
    while at < len(raw):
        page, reason, where, n = struct.unpack_from("<IIII", raw, at)
        at += 16
        res.append((page, reason, where, raw[at:at + n]))
        at += n
    assert len(lines) == 1 and int(lines[0].split()[1]) == len(res)
    return lines[0], res


def lz4_table(n=3000):
    k = np.arange(n)
    rng = np.random.default_rng(11)
    return pa.table({"i": pa.array(k * 7 % 1000, pa.int64(), mask=k % 5 == 0), "f": pa.array(rng.random(n)), "s": pa.array(["str%d" % (v % 17) for v in k], mask=k % 7 == 0),
                     "p": pa.array(rng.integers(0, 1 << 40, n), pa.int64()), "b": pa.array(k % 3 == 0)})


def _skip(b, p, ty):
    """behind the value of compact-protocol type `ty` at b[p:]"""
    if ty in (1, 2):
        return p
    if ty == 3:
        return p + 1
    if ty in (4, 5, 6):
        return _varint(b, p)[1]
    if ty == 7:
        return p + 8
    if ty == 8:
        n, p = _varint(b, p)
        return p + n
    if ty == 12:
        return _struct(b, p)[1]
    assert ty in (9, 10), "thrift type %d" % ty
    n, et, p = b[p] >> 4, b[p] & 15, p + 1
    if n == 15:
        n, p = _varint(b, p)
    for _ in range(n):
        p = p + 1 if et in (1, 2) else _skip(b, p, et)
    return p


def _fields(b, p, want):
    """where the elements of list field `want` of the struct at b[p:] begin (structs)"""
    last = 0
    while True:
        h = b[p]
        p += 1
        assert h, "no field %d" % want
        ty, delta = h & 15, h >> 4
        if delta:
            fid = last + delta
        else:
            z, p = _varint(b, p)
            fid = (z >> 1) ^ -(z & 1)
        last = fid
        if fid == want:
            assert ty == 9 and b[p] & 15 == 12
            n, p = (b[p] >> 4, p + 1) if b[p] >> 4 != 15 else _varint(b, p + 1)
            out = []
            for _ in range(n):
                out.append(p)
                _, p = _struct(b, p)
            return out
        p = _skip(b, p, ty)


def codec_varints(data):
    """where the codec varint of every column chunk lies in the footer: FileMetaData.row_groups (4) -> RowGroup.columns (1) ->
    ColumnChunk.meta_data (3) -> ColumnMetaData.codec (4)"""
    n = struct.unpack_from("<I", data, len(data) - 8)[0]
    out = []
    for rg in _fields(data, len(data) - 8 - n, 4):
        for cc in _fields(data, rg, 1):
            value, at, length = _struct(data, cc)[0][3][4]
            assert length == 1
            out.append((at, value))
    return out


def legacy_id(data):
    """the file with every chunk's codec patched in place from LZ4_RAW (7) to the legacy LZ4 (5): varint 0x0e -> 0x0a"""
    b = bytearray(data)
    where = codec_varints(data)
    assert where and all(v == 7 and b[at] == 0x0E for at, v in where)
    for at, _ in where:
        b[at] = 0x0A
    return bytes(b)


def unpacked_by_the_codec(path, col):
    """what pa.Codec("lz4_raw") makes of the compressed values of every page of a column, over all row groups, in page order"""
    want = []
    for rg in range(pq.ParquetFile(path).metadata.num_row_groups):
        data, pages = _pages(path, col, rg)
        for pg in pages:
            lev = pg["h"][8][5][0] + pg["h"][8][6][0] if pg["type"] == 3 else 0          # (V2: the levels lie uncompressed in front)
            payload = data[pg["payload"] + lev:pg["payload"] + pg["size"]]
            if pg["type"] == 3 and (len(payload) == 0 or pg["h"][8].get(7, True) is False):
                continue                                   # (nothing to unpack, or values the writer left uncompressed)
            want.append(LZ4.decompress(payload, decompressed_size=pg["h"][2][0] - lev, asbytes=True))
    return want


@pytest.mark.parametrize("version", ("1.0", "2.0"))
@pytest.mark.parametrize("dictionary", (True, False))
@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_the_pages_of_lz4_files_unpack_to_what_the_codec_unpacks(exes, layout, dictionary, version):
    tbl = lz4_table()
    path, old = str(exes["dir"] / "l.parquet"), str(exes["dir"] / "l5.parquet")
    pq.write_table(tbl, path, compression="lz4", use_dictionary=dictionary, data_page_version=version, **LAYOUTS[layout])
    data = open(path, "rb").read()
    assert all(v == 7 for _, v in codec_varints(data)) and len(codec_varints(data)) == tbl.num_columns * pq.ParquetFile(path).metadata.num_row_groups
    with open(old, "wb") as f:
        f.write(legacy_id(data))
    assert all(v == 5 for _, v in codec_varints(open(old, "rb").read()))
    assert pq.read_table(old).equals(pq.read_table(path))                                        # (Arrow's reader falls back to the bare block)
    enc = 2 if version == "2.0" else 1
    for col in range(tbl.num_columns):
        want = unpacked_by_the_codec(path, col)
        for which in BOTH:
            for p in (path, old):                          # the legacy id: the bare-block fallback, the same pages
                head, got = run_pages(exes, which, p, tbl.schema, [col], encodings=enc)
                assert head == "PAGES %d 0 0 0" % len(want)
                assert all(r == 0 and w == 0 for _, r, w, _ in got)
                assert [g for _, _, _, g in got] == want, col
    for p in (path, old):                                  # every column: the slots do not overlap
        head, got = run_pages(exes, "plain", p, tbl.schema, encodings=2)
        assert head.startswith("PAGES ") and all(r == 0 for _, r, _, _ in got)


def test_the_five_switches_are_independent(exes):
    tbl = lz4_table(800)
    path = str(exes["dir"] / "sw.parquet")

    def answers(**kw):
        return [run_pages(exes, w, path, tbl.schema, **kw)[0] for w in BOTH]
    pq.write_table(tbl, path, compression="lz4")
    for level in (1, 2):                                   # the switch off is what it was, whatever the other four say
        for encodings in (1, 2):
            for codecs in (1, 2):
                for gzip in (0, 1):
                    assert answers(level=level, encodings=encodings, codecs=codecs, gzip=gzip, lz4=0) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2
    npages = sum(len(_pages(path, c)[1]) for c in range(tbl.num_columns))
    assert answers(lz4=1) == ["PAGES %d 0 0 0" % npages] * 2
    old = legacy_id(open(path, "rb").read())               # ... and so for the legacy id
    with open(path, "wb") as f:
        f.write(old)
    assert answers(level=2, encodings=2, codecs=2, gzip=1, lz4=0) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2
    assert answers(lz4=1) == ["PAGES %d 0 0 0" % npages] * 2
    # the other codecs stay with their switches
    pq.write_table(tbl, path, compression={"i": "snappy", "f": "lz4", "s": "zstd", "p": "NONE", "b": "gzip"})
    assert answers(level=1, codecs=2, gzip=1, lz4=1) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2
    assert answers(level=2, codecs=2, gzip=1, lz4=0) == ["NEEDS_HOST %d 0 1 -1" % R_CODEC] * 2
    assert answers(level=2, codecs=1, gzip=1, lz4=1) == ["NEEDS_HOST %d 0 2 -1" % R_CODEC] * 2
    assert answers(level=2, codecs=2, gzip=0, lz4=1) == ["NEEDS_HOST %d 0 4 -1" % R_CODEC] * 2
    head = answers(level=2, codecs=2, gzip=1, lz4=1)
    assert head[0] == head[1] and head[0].split()[0] == "PAGES" and all(int(v) >= 1 for v in head[0].split()[1:])
    head = answers(lz4=1, proj=[1, 3])                                                            # (an unprojected codec is not looked at)
    assert head[0] == head[1] and head[0].split()[2:] == ["0", "0", "0"] and int(head[0].split()[1]) >= 1
    if pa.Codec.is_available("brotli"):                    # brotli stays on the host
        pq.write_table(tbl, path, compression="brotli")
        assert answers(level=2, codecs=2, encodings=2, gzip=1, lz4=1) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2
    # data pages V2 need the encoding set as well
    pq.write_table(tbl, path, compression="lz4", data_page_version="2.0")
    assert all(a.startswith("NEEDS_HOST %d " % R_PAGE_V2) for a in answers(lz4=1))
    assert all(a.startswith("PAGES ") for a in answers(lz4=1, encodings=2))


def lz4_hostile_table():
    k = np.arange(3000)
    return pa.table({"i": pa.array(k * 7 % 1000, pa.int64(), mask=k % 5 == 0), "s": pa.array(["str%d" % (v % 17) for v in k], mask=k % 7 == 0)})


def damaged_lz4_file(path):
    """the file of lz4_hostile_table() (compression="lz4", use_dictionary=False, data_page_size=4096) with column 0's second page
    damaged in place: the offset of its first match set to 0, which only the decoder sees. -> (bytes, where: "0 0 1")"""
    data, pages = _pages(path, 0)
    assert len(pages) >= 3 and all(pg["type"] == 0 for pg in pages)
    at = pages[1]["payload"]
    lit = data[at] >> 4
    assert lit < 15
    return data[:at + 1 + lit] + b"\x00\x00" + data[at + 3 + lit:], "0 0 1"


def test_an_lz4_page_damaged_in_place(exes):
    tbl = lz4_hostile_table()
    path = str(exes["dir"] / "lz4_hostile.parquet")
    pq.write_table(tbl, path, compression="lz4", use_dictionary=False, data_page_size=4096)
    bad = str(exes["dir"] / "lz4_bad.parquet")
    data, where = damaged_lz4_file(path)
    with open(bad, "wb") as f:
        f.write(data)
    for w in BOTH:
        head, got = run_pages(exes, w, bad, tbl.schema)
        assert head.startswith("PAGES ") and [(p, r) for p, r, _, _ in got if r] == [(1, R_LZ4_OFFSET)]
    # random single-byte damage inside the compressed pages: a reason or pages, never a report
    good = open(path, "rb").read()
    pages = _pages(path, 0)[1]
    first, last = pages[0]["payload"], pages[-1]["payload"] + pages[-1]["size"]
    rng = random.Random(5)
    for _ in range(60):
        at = rng.randrange(first, last)
        with open(bad, "wb") as f:
            f.write(good[:at] + bytes([rng.choice([0x00, 0xFF, 0xF0, good[at] ^ 0x10])]) + good[at + 1:])
        head, got = run_pages(exes, "san", bad, tbl.schema)
        assert head.startswith("NEEDS_HOST ") or head.startswith("PAGES "), (at, head)
        assert all(r == 0 or R_LZ4_SIZE <= r <= R_LZ4_END for _, r, _, _ in got)


# ---------------------------------------------------------------- a whole file in Hadoop's framing
def fitted_block(data, period, size):
    """an LZ4 block of exactly `size` bytes that spells `data`, which repeats with `period`: the first period as literals, one
    match, the rest as literals — the match as long as the size allows, and the last 12 bytes literals, as liblz4, which Arrow's
    reader decodes the frames with, holds a block to the encoder's end rules. None where no match length gives the size."""
    for m in range(len(data) - period - 12, 3, -1):
        block = seq(data[:period], period, m) + seq(data[period + m:])
        if len(block) == size:
            return block
        if len(block) > size:
            return None
    return None


def hadoop_payload(data, period, frames=1):
    """`data` in Hadoop's framing, in as many bytes as it has itself: each of the `frames` frames is 8 bytes and a block fitted to
    be 8 bytes shorter than what it spells"""
    for shift in range(20):                                # (where a part finds no fit, the cuts move by a period)
        cut = [0] + [(len(data) * j // frames // period + shift) * period for j in range(1, frames)] + [len(data)]
        parts = [data[a:b] for a, b in zip(cut, cut[1:])]
        blocks = [fitted_block(p, period, len(p) - 8) for p in parts]
        if all(b is not None for b in blocks):
            out = b"".join(frame(p, b) for p, b in zip(parts, blocks))
            assert len(out) == len(data) and [model(b) for b in blocks] == parts and b"".join(parts) == data
            return out, frames
    raise AssertionError("no fit")


def hadoop_table(n=4000):
    k = np.arange(n)
    return pa.table({"v": pa.array(k % 4, pa.int64()), "w": pa.array(k % 3 * 1000, pa.int32())},
                    schema=pa.schema([pa.field("v", pa.int64(), nullable=False), pa.field("w", pa.int32(), nullable=False)]))


def hadoop_file(path):
    """hadoop_table() as a Hadoop writer would have left it under the legacy id: written uncompressed (required columns, PLAIN, data
    pages V1: a page's payload is its values), then every page's payload replaced in place by Hadoop frames of the same total size
    around LZ4 blocks of the same values, and the codec of every chunk patched from 0 to 5. -> (bytes, frames in all)"""
    pq.write_table(hadoop_table(), path, compression="NONE", use_dictionary=False, data_page_size=4096, write_statistics=False)
    b = bytearray(open(path, "rb").read())
    frames = 0
    for col, period, least in ((0, 32, 1), (1, 12, 2)):
        data, pages = _pages(path, col)
        assert len(pages) >= 2 and all(pg["type"] == 0 for pg in pages)
        for pg in pages:
            payload, k = hadoop_payload(data[pg["payload"]:pg["payload"] + pg["size"]], period, least)
            b[pg["payload"]:pg["payload"] + pg["size"]] = payload
            frames += k
    for at, value in codec_varints(bytes(b)):
        assert value == 0 and b[at] == 0
        b[at] = 0x0A
    return bytes(b), frames


def test_a_file_in_hadoop_framing_is_split_into_its_frames(exes):
    tbl = hadoop_table()
    path = str(exes["dir"] / "hadoop.parquet")
    data, frames = hadoop_file(path)
    plain = {c: [d[pg["payload"]:pg["payload"] + pg["size"]] for pg in pages] for c in (0, 1) for d, pages in [_pages(path, c)]}
    with open(path, "wb") as f:
        f.write(data)
    assert pq.read_table(path).equals(tbl)                 # (Arrow's reader takes the frames)
    assert frames > sum(map(len, plain.values()))          # (some pages have more than one)
    for which in BOTH:
        head, got = run_pages(exes, which, path, tbl.schema)
        assert head == "PAGES %d 0 0 0" % frames and all(r == 0 for _, r, _, _ in got)
        pages = {}
        for page, _, where, out in got:
            assert where == len(pages.get(page, b""))
            pages[page] = pages.get(page, b"") + out
        assert [pages[p] for p in sorted(pages)] == plain[0] + plain[1]
        assert run_pages(exes, which, path, tbl.schema, level=2, encodings=2, codecs=2, gzip=1, lz4=0)[0] == "NEEDS_HOST %d 0 0 -1" % R_CODEC
