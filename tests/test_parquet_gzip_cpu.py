"""The gzip switch of the device Parquet decoder without a GPU: tests/cpp/parquet_gzip_tests.cpp contains the page
walk with the switch (csrc/parquet_meta.hpp) and the DEFLATE decoder k_pq_ungzip runs (csrc/device/qhip_inflate.inc, the same text
with loops that stand for the lanes). Raw members are compared with `zlib.decompress(member, 31)`, damaged ones with
`zlib.decompressobj(-15)` over the DEFLATE body (a model that checks no CRC, as the decoder checks none), the pages of whole
files with zlib over each page's payload. Built with g++ as a stand-alone program (nothing of it is loaded into Python), plainly
and with the address and undefined-behaviour sanitizers; every member is decoded from and into heap blocks of exactly its sizes,
so a hostile member must end in its reason and never in a report. All comparisons are exact.

The member lists below are also what tests/test_gpu_parquet_gzip.py sends through the device."""
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests.test_parquet_cpu import BOTH, FLAGS, LAYOUTS, R_CODEC, R_PAGE_V2, SAN, _code, _finish, _pages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "parquet_gzip_tests.cpp")
(R_GZIP_MEMBER, R_GZIP_SIZE, R_GZIP_BLOCK, R_GZIP_LENGTHS, R_GZIP_CODE, R_GZIP_SYMBOL, R_GZIP_DISTANCE, R_GZIP_OUTPUT, R_GZIP_INPUT,
 R_GZIP_TRAILER) = range(58, 68)

# what of the format a member used (QH_INFLF_* of qhip_inflate.inc)
F_STORED, F_FIXED, F_DYNAMIC, F_REP16, F_REP17, F_REP18, F_LEN258, F_DIST32K, F_LONG = range(9)
ALL_FORMS = list(range(9))
LIT_BITS, DIST_BITS = 10, 9                                # the widths of the decoder's primary tables

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_gzip_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("parquet_gzip_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


# ---------------------------------------------------------------- DEFLATE by hand (RFC 1951), gzip members (RFC 1952)
class Bits:
    """a forward bit writer, least significant bit first; a Huffman code goes in from its most significant bit"""

    def __init__(self):
        self.x, self.n = 0, 0

    def put(self, v, n):
        assert 0 <= v < 1 << n if n else v == 0
        self.x |= v << self.n
        self.n += n

    def code(self, code, length):
        for k in reversed(range(length)):
            self.put(code >> k & 1, 1)

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def bytes(self, data=b""):
        self.align()
        for b in data:
            self.put(b, 8)
        return self

    def done(self):
        return self.x.to_bytes((self.n + 7) // 8, "little")


def canon(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (a list, or {symbol: length})"""
    items = sorted(lens.items()) if isinstance(lens, dict) else list(enumerate(lens))
    count = [0] * 17
    for _, n in items:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in items:
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def balanced(used):
    """a complete code over these symbols (two at the least), no code longer than 5 bits"""
    used = sorted(used)
    if len(used) == 1:
        used = sorted(used + [0 if used[0] else 1])
    m = (len(used) - 1).bit_length()
    short = (1 << m) - len(used)
    return {s: (m - 1 if k < short else m) for k, s in enumerate(used)}


def rle_lengths(lens):
    """the code-length symbols [(symbol, repeat count or None)] of one list of lengths, repeats taken greedily — across the border
    between the literal/length lengths and the distance lengths where equal lengths straddle it"""
    seq, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            n = min(run, 138)
            seq.append((18, n) if n >= 11 else (17, n))
        elif v and i and lens[i - 1] == v and run >= 3:
            n = min(run, 6)
            seq.append((16, n))
        else:
            n = 1
            seq.append((v, None))
        i += n
    return seq


def put_tokens(w, tokens, lit, dist):
    """tokens: ("lit", byte), ("match", length, distance), ("end",), and for hostile streams ("sym", literal/length symbol),
    ("dsym", distance symbol), ("bits", value, count)"""
    for t in tokens:
        if t[0] == "lit" or t[0] == "sym":
            w.code(*lit[t[1]])
        elif t[0] == "end":
            w.code(*lit[256])
        elif t[0] == "dsym":
            w.code(*dist[t[1]])
        elif t[0] == "bits":
            w.put(t[1], t[2])
        else:
            _, length, distance = t
            i = max(k for k in range(29) if LBASE[k] <= length) if length < 258 else 28
            w.code(*lit[257 + i])
            w.put(length - LBASE[i], LEXT[i])
            j = max(k for k in range(30) if DBASE[k] <= distance)
            w.code(*dist[j])
            w.put(distance - DBASE[j], DEXT[j])


def spell(tokens, out=None):
    """what the tokens spell, byte by byte"""
    out = bytearray() if out is None else out
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "match":
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return out


def stored(w, data, final=False, nlen=None):
    w.put(int(final), 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
    return w.bytes(data)


def fixed(w, tokens, final=False):
    w.put(int(final), 1)
    w.put(1, 2)
    put_tokens(w, tokens, canon(FIXED_LIT), canon(FIXED_DIST))
    return w


def dynamic(w, tokens, lit_lens, dist_lens, final=False, seq=None, cl_lens=None, hclen=None, hlit=None, hdist=None):
    """a dynamic block. seq: the code-length symbols, rle_lengths() of both lists otherwise; cl_lens: the code-length code, a
    balanced one over the symbols of seq otherwise; hclen / hlit / hdist: the counts the header claims"""
    w.put(int(final), 1)
    w.put(2, 2)
    seq = rle_lengths(list(lit_lens) + list(dist_lens)) if seq is None else seq
    cl_lens = balanced({s for s, _ in seq}) if cl_lens is None else cl_lens
    w.put((len(lit_lens) if hlit is None else hlit) - 257, 5)
    w.put((len(dist_lens) if hdist is None else hdist) - 1, 5)
    count = max(4, 1 + max(CL_ORDER.index(s) for s, n in cl_lens.items() if n)) if hclen is None else hclen
    w.put(count - 4, 4)
    for s in CL_ORDER[:count]:
        w.put(cl_lens.get(s, 0), 3)
    codes = canon(cl_lens)
    for s, rep in seq:
        w.code(*codes[s])
        if s == 16:
            w.put(rep - 3, 2)
        elif s == 17:
            w.put(rep - 3, 3)
        elif s == 18:
            w.put(rep - 11, 7)
    if tokens is not None:
        put_tokens(w, tokens, canon(list(lit_lens)), canon(list(dist_lens)))
    return w


def member(body, data=None, isize=None, flg=0, extra=b"", cm=8, magic=b"\x1f\x8b", hcrc=True):
    """a gzip member around the DEFLATE stream `body`. data: what it spells (for CRC32 and ISIZE); isize: ISIZE alone (the CRC32,
    which nothing here verifies, is then 0); extra: the optional fields, behind which FHCRC is added when flg asks for it"""
    crc = zlib.crc32(data) if data is not None else 0
    isize = len(data) if isize is None else isize
    head = magic + bytes([cm, flg]) + bytes(4) + b"\x00\xff" + extra
    if flg & 2 and hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + body + struct.pack("<II", crc, isize & 0xFFFFFFFF)


def lens_of(pairs, n):
    out = [0] * n
    for s, v in pairs.items():
        out[s] = v
    return out


def handmade_members():
    """{name: (member, expected output)}: the legal forms zlib's compressor does not emit"""
    rng = random.Random(29)
    out = {}

    def one(name, w, tokens_list, **kw):
        data = bytearray()
        for t in tokens_list:
            if isinstance(t, (bytes, bytearray)):
                data += t
            else:
                spell(t, data)
        out[name] = (member(w.done(), bytes(data), **kw), bytes(data))

    # a dynamic block whose distance code is a single code of length 1
    toks = [("lit", 97), ("match", 3, 1), ("lit", 97), ("match", 258, 1), ("end",)]
    one("a single distance code of length 1", dynamic(Bits(), toks, lens_of({97: 1, 256: 2, 257: 3, 285: 3}, 286), [1], final=True), [toks])
    # ... and one with no distance code at all: literals only
    toks = [("lit", b) for b in b"no matches here"] + [("end",)]
    syms = sorted({t[1] for t in toks[:-1]} | {256})
    one("no distance code", dynamic(Bits(), toks, lens_of(balanced(syms), 257), [0], final=True), [toks])
    # HCLEN = 4: eight lengths of the code-length code, which end at symbol 6 (16 17 18 0 8 7 9 6)
    toks = [("lit", b) for b in bytes(range(63)) * 2] + [("end",)]
    w = dynamic(Bits(), toks, lens_of({**{s: 6 for s in range(63)}, 256: 6}, 257), [0], final=True)
    assert w.x >> 13 & 15 == 4
    one("HCLEN = 4", w, [toks])
    # repeats that cross from the literal/length lengths into the distance lengths: zeros (17), and a length (16)
    toks = [("lit", b) for b in b"abcd"] + [("match", 3, 4), ("end",)]
    lit, dist = lens_of({97: 2, 98: 2, 99: 3, 100: 3, 256: 3, 257: 3}, 260), [0, 0, 0, 1]
    seq = rle_lengths(lit + dist)
    assert seq[-2:] == [(17, 5), (1, None)]
    one("a repeat of zeros across the border", dynamic(Bits(), toks, lit, dist, final=True, seq=seq), [toks])
    toks = [("lit", 97), ("match", 3, 1), ("match", 4, 3), ("end",)]
    lit, dist = lens_of({97: 1, 256: 2, 257: 3, 258: 3}, 259), [3, 3, 3, 3, 2, 2]
    seq = rle_lengths(lit + dist)
    assert seq[-4:] == [(3, None), (16, 5), (2, None), (2, None)]
    one("a repeat of a length across the border", dynamic(Bits(), toks, lit, dist, final=True, seq=seq), [toks])
    # a stored block of length 0 as the final block, behind a block that ends inside a byte
    toks = [("lit", b) for b in b"hello, "] + [("match", 5, 7), ("end",)]
    one("an empty stored block as the final block", stored(fixed(Bits(), toks), b"", final=True), [toks])
    one("nothing but an empty stored block", stored(Bits(), b"", final=True), [])
    # codes of every length up to 15 bits, for literals and for distances
    toks = [("lit", b) for b in range(15)] * 2 + [("match", 3, DBASE[j]) for j in range(4)] + [("end",)]
    lit = lens_of({**{s: s + 1 for s in range(13)}, 13: 15, 14: 15, 256: 15, 257: 15}, 258)      # 1 .. 13, then four codes of 15 bits: 2^-13 left
    dist = [15, 15, 14, 13] + list(range(12, 0, -1))                                              # 16 codes: 1 .. 13, 14, 15, 15
    one("codes of 15 bits", dynamic(Bits(), toks, lit, dist, final=True), [toks])
    # the longest distance there is, 32768, which zlib's compressor never reaches, behind stored blocks; with the longest length
    head = bytes(rng.getrandbits(8) for _ in range(32768))
    toks = [("match", 258, 32768)] * 3 + [("match", 70, 32768), ("lit", 7), ("match", 258, 32768 - 600), ("end",)]
    one("a distance of 32768", fixed(stored(stored(Bits(), head[:30000]), head[30000:]), toks, final=True), [head, toks])
    # a member header with FEXTRA, FNAME and FHCRC (and FCOMMENT)
    toks = [("lit", b) for b in b"header"] + [("end",)]
    one("a header with FEXTRA, FNAME and FHCRC", fixed(Bits(), toks, final=True), [toks], flg=4 | 8 | 2, extra=struct.pack("<H", 5) + b"extra" + b"name.txt\x00")
    one("a header with every optional field", fixed(Bits(), toks, final=True), [toks], flg=1 | 2 | 4 | 8 | 16,
        extra=struct.pack("<H", 0) + b"n\x00" + b"a comment\x00")
    return out


def compressor_inputs():
    """{name: bytes}: what the compressor is given, with every setting of compressor_settings()"""
    rng = random.Random(7)
    rnd = lambda n: bytes(rng.getrandbits(8) for _ in range(n))     # noqa: E731
    text = ("row %d of the lineitem table, shipped by %s|" * 300 % sum(((k * k % 977, ("AIR", "RAIL", "TRUCK", "MAIL")[k * 7 % 4]) for k in range(300)), ())).encode()
    out = {"empty": b"", "one byte": b"q"}
    for n in (63, 64, 65):
        out["text %d" % n] = text[:n]
    out["a run of one byte"] = b"\x5a" * 100_000
    out["period 3"] = b"abc" * 7000
    out["period 70"] = bytes(range(70)) * 900
    out["text"] = text
    out["random bytes"] = rnd(5000)
    out["300 KB with matches at the window's far end"] = (rnd(32500) * 10)[:300_000]
    out["skewed bytes"] = bytes(rng.choices(range(18), [2.0 ** -k for k in range(18)], k=40_000))      # (codes longer than the primary tables are wide)
    out["int64 prices"] = np.random.default_rng(7).integers(100, 100_000, 6000).astype(np.int64).tobytes()
    return out


def compressor_settings():
    """{name: (level, memLevel, strategy, flushes)}"""
    s = {"level %d" % lv: (lv, 8, zlib.Z_DEFAULT_STRATEGY, False) for lv in (0, 1, 6, 9)}
    s.update({"Z_FIXED": (6, 8, zlib.Z_FIXED, False), "Z_HUFFMAN_ONLY": (6, 8, zlib.Z_HUFFMAN_ONLY, False), "Z_RLE": (6, 8, zlib.Z_RLE, False),
              "Z_FILTERED": (6, 8, zlib.Z_FILTERED, False), "memLevel 1": (6, 1, zlib.Z_DEFAULT_STRATEGY, False),
              "flushes": (6, 8, zlib.Z_DEFAULT_STRATEGY, True)})
    return s


def compress(data, level, mem, strategy, flushes):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    if not flushes:
        return co.compress(data) + co.flush()
    a, b = len(data) // 3, 2 * len(data) // 3              # (an empty stored block each, and what follows begins off a byte boundary no more)
    return co.compress(data[:a]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[a:b]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(data[b:]) + co.flush()


def compressed_members():
    out = {}
    for sname, setting in compressor_settings().items():
        for name, data in compressor_inputs().items():
            out["%s: %s" % (sname, name)] = (compress(data, *setting), data)
    return out


def good_members():
    """{name: (member, output)}: the compressor's outputs with every setting, then the hand-made members"""
    out = compressed_members()
    out.update(handmade_members())
    return out


def body_of(m):
    """the DEFLATE body of a member the decoder's header check accepts"""
    flg, at = m[3], 10
    if flg & 4:
        at += 2 + struct.unpack_from("<H", m, at)[0]
    for bit in (8, 16):
        if flg & bit:
            at = m.index(b"\x00", at) + 1
    if flg & 2:
        at += 2
    return at, m[at:len(m) - 8]


# ---------------------------------------------------------------- the test's own reader of a DEFLATE stream
def parse_deflate(body):
    """(the set of forms F_* the stream uses, its output): an independent walk over the blocks and symbols of a sound stream"""
    x, pos, forms, out = int.from_bytes(body, "little"), 0, set(), bytearray()

    def take(n):
        nonlocal pos
        v = x >> pos & ((1 << n) - 1)
        pos += n
        return v

    def decoder(lens):
        table = {(n, c): s for s, (c, n) in canon(lens).items()}

        def read():
            code = 0
            for n in range(1, 16):
                code = code << 1 | take(1)
                if (n, code) in table:
                    return table[(n, code)], n
            raise AssertionError("no code")
        return read
    while True:
        final, kind = take(1), take(2)
        forms.add(kind)
        if kind == 0:
            pos = (pos + 7) // 8 * 8
            n, inv = take(16), take(16)
            assert n ^ inv == 0xFFFF
            out += body[pos // 8:pos // 8 + n]
            pos += 8 * n
        else:
            if kind == 1:
                lit, dist = decoder(FIXED_LIT), decoder(FIXED_DIST)
            else:
                hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl[s] = take(3)
                read, lens = decoder(cl), []
                while len(lens) < hlit + hdist:
                    s, _ = read()
                    if s < 16:
                        lens.append(s)
                    else:
                        forms.add(F_REP16 + s - 16)
                        lens += [lens[-1]] * (3 + take(2)) if s == 16 else [0] * (3 + take(3)) if s == 17 else [0] * (11 + take(7))
                assert len(lens) == hlit + hdist
                lit, dist = decoder(lens[:hlit]), decoder(lens[hlit:])
            while True:
                s, n = lit()
                if n > LIT_BITS:
                    forms.add(F_LONG)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    length = LBASE[s - 257] + take(LEXT[s - 257])
                    d, n = dist()
                    if n > DIST_BITS:
                        forms.add(F_LONG)
                    distance = DBASE[d] + take(DEXT[d])
                    assert distance <= len(out)
                    if length == 258:
                        forms.add(F_LEN258)
                    if distance == 32768:
                        forms.add(F_DIST32K)
                    src = bytes(out[len(out) - distance:len(out) - distance + length])
                    out += (src * (length // len(src) + 1))[:length]
        if final:
            break
    assert (pos + 7) // 8 == len(body)
    return forms, bytes(out)


def hostile_members():
    """{name: (member, declared size, reason)}: one at the least per check of the decoder and of the member header"""
    hello = [("lit", b) for b in b"hello"]
    good_body = fixed(Bits(), hello + [("end",)], final=True).done()
    good = member(good_body, b"hello")
    lit_ok = lens_of({97: 1, 256: 2, 257: 2}, 258)

    def m(w, n):
        return (member(w.done() if isinstance(w, Bits) else w, isize=n), n)

    def dyn(n=4, tokens=(("lit", 97), ("end",)), lit=lit_ok, dist=(1, 1), **kw):
        return m(dynamic(Bits(), list(tokens) if tokens is not None else None, lit, list(dist), final=True, **kw), n)
    ten = b"0123456789"
    h = {
        # ---- the member header (the host's check)
        "no bytes at all": (b"", 0, R_GZIP_MEMBER),
        "wrong magic": (member(good_body, b"hello", magic=b"\x1f\x8c"), 5, R_GZIP_MEMBER),
        "a zlib wrapper": (zlib.compress(b"hello" * 10), 50, R_GZIP_MEMBER),
        "a raw DEFLATE stream": (zlib.compress(b"hello" * 10)[2:-4] + bytes(12), 50, R_GZIP_MEMBER),
        "a method other than 8": (member(good_body, b"hello", cm=7), 5, R_GZIP_MEMBER),
        "a reserved flag": (member(good_body, b"hello", flg=0x20), 5, R_GZIP_MEMBER),
        "FEXTRA past the member": (member(good_body, b"hello", flg=4, extra=struct.pack("<H", 500)), 5, R_GZIP_MEMBER),
        "FEXTRA cut off in its length": (good[:3] + b"\x04" + good[4:10] + b"\x01", 5, R_GZIP_MEMBER),
        "FNAME without its end": (member(good_body.replace(b"\x00", b"\x01"), isize=5, flg=8, extra=b"name")[:-8] + b"\x01" * 8, 0x01010101, R_GZIP_MEMBER),
        "FCOMMENT without its end": (good[:3] + b"\x10" + b"\x01" * 30, 0x01010101, R_GZIP_MEMBER),
        "FHCRC cut off": (good[:3] + b"\x02" + good[4:10] + b"\x01", 5, R_GZIP_MEMBER),
        "a header cut off": (good[:9], 5, R_GZIP_MEMBER),
        "no body": (good[:10] + good[-8:], 5, R_GZIP_MEMBER),
        "a trailer one byte short": (good[:-1], 5, R_GZIP_SIZE),
        "ISIZE above the declared size": (good, 4, R_GZIP_SIZE),
        "ISIZE below the declared size": (good, 6, R_GZIP_SIZE),
        "a claim far above what the body can produce": (member(good_body, isize=70_000), 70_000, R_GZIP_SIZE),
        "a claim of 1033 bytes per body byte": (member(b"\x03\x00", isize=2 * 1032 + 1), 2 * 1032 + 1, R_GZIP_SIZE),
        # ---- block headers
        "a block of type 3": m(_bits([(1, 1), (3, 2), (0, 13)]), 0) + (R_GZIP_BLOCK,),
        "a stored block whose NLEN is not LEN's complement": m(stored(Bits(), ten, final=True, nlen=10), 10) + (R_GZIP_BLOCK,),
        # ---- the code lengths of a dynamic block
        "HLIT of 287": dyn(lit=lit_ok, hlit=287) + (R_GZIP_LENGTHS,),
        "HLIT of 288": dyn(lit=lit_ok, hlit=288) + (R_GZIP_LENGTHS,),
        "HDIST of 31": dyn(hdist=31) + (R_GZIP_LENGTHS,),
        "HDIST of 32": dyn(hdist=32) + (R_GZIP_LENGTHS,),
        "a repeat with no previous length": dyn(seq=[(16, 3)] + rle_lengths(lit_ok[3:] + [1, 1]), cl_lens=balanced({16, 18, 0, 1, 2})) + (R_GZIP_LENGTHS,),
        "a repeat past the count": dyn(seq=rle_lengths(lit_ok + [1])[:-1] + [(1, None), (16, 3)], cl_lens=balanced({16, 18, 0, 1, 2}), tokens=None) + (R_GZIP_LENGTHS,),
        "a repeat of zeros past the count": dyn(seq=rle_lengths(lit_ok + [1, 1]) + [(18, 138)], lit=lit_ok, tokens=None, hlit=258 + 1) + (R_GZIP_LENGTHS,),
        "an over-subscribed code-length code": dyn(cl_lens={0: 1, 1: 1, 2: 2, 18: 2}) + (R_GZIP_LENGTHS,),
        "an incomplete code-length code": dyn(cl_lens={0: 2, 1: 2, 2: 2, 18: 3}, tokens=None) + (R_GZIP_LENGTHS,),
        "a code-length code of a single code": dyn(cl_lens={0: 1}, seq=[(0, None)] * 260, tokens=None) + (R_GZIP_LENGTHS,),
        # ---- the two codes
        "an over-subscribed literal/length code": dyn(lit=lens_of({97: 1, 98: 1, 256: 2}, 257)) + (R_GZIP_CODE,),
        "an incomplete literal/length code": dyn(lit=lens_of({97: 2, 256: 2, 257: 2}, 258)) + (R_GZIP_CODE,),
        "a literal/length code of a single code": dyn(1, tokens=(("end",),), lit=lens_of({256: 1}, 257)) + (R_GZIP_CODE,),
        "an over-subscribed distance code": dyn(dist=(1, 1, 1)) + (R_GZIP_CODE,),
        "an incomplete distance code of two codes": dyn(dist=(2, 2)) + (R_GZIP_CODE,),
        "a single distance code of length 2": dyn(dist=(0, 2)) + (R_GZIP_CODE,),
        "no end-of-block code": dyn(lit=lens_of({97: 1, 98: 1}, 257), tokens=(("lit", 97),)) + (R_GZIP_CODE,),
        "the fewest code-length lengths there are, which reach no length but 0": dyn(seq=[(18, 138), (18, 122)], cl_lens={18: 1, 0: 1}, tokens=None, hclen=4) + (R_GZIP_CODE,),
        # ---- symbols
        "literal/length symbol 286": m(fixed(Bits(), hello + [("sym", 286), ("bits", 0, 5), ("end",)], final=True), 8) + (R_GZIP_SYMBOL,),
        "literal/length symbol 287": m(fixed(Bits(), hello + [("sym", 287), ("bits", 0, 5), ("end",)], final=True), 8) + (R_GZIP_SYMBOL,),
        "distance symbol 30": m(fixed(Bits(), hello + [("sym", 257), ("dsym", 30), ("end",)], final=True), 8) + (R_GZIP_SYMBOL,),
        "distance symbol 31": m(fixed(Bits(), hello + [("sym", 257), ("dsym", 31), ("end",)], final=True), 8) + (R_GZIP_SYMBOL,),
        "the bit that is no code of a single distance code": dyn(4, tokens=(("lit", 97), ("sym", 257), ("bits", 1, 1), ("end",)), dist=(1,)) + (R_GZIP_SYMBOL,),
        "a match where there is no distance code": dyn(4, tokens=(("lit", 97), ("sym", 257), ("bits", 0, 1), ("end",)), dist=(0,)) + (R_GZIP_SYMBOL,),
        # ---- distances (a distance of 0 cannot be written: the smallest base is 1; the decoder's check of it is never reached)
        "a distance one beyond the bytes produced": m(fixed(Bits(), hello + [("sym", 257), ("dsym", 4), ("bits", 1, 1), ("end",)], final=True), 8) + (R_GZIP_DISTANCE,),
        "a match as the member's first bytes": m(fixed(Bits(), [("sym", 257), ("dsym", 0), ("end",)], final=True), 3) + (R_GZIP_DISTANCE,),
        "a distance of 32768 behind 32767 bytes": m(fixed(stored(Bits(), bytes(32767)), [("sym", 285), ("dsym", 29), ("bits", 8191, 13), ("end",)], final=True), 33025) + (R_GZIP_DISTANCE,),
        # ---- output
        "a literal past the declared size": m(fixed(Bits(), hello + [("end",)], final=True), 4) + (R_GZIP_OUTPUT,),
        "a match past the declared size": m(fixed(Bits(), hello + [("match", 10, 5), ("end",)], final=True), 14) + (R_GZIP_OUTPUT,),
        "a stored block past the declared size": m(stored(Bits(), ten, final=True), 9) + (R_GZIP_OUTPUT,),
        "a final block that ends with output missing": m(fixed(Bits(), hello + [("end",)], final=True), 6) + (R_GZIP_OUTPUT,),
        "64 literals pending at the declared size": m(fixed(Bits(), [("lit", 1)] * 65 + [("end",)], final=True), 64) + (R_GZIP_OUTPUT,),
        # ---- input
        "the input ends inside a block header": m(b"\x05", 1) + (R_GZIP_INPUT,),
        "the input ends inside the code lengths": m(dynamic(Bits(), None, lit_ok, [1, 1], final=True).done()[:6], 4) + (R_GZIP_INPUT,),
        "the input ends inside a literal": m(fixed(Bits(), hello, final=True).done()[:3], 2) + (R_GZIP_INPUT,),
        "the input ends inside a distance's extra bits": m(fixed(Bits(), hello + [("sym", 257), ("dsym", 8)], final=True).done(), 8) + (R_GZIP_INPUT,),
        "no end of block before the trailer": m(fixed(Bits(), hello, final=True).done(), 5) + (R_GZIP_INPUT,),
        "no final block": m(fixed(Bits(), hello + [("end",)]), 5) + (R_GZIP_INPUT,),
        "a stored block's lengths cut off": m(_bits([(1, 1), (0, 2), (0, 5), (10, 16)]), 10) + (R_GZIP_INPUT,),
        "a stored block past the input": m(stored(Bits(), ten, final=True).done()[:-1], 10) + (R_GZIP_INPUT,),
        # ---- behind the final block
        "a byte between the final block and the trailer": m(good_body + b"\x00", 5) + (R_GZIP_TRAILER,),
        "a second member": (good + good, 5, R_GZIP_TRAILER),
        "a second member behind an empty first one": (member(b"\x03\x00", b"") + member(b"\x03\x00", b""), 0, R_GZIP_TRAILER),
    }
    return h


def _bits(fields):
    w = Bits()
    for v, n in fields:
        w.put(v, n)
    return w


def run_members(exes, which, members):
    """members: [(bytes, declared size)] -> per member (its output bytes or its reason, the forms it used as a set)"""
    path, out_path = str(exes["dir"] / "members.bin"), str(exes["dir"] / "members.out")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(members)))
        for data, declared in members:
            f.write(struct.pack("<II", len(data), declared) + data)
    assert _finish(subprocess.run([exes[which], "streams", path, out_path], capture_output=True)) == []
    raw, at, res = open(out_path, "rb").read(), 0, []
    for _ in members:
        reason, forms, n = struct.unpack_from("<III", raw, at)
        at += 12
        res.append((reason if reason else raw[at:at + n], {b for b in range(16) if forms >> b & 1}))
        at += n
    assert at == len(raw)
    return res


def cpu_model_results(exes, members, which="plain"):
    return [r for r, _ in run_members(exes, which, members)]


def test_compressed_members_equal_zlib_and_cover_the_format(exes):
    good = compressed_members()
    parsed = {}
    for name, (s, data) in good.items():
        assert zlib.decompress(s, 31) == data, name
        forms, out = parse_deflate(body_of(s)[1])
        assert out == data, name
        parsed[name] = forms
    # a different build of the compressor must not quietly test less: every form but the distance it never reaches
    seen = set().union(*parsed.values())
    assert sorted(seen) == [f for f in ALL_FORMS if f != F_DIST32K]
    assert all(parsed["level 0: " + k] == {F_STORED} for k in compressor_inputs())
    assert all(parsed["Z_FIXED: " + k] <= {F_FIXED, F_STORED, F_LEN258} for k in compressor_inputs())
    for setting in ("level 1", "level 6", "level 9"):
        assert parsed[setting + ": random bytes"] == {F_STORED}                # what does not compress comes out as stored blocks
    assert {F_STORED, F_DYNAMIC} <= parsed["flushes: text"]                     # (the empty stored block of a flush)
    for which in BOTH:
        got = run_members(exes, which, [(s, len(d)) for s, d in good.values()])
        for (name, (_, data)), (g, forms) in zip(good.items(), got):
            assert g == data, (name, g if isinstance(g, int) else len(g))
            assert forms == parsed[name], name                                   # the decoder took the path the stream spells


def test_handmade_members_cover_what_the_compressor_does_not_emit(exes):
    made = handmade_members()
    seen = set()
    for name, (s, want) in made.items():
        assert zlib.decompress(s, 31) == want, name                              # (the member says what its name says)
        forms, out = parse_deflate(body_of(s)[1])
        assert out == want, name
        seen |= forms
    assert {F_DIST32K, F_LONG, F_REP16, F_REP17, F_REP18, F_LEN258, F_STORED, F_FIXED, F_DYNAMIC} <= seen
    for which in BOTH:
        got = run_members(exes, which, [(s, len(w)) for s, w in made.values()])
        for (name, (_, want)), (g, _) in zip(made.items(), got):
            assert g == want, (name, g if isinstance(g, int) else len(g))


def test_hostile_members_are_refused_each_with_its_reason(exes):
    hostile = hostile_members()
    assert {r for _, _, r in hostile.values()} == set(range(R_GZIP_MEMBER, R_GZIP_TRAILER + 1))
    for name, (s, declared, reason) in hostile.items():
        # what the decoder refuses behind the header, the reference refuses as well, or it yields another size
        if reason > R_GZIP_SIZE and reason != R_GZIP_TRAILER:
            d = zlib.decompressobj(-15)
            try:
                out = d.decompress(body_of(s)[1])
                assert not d.eof or len(out) != declared, name
            except zlib.error:
                pass
    for which in BOTH:
        got = run_members(exes, which, [(s, declared) for s, declared, _ in hostile.values()])
        for (name, (_, _, reason)), (g, _) in zip(hostile.items(), got):
            assert g == reason, (name, g if isinstance(g, int) else "decoded %d bytes" % len(g))
    # every truncation of good members' bodies, the trailer kept: a reason, never a report, and never an output
    good = good_members()
    cuts = []
    for name in ("level 6: text", "memLevel 1: int64 prices", "Z_FIXED: text 65", "codes of 15 bits", "a repeat of a length across the border"):
        s, data = good[name]
        at, body = body_of(s)
        cuts += [(s[:at] + body[:k] + s[-8:], len(data)) for k in list(range(1, min(len(body), 80))) + [len(body) // 2, len(body) - 1]]
    for g, _ in run_members(exes, "san", cuts):
        assert isinstance(g, int) and R_GZIP_MEMBER <= g <= R_GZIP_TRAILER, g


def damaged_members():
    """[(member, declared size)]: a few thousand members with random damage to the DEFLATE body (the header and the trailer kept,
    so that the decoder and not the header check meets it) or to the member as a whole: bit flips, truncation, inserted bytes"""
    rng = random.Random(13)
    good = good_members()
    cases = []
    names = ("level 6: text", "level 9: int64 prices", "level 1: period 70", "memLevel 1: text", "Z_FIXED: text", "Z_HUFFMAN_ONLY: random bytes", "Z_RLE: a run of one byte",
             "flushes: text", "level 6: text 65", "level 0: text 64", "codes of 15 bits", "a repeat of zeros across the border", "a single distance code of length 1",
             "a header with FEXTRA, FNAME and FHCRC")
    for name in names:
        s, data = good[name]
        at, body = body_of(s)
        for k in range(220):
            whole = k % 11 == 10
            b = bytearray(s if whole else body)
            kind = rng.randrange(4)
            # (the first bytes hold the block header and the code lengths: half the damage goes there)
            p = rng.randrange(len(b)) if rng.random() < 0.5 else rng.randrange(min(len(b), 48))
            if kind == 0:
                b[p] ^= 1 << rng.randrange(8)
            elif kind == 1:
                b[p] = rng.choice([0x00, 0xFF, 0xFE, 0x01, b[p] ^ 0x80])
            elif kind == 2:
                del b[p:p + rng.choice([1, 1, 2, len(b)])]
            else:
                b[p:p] = bytes(rng.getrandbits(8) for _ in range(rng.choice([1, 1, 2, 9])))
            cases.append((bytes(b), len(data)) if whole else (s[:at] + bytes(b) + s[-8:], len(data)))
    return cases


def test_random_damage_to_members_never_reads_or_writes_outside(exes):
    cases = damaged_members()
    assert len(cases) > 3000
    got = run_members(exes, "san", cases)
    assert [g for g, _ in run_members(exes, "plain", cases)] == [g for g, _ in got]
    refused = accepted = 0
    for k, ((s, declared), (g, _)) in enumerate(zip(cases, got)):
        assert (isinstance(g, bytes) and len(g) == declared) or R_GZIP_MEMBER <= g <= R_GZIP_TRAILER, k
        if isinstance(g, int) and g <= R_GZIP_SIZE:
            refused += 1
            continue                                       # (the header check: there is no body to give the reference)
        d = zlib.decompressobj(-15)
        try:
            want = d.decompress(body_of(s)[1])
            ok = d.eof
        except zlib.error:
            ok = False
        if not ok:
            assert isinstance(g, int), (k, "the reference refuses the body, the decoder does not")
        elif isinstance(g, bytes) and len(want) == declared:
            assert g == want, k
        refused += isinstance(g, int)
        accepted += isinstance(g, bytes)
    assert refused > len(cases) // 3 and accepted > 20     # (no checksum is verified: damage may decode)


# ---------------------------------------------------------------- whole files: the page walk with the gzip switch
def run_pages(exes, which, path, schema, proj=None, level=1, encodings=1, codecs=1, gzip=1):
    out_path = str(exes["dir"] / "pages.out")
    args = [exes[which], "pages", path, ",".join(_code(f.type) for f in schema), ",".join(map(str, proj)) if proj else "-", str(level), str(encodings), str(codecs),
            str(gzip), out_path]
    lines = _finish(subprocess.run(args, capture_output=True))
    if lines[0].startswith("NEEDS_HOST"):
        return lines[0], []
    raw, at, res = open(out_path, "rb").read(), 0, []
    while at < len(raw):
        page, reason, n = struct.unpack_from("<III", raw, at)
        at += 12
        res.append((page, reason, raw[at:at + n]))
        at += n
    assert len(lines) == 1 and int(lines[0].split()[1]) == len(res)
    return lines[0], res


def gzip_table(n=3000):
    k = np.arange(n)
    rng = np.random.default_rng(11)
    return pa.table({"i": pa.array(k * 7 % 1000, pa.int64(), mask=k % 5 == 0), "f": pa.array(rng.random(n)), "s": pa.array(["str%d" % (v % 17) for v in k], mask=k % 7 == 0),
                     "p": pa.array(rng.integers(0, 1 << 40, n), pa.int64()), "b": pa.array(k % 3 == 0)})


def unpacked_by_zlib(path, col):
    """what zlib makes of the compressed values of every page of a column, over all row groups, in the order of the pages"""
    want = []
    for rg in range(pq.ParquetFile(path).metadata.num_row_groups):
        data, pages = _pages(path, col, rg)
        for pg in pages:
            lev = pg["h"][8][5][0] + pg["h"][8][6][0] if pg["type"] == 3 else 0          # (V2: the levels lie uncompressed in front)
            payload = data[pg["payload"] + lev:pg["payload"] + pg["size"]]
            if pg["type"] == 3 and (len(payload) == 0 or pg["h"][8].get(7, True) is False):
                continue                                   # (nothing to unpack, or values the writer left uncompressed)
            want.append(zlib.decompress(payload, 31))
            assert len(want[-1]) == pg["h"][2][0] - lev
    return want


@pytest.mark.parametrize("version", ("1.0", "2.0"))
@pytest.mark.parametrize("dictionary", (True, False))
@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_the_pages_of_gzip_files_unpack_to_what_zlib_unpacks(exes, layout, dictionary, version):
    tbl = gzip_table()
    for level in (1, 6, 9):
        path = str(exes["dir"] / "g.parquet")
        pq.write_table(tbl, path, compression="gzip", compression_level=level, use_dictionary=dictionary, data_page_version=version, **LAYOUTS[layout])
        assert pq.ParquetFile(path).metadata.row_group(0).column(0).compression == "GZIP"
        for col in range(tbl.num_columns):
            want = unpacked_by_zlib(path, col)
            for which in BOTH if level == 6 else ("plain",):
                head, got = run_pages(exes, which, path, tbl.schema, [col], encodings=2 if version == "2.0" else 1)
                assert head == "PAGES %d 0 0" % len(want)
                assert all(r == 0 for _, r, _ in got)
                assert [g for _, _, g in got] == want, col
        head, got = run_pages(exes, "plain", path, tbl.schema, encodings=2)                     # every column: the slots do not overlap
        assert head.startswith("PAGES ") and all(r == 0 for _, r, _ in got)


def test_the_four_switches_are_independent(exes):
    tbl = gzip_table(800)
    path = str(exes["dir"] / "sw.parquet")

    def answers(**kw):
        return [run_pages(exes, w, path, tbl.schema, **kw)[0] for w in BOTH]
    pq.write_table(tbl, path, compression="gzip")
    for level in (1, 2):                                   # the switch off is what it was, whatever the other three say
        for encodings in (1, 2):
            for codecs in (1, 2):
                assert answers(level=level, encodings=encodings, codecs=codecs, gzip=0) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2
    npages = sum(len(_pages(path, c)[1]) for c in range(tbl.num_columns))
    assert answers(gzip=1) == ["PAGES %d 0 0" % npages] * 2
    # SNAPPY stays with the level
    pq.write_table(tbl, path, compression={"i": "snappy", "f": "gzip", "s": "gzip", "p": "NONE", "b": "snappy"})
    assert answers(level=1, gzip=1) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2
    assert answers(level=2, gzip=0) == ["NEEDS_HOST %d 0 1 -1" % R_CODEC] * 2
    head = answers(level=2, gzip=1)
    assert head[0] == head[1] and head[0].split()[0] == "PAGES" and int(head[0].split()[1]) >= 3 and head[0].split()[2] == "0" and int(head[0].split()[3]) >= 3
    head = answers(level=1, gzip=1, proj=[1, 3, 2])                                               # (an unprojected codec is not looked at)
    assert head[0] == head[1] and head[0].split()[2:] == ["0", "0"] and int(head[0].split()[1]) >= 3
    # ZSTD stays with the codec set
    pq.write_table(tbl, path, compression={"i": "zstd", "f": "gzip", "s": "gzip", "p": "NONE", "b": "zstd"})
    assert answers(codecs=1, gzip=1) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2
    assert answers(codecs=2, gzip=0) == ["NEEDS_HOST %d 0 1 -1" % R_CODEC] * 2
    head = answers(codecs=2, gzip=1)
    assert head[0] == head[1] and head[0].split()[0] == "PAGES" and int(head[0].split()[1]) >= 3 and int(head[0].split()[2]) >= 3 and head[0].split()[3] == "0"
    head = answers(codecs=1, gzip=1, proj=[2, 1])
    assert head[0] == head[1] and head[0].split()[2:] == ["0", "0"] and int(head[0].split()[1]) >= 2
    for codec in ("lz4", "brotli"):                        # these stay on the host
        if pa.Codec.is_available(codec):
            pq.write_table(tbl, path, compression=codec)
            assert answers(level=2, codecs=2, encodings=2, gzip=1) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2, codec
    # data pages V2 need the encoding set as well
    pq.write_table(tbl, path, compression="gzip", data_page_version="2.0")
    assert all(a.startswith("NEEDS_HOST %d " % R_PAGE_V2) for a in answers(gzip=1))
    assert all(a.startswith("PAGES ") for a in answers(gzip=1, encodings=2))


def gzip_hostile_table():
    k = np.arange(3000)
    return pa.table({"i": pa.array(k * 7 % 1000, pa.int64(), mask=k % 5 == 0), "s": pa.array(["str%d" % (v % 17) for v in k], mask=k % 7 == 0)})


def damaged_gzip_file(path, what="isize"):
    """the file of gzip_hostile_table() (compression="gzip", use_dictionary=False, data_page_size=4096) with column 0's second page
    damaged in place. "isize": its ISIZE one higher, which the page walk sees; "btype": the type of its first block overwritten by
    the reserved type 3, which only the decoder sees. -> (bytes, where: "0 0 1")"""
    data, pages = _pages(path, 0)
    assert len(pages) >= 3 and all(pg["type"] == 0 for pg in pages)
    at, size = pages[1]["payload"], pages[1]["size"]
    assert data[at:at + 4] == b"\x1f\x8b\x08\x00"
    if what == "btype":
        return data[:at + 10] + bytes([data[at + 10] | 6]) + data[at + 11:], "0 0 1"
    end = at + size
    return data[:end - 4] + struct.pack("<I", struct.unpack_from("<I", data, end - 4)[0] + 1) + data[end:], "0 0 1"


def test_a_gzip_page_damaged_in_place(exes):
    tbl = gzip_hostile_table()
    path = str(exes["dir"] / "gzip_hostile.parquet")
    pq.write_table(tbl, path, compression="gzip", use_dictionary=False, data_page_size=4096)
    bad = str(exes["dir"] / "gzip_bad.parquet")
    data, where = damaged_gzip_file(path)
    with open(bad, "wb") as f:
        f.write(data)
    for w in BOTH:
        assert run_pages(exes, w, bad, tbl.schema)[0] == "NEEDS_HOST %d %s" % (R_GZIP_SIZE, where)
    data, where = damaged_gzip_file(path, "btype")
    with open(bad, "wb") as f:
        f.write(data)
    for w in BOTH:
        head, got = run_pages(exes, w, bad, tbl.schema)
        assert head.startswith("PAGES ") and [(p, r) for p, r, _ in got if r] == [(1, R_GZIP_BLOCK)]
    # random single-byte damage inside the compressed pages: a reason or pages, never a report
    good = open(path, "rb").read()
    pages = _pages(path, 0)[1]
    first, last = pages[0]["payload"], pages[-1]["payload"] + pages[-1]["size"]
    rng = random.Random(5)
    for _ in range(60):
        at = rng.randrange(first, last)
        with open(bad, "wb") as f:
            f.write(good[:at] + bytes([rng.choice([0x00, 0xFF, 0xFE, good[at] ^ 0x10])]) + good[at + 1:])
        head, got = run_pages(exes, "san", bad, tbl.schema)
        assert head.startswith("NEEDS_HOST ") or head.startswith("PAGES "), (at, head)
        assert all(r == 0 or R_GZIP_MEMBER <= r <= R_GZIP_TRAILER for _, r, _ in got)
