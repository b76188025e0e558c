"""Codec set 2 of the device Parquet decoder without a GPU: tests/cpp/parquet_zstd_tests.cpp contains the page walk
at codec set 2 (csrc/parquet_meta.hpp) and the Zstandard decoder k_pq_unzstd runs (csrc/device/qhip_zstd.inc, the same text with
loops that stand for the lanes). Raw frames are compared with `pyarrow.Codec("zstd").decompress`, the pages of whole files with
the same over each page's payload. Built with g++ as a stand-alone program (nothing of it is loaded into Python), plainly and
with the address and undefined-behaviour sanitizers; every frame is decoded from and into heap blocks of exactly its sizes, so a
hostile frame must end in its reason and never in a report. All comparisons are exact.

The frame lists below are also what tests/test_gpu_parquet_zstd.py sends through the device."""
import os
import random
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests.test_parquet_cpu import BOTH, FLAGS, R_CODEC, R_PAGE_V2, SAN, _code, _finish, _pages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "parquet_zstd_tests.cpp")
(R_ZSTD_FRAME, R_ZSTD_SIZE, R_ZSTD_BLOCK, R_ZSTD_LITERALS, R_ZSTD_HUFFMAN, R_ZSTD_FSE, R_ZSTD_SEQUENCES, R_ZSTD_BITS, R_ZSTD_OUTPUT,
 R_ZSTD_OFFSET) = range(48, 58)
LEVELS = (1, 3, 9, 19)

# what of the format a frame used (QH_ZSF_* of qhip_zstd.inc)
F_BLOCK_RAW, F_BLOCK_RLE, F_BLOCK_COMPRESSED, F_LIT_RAW, F_LIT_RLE, F_LIT_HUFFMAN, F_LIT_TREELESS, F_STREAMS1, F_STREAMS4, F_WEIGHTS_DIRECT, F_WEIGHTS_FSE = range(11)
F_LL, F_OF, F_ML, F_REP, F_COUNT3, F_LL0 = 11, 15, 19, 23, 27, 28
# the compressor must reach all of these over compressed_inputs(); the hand-made frames add the rest
COMPRESSOR_FORMS = ([F_BLOCK_RAW, F_BLOCK_RLE, F_BLOCK_COMPRESSED, F_LIT_RAW, F_LIT_HUFFMAN, F_LIT_TREELESS, F_STREAMS1, F_STREAMS4, F_WEIGHTS_FSE]
                    + [F_LL + m for m in range(4)] + [F_OF + m for m in range(4)] + [F_ML + m for m in range(4)] + [F_REP + i for i in range(4)])
HANDMADE_FORMS = [F_LIT_RLE, F_WEIGHTS_DIRECT, F_COUNT3, F_LL0, F_REP + 3, F_BLOCK_RAW, F_BLOCK_RLE, F_STREAMS1, F_STREAMS4]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_zstd_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("parquet_zstd_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


# ---------------------------------------------------------------- Zstandard frames by hand (RFC 8878)
MAGIC = bytes([0x28, 0xB5, 0x2F, 0xFD])
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def backward_bits(reads):
    """a backward bit stream from [(value, bits)] in the order the decoder reads them"""
    x, pos = 0, 0
    for v, n in reversed(reads):
        assert 0 <= v < 1 << n if n else v == 0
        x |= v << pos
        pos += n
    x |= 1 << pos                                         # the end mark
    return x.to_bytes(pos // 8 + 1, "little")


def xxh64(data, seed=0):
    """XXH64, whose low 4 bytes are a frame's content checksum"""
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
    rotl = lambda x, r: (x << r | x >> (64 - r)) & M      # noqa: E731
    rnd = lambda acc, v: rotl((acc + v * P2) & M, 31) * P1 & M      # noqa: E731
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        while p + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(data[p + 8 * k:p + 8 * k + 8], "little"))
            p += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[p:p + 8], "little")), 27) * P1 + P4) & M
        p += 8
    if p + 4 <= n:
        h = (rotl(h ^ int.from_bytes(data[p:p + 4], "little") * P1 & M, 23) * P2 + P3) & M
        p += 4
    while p < n:
        h = rotl(h ^ data[p] * P5 & M, 11) * P1 & M
        p += 1
    h = (h ^ h >> 33) * P2 & M
    h = (h ^ h >> 29) * P3 & M
    return h ^ h >> 32


def fwd_bits(fields):
    """forward bits, least significant first, from [(value, bits)]"""
    x, pos = 0, 0
    for v, n in fields:
        x |= v << pos
        pos += n
    return x.to_bytes((pos + 7) // 8, "little")


def frame(blocks, n, fcs=None, window=False, checksum=None):
    """fcs: None for none (then a window byte), else its bytes 1 / 2 / 4 / 8; window: a window byte next to an FCS of 2+ bytes;
    checksum: the content, whose checksum follows the last block"""
    flag = {None: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs]
    single = fcs is not None and not window
    assert fcs != 1 or single
    out = MAGIC + bytes([flag << 6 | (0x20 if single else 0) | (4 if checksum is not None else 0)])
    if not single:
        out += b"\x58"                                    # 1 MB: never enforced
    if fcs:
        out += (n - 256 if fcs == 2 else n).to_bytes(fcs, "little")
    out += b"".join(blocks)
    return out + ((xxh64(checksum) & 0xFFFFFFFF).to_bytes(4, "little") if checksum is not None else b"")


def block(kind, size, body, last=False):
    return (int(last) | kind << 1 | size << 3).to_bytes(3, "little") + body


def raw_block(data, last=False):
    return block(0, len(data), data, last)


def rle_block(byte, count, last=False):
    return block(1, count, bytes([byte]), last)


def comp_block(literals, sequences, last=False):
    return block(2, len(literals) + len(sequences), literals + sequences, last)


def _lit_head(kind, n, fmt=None):
    if fmt is None:
        fmt = (n & 1) << 1 if n < 32 else 1 if n < 4096 else 3
    if fmt in (0, 2):
        assert n < 32 and fmt == (n & 1) << 1
        return bytes([kind | n << 3])
    return (kind | fmt << 2 | n << 4).to_bytes(2 if fmt == 1 else 3, "little")


def lit_raw(data, fmt=None):
    return _lit_head(0, len(data), fmt) + data


def lit_rle(byte, count, fmt=None):
    return _lit_head(1, count, fmt) + bytes([byte])


def huffman_codes(weights):
    """{symbol: (code, length)} of a complete weight list (the implied last weight included)"""
    total = sum(1 << (w - 1) for w in weights if w)
    maxbits = total.bit_length() - 1
    assert total == 1 << maxbits
    codes, cell = {}, 0
    for w in range(1, maxbits + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (cell >> (w - 1), maxbits + 1 - w)
                cell += 1 << (w - 1)
    return codes


def lit_huffman(data, weights, streams=1, tree=True):
    """Huffman literals with direct 4-bit weights; tree=False: a treeless section that reuses the table before"""
    codes = huffman_codes(weights)
    desc = b""
    if tree:
        given = weights[:-1]
        nib = given + [0] * (len(given) & 1)
        desc = bytes([127 + len(given)]) + bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))
    enc = lambda part: backward_bits([codes[b] for b in part])      # noqa: E731
    if streams == 1:
        body, fmt = enc(data), 0
    else:
        seg = (len(data) + 3) // 4
        parts = [enc(data[k * seg:(k + 1) * seg]) for k in range(3)] + [enc(data[3 * seg:])]
        body, fmt = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts), 1
    comp = len(desc) + len(body)
    assert len(data) < 1024 and comp < 1024
    return ((2 if tree else 3) | fmt << 2 | len(data) << 4 | comp << 14).to_bytes(3, "little") + desc + body


def seq_count(n, three=False):
    if n < 128 and not three:
        return bytes([n])
    if n < 0x7F00 and not three:
        return bytes([(n >> 8) + 128, n & 255])
    return b"\xff" + (n - 0x7F00).to_bytes(2, "little")


def seq_rle(llc, ofc, mlc, extras, three=False):
    """a sequences section whose three tables are RLE: the bit stream is nothing but the extra bits. extras: [(ll, ml, of)]"""
    reads = []
    for ll, ml, of in extras:
        reads += [(of, ofc), (ml, ML_BITS[mlc]), (ll, LL_BITS[llc])]
    return seq_count(len(extras), three) + bytes([0x54, llc, ofc, mlc]) + backward_bits(reads), [(LL_BASE[llc] + ll, ML_BASE[mlc] + ml, (1 << ofc) + of) for ll, ml, of in extras]


class Model:
    """what a frame's blocks spell: the literals and (literal length, match length, offset value) triples of each block executed
    byte by byte with the repeat offsets of the format"""

    def __init__(self):
        self.out, self.rep = bytearray(), [1, 4, 8]

    def raw(self, data):
        self.out += data

    def compressed(self, literals, seqs):
        lp = 0
        for ll, ml, ov in seqs:
            self.out += literals[lp:lp + ll]
            lp += ll
            if ov > 3:
                off = ov - 3
                self.rep = [off, self.rep[0], self.rep[1]]
            else:
                idx = ov - 1 + (1 if ll == 0 else 0)
                if idx == 0:
                    off = self.rep[0]
                else:
                    off = self.rep[idx] if idx < 3 else self.rep[0] - 1
                    self.rep = [off, self.rep[0], self.rep[1]] if idx != 1 else [off, self.rep[0], self.rep[2]]
            assert 0 < off <= len(self.out)
            for _ in range(ml):
                self.out.append(self.out[-off])
        self.out += literals[lp:]


def handmade_frames():
    """{name: (frame, expected output)}: the legal forms the compressor does not emit, or not reliably"""
    rng = random.Random(23)
    rnd = lambda n, top=256: bytes(rng.randrange(top) for _ in range(n))      # noqa: E731
    out = {}

    def one(name, make, **kw):
        """make(model) -> the blocks; the frame carries the model's size"""
        m = Model()
        blocks = make(m)
        if not name.startswith("frame:") and len(m.out) < 8192:
            kw = {"fcs": 4, "window": True}                # (a block may not be larger than the window, which without a window byte is the content)
        if kw.get("checksum"):
            kw["checksum"] = bytes(m.out)
        out[name] = (frame(blocks, len(m.out), **kw), bytes(m.out))

    def simple(lits_section, literals, seqsec):
        def make(m):
            m.compressed(literals, seqsec[1])
            return [comp_block(lits_section, seqsec[0], last=True)]
        return make

    # direct 4-bit weights, one stream and four
    weights = [4, 3, 2, 0, 1, 1]                          # symbols 0..5, the last implied
    text = bytes(rng.choice([0, 0, 0, 0, 1, 1, 2, 4, 5]) for _ in range(700))
    for streams in (1, 4):
        one("direct weights, %d stream(s)" % streams, simple(lit_huffman(text, weights, streams), text, seq_rle(5, 2, 7, [(0, 0, 3), (0, 0, 1)])), fcs=2)

    def treeless(m):
        a, b = text[:300], text[300:]
        m.compressed(a, [])
        m.compressed(b, [])
        return [comp_block(lit_huffman(a, weights, 1), b"\x00"), comp_block(lit_huffman(b, weights, 4, tree=False), b"\x00", last=True)]
    one("treeless literals behind direct weights", treeless, fcs=2)
    # an odd number of weights, up to the longest code
    w11 = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]
    data = bytes(rng.choice([0] * 40 + [1] * 20 + list(range(12))) for _ in range(900))
    one("direct weights up to 11 bits", simple(lit_huffman(data, w11, 4), data, (b"\x00", [])), fcs=2)
    # RLE literals, every header size
    for count, fmt in ((20, 0), (21, 2), (300, 1), (300, 3), (5000, 3)):            # (in a 1-byte header the size's lowest bit is the format's upper bit)
        lits = bytes([0x61]) * count
        one("RLE literals %d, size format %d" % (count, fmt), simple(lit_rle(0x61, count, fmt), lits, seq_rle(3, 2, 2, [(0, 0, 0), (0, 0, 1)])), fcs=2)
    for n, fmt in ((4, 0), (5, 2), (31, 2), (40, 1), (40, 3), (4096, 3)):
        lits = rnd(n)
        one("raw literals %d, size format %d" % (n, fmt), simple(lit_raw(lits, fmt), lits, seq_rle(2, 2, 1, [(0, 0, 1)])), fcs=4)

    # the 3-byte sequence count: 0x7F00 + 5 sequences of no literals and a 3-byte match at offsets 1 .. 4
    def many(m):
        head = rnd(16)
        m.raw(head)
        sec, seqs = seq_rle(0, 2, 0, [(0, 0, rng.randrange(4)) for _ in range(0x7F00 + 5)])
        m.compressed(b"", seqs)
        return [raw_block(head), comp_block(lit_raw(b""), sec, last=True)]
    one("0x7F05 sequences", many, fcs=4)
    one("the 3-byte count for 0x7F00 sequences exactly", lambda m: (m.raw(b"abcdefgh"), m.compressed(b"", seq_rle(0, 0, 0, [(0, 0, 0)] * 0x7F00)[1]),
                                                                     [raw_block(b"abcdefgh"), comp_block(lit_raw(b""), seq_rle(0, 0, 0, [(0, 0, 0)] * 0x7F00)[0], last=True)])[2], fcs=4)

    # repeat offsets: ll == 0 with ov 1, 2 and 3 (indices 1, 2, 3), ll > 0 with ov 1 .. 3 (indices 0 .. 2)
    def repeats(m):
        head = rnd(40)
        m.raw(head)
        blocks = [raw_block(head)]
        for llc, ofc, extras in ((0, 0, [(0, 0, 0)] * 3), (0, 1, [(0, 0, 0), (0, 0, 1), (0, 0, 1), (0, 0, 0), (0, 0, 1)]), (2, 0, [(0, 0, 0)] * 2),
                                 (1, 1, [(0, 0, 0), (0, 0, 1), (0, 0, 0)]), (0, 3, [(0, 0, 4)]), (0, 1, [(0, 0, 1)] * 3)):
            sec, seqs = seq_rle(llc, ofc, 4, extras)
            lits = rnd(sum(s[0] for s in seqs) + 2)
            m.compressed(lits, seqs)
            blocks.append(comp_block(lit_raw(lits), sec))
        return blocks + [raw_block(b"", last=True)]
    one("repeat offsets, every index, with and without literals", repeats, fcs=2)

    # overlapping matches at offsets 1, 2, 3 and 4; matches of 64 and 65 bytes; an offset equal to the bytes produced
    def overlaps(m):
        lits = rnd(18)
        sec, seqs = seq_rle(3, 2, 39, [(0, 5, 0), (0, 6, 1), (0, 5, 2), (0, 6, 3), (0, 0, 0), (0, 7, 1)])      # (match lengths 59 + extra)
        m.compressed(lits + b"xyz", seqs)
        return [comp_block(lit_raw(lits + b"xyz"), sec, last=True)]
    one("overlapping matches of 64 and 65 bytes at offsets 1 .. 4", overlaps, fcs=2)
    one("an offset equal to the bytes produced", simple(lit_raw(b"hello"), b"hello", seq_rle(5, 3, 2, [(0, 0, 0)])), fcs=1)

    def longest(m):
        # a match of 131 074 bytes (65539 + 2^16 - 1), the longest the format can write, across two more blocks' worth of output
        head = rnd(100)
        m.raw(head)
        blocks = [raw_block(head)]
        for ofc, of in ((2, 0), (6, 33), (7, 0)):         # offsets 1, 94 (above the wavefront's width), 125
            sec, seqs = seq_rle(1, ofc, 52, [(0, 65535, of)])
            m.compressed(b"Q", seqs)
            blocks.append(comp_block(lit_raw(b"Q"), sec))
        m.raw(b"\x2a" * 70)
        # (the host's bound counts 128 KB per compressed block: an empty one makes room for what the long matches add)
        return blocks + [rle_block(0x2A, 70), comp_block(lit_raw(b""), b"\x00"), raw_block(b"", last=True)]
    one("matches of 131074 bytes", longest, fcs=4)

    # frame headers: no FCS (a window byte), a window byte next to an FCS, the checksum flag, every FCS size
    body = rnd(300)
    for name, kw in (("no FCS", {}), ("window byte and 4-byte FCS", {"fcs": 4, "window": True}), ("checksum flag", {"fcs": 2, "checksum": True}),
                     ("checksum flag without FCS", {"checksum": True}), ("2-byte FCS", {"fcs": 2}), ("8-byte FCS", {"fcs": 8})):
        one("frame: " + name, lambda m: (m.raw(body), [raw_block(body[:100]), raw_block(body[100:], last=True)])[1], **kw)
    one("frame: 1-byte FCS", lambda m: (m.raw(body[:200]), [raw_block(body[:200], last=True)])[1], fcs=1)
    one("frame: 2-byte FCS of 256", lambda m: (m.raw(body[:256]), [raw_block(body[:256], last=True)])[1], fcs=2)
    one("RLE blocks and empty blocks", lambda m: (m.raw(b"\x07" * 1000 + b"ab" + b"\x00" * 131072), [rle_block(7, 1000), raw_block(b""), rle_block(9, 0), raw_block(b"ab"),
                                                                                                      rle_block(0, 131072, last=True)])[1], fcs=4)
    return out


def compressed_inputs():
    """{name: bytes}: what the compressor is given, at every level of LEVELS"""
    rng = random.Random(7)
    nrng = np.random.default_rng(7)
    rnd = lambda n: bytes(rng.getrandbits(8) for _ in range(n))     # noqa: E731
    text = ("row %d of the lineitem table, shipped by %s|" * 40 % sum(((k, ("AIR", "RAIL", "TRUCK")[k % 3]) for k in range(40)), ())).encode()
    vocab = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta"]
    out = {"empty": b"", "one byte": b"q"}
    for n in (2, 3, 7, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000):
        out["text %d" % n] = (text * 2)[:n]
    out["300 000 zeros"] = bytes(300_000)
    out["1000 random bytes"] = rnd(1000)
    out["ascending int64"] = np.arange(40_000, dtype=np.int64).tobytes()
    out["random int64 prices"] = nrng.integers(100, 100_000, 40_000).astype(np.int64).tobytes()
    words = " ".join(rng.choice(vocab) for _ in range(66_000)).encode()
    out["words"] = words[:370_000]
    assert len(out["words"]) == 370_000
    out["4 symbols"] = bytes(nrng.choice(4, 200_000, p=[.7, .2, .05, .05]).astype(np.uint8))
    out["mixed"] = rnd(3000) + words[:50_000] + bytes(70_000) + out["ascending int64"][:40_000] + rnd(200) + words[1000:9000]
    return out


def good_frames():
    """{name: (frame, output)}: the compressor's outputs at every level, then the hand-made frames"""
    out = {}
    for level in LEVELS:
        codec = pa.Codec("zstd", compression_level=level)
        for name, data in compressed_inputs().items():
            out["level %d: %s" % (level, name)] = (codec.compress(data, asbytes=True), data)
    out.update(handmade_frames())
    return out


def hostile_frames():
    """{name: (frame, declared size, reason)}"""
    good = raw_block(b"0123456789", last=True)
    lits10 = lit_raw(b"0123456789")
    bad_weights = bytes([2 | 0 << 2 | 4 << 4 & 0xFF, 0, 0])      # (overwritten below)

    def comp(lits, seqs, n, **kw):
        return frame([comp_block(lits, seqs, last=True)], n, fcs=kw.pop("fcs", 1), **kw)

    def huf_section(desc_and_streams, regen, fmt=0):
        return (2 | fmt << 2 | regen << 4 | len(desc_and_streams) << 14).to_bytes(3, "little") + desc_and_streams
    del bad_weights
    fse_big = bytes([0x0F])                                # accuracy 20
    h = {
        "no bytes at all": (b"", 0, R_ZSTD_FRAME),
        "wrong magic": (b"\x28\xb5\x2f\xfc" + frame([good], 10, fcs=1)[4:], 10, R_ZSTD_FRAME),
        "a dictionary id": (MAGIC + bytes([0x21, 7, 10]) + good, 10, R_ZSTD_FRAME),
        "the reserved bit": (MAGIC + bytes([0x28, 10]) + good, 10, R_ZSTD_FRAME),
        "a second frame": (frame([good], 10, fcs=1) * 2, 10, R_ZSTD_FRAME),
        "a skippable frame": (bytes([0x50, 0x2A, 0x4D, 0x18, 4, 0, 0, 0, 1, 2, 3, 4]) + frame([good], 10, fcs=1), 10, R_ZSTD_FRAME),
        "a skippable frame behind": (frame([good], 10, fcs=1) + bytes([0x50, 0x2A, 0x4D, 0x18, 0, 0, 0, 0]), 10, R_ZSTD_FRAME),
        "3 bytes behind the last block": (frame([good], 10, fcs=1) + b"abc", 10, R_ZSTD_FRAME),
        "4 bytes behind the last block, no checksum flag": (frame([good], 10, fcs=1) + b"abcd", 10, R_ZSTD_FRAME),
        "checksum flag, 3 bytes": (frame([good], 10, fcs=1, checksum=b"0123456789")[:-1], 10, R_ZSTD_FRAME),
        "header cut off in the FCS": (MAGIC + bytes([0xE0, 1, 2, 3]), 10, R_ZSTD_FRAME),
        "FCS above the declared size": (frame([good], 11, fcs=1), 10, R_ZSTD_SIZE),
        "FCS below the declared size": (frame([good], 10, fcs=1), 11, R_ZSTD_SIZE),
        "raw blocks that add up to less": (frame([good], 11), 11, R_ZSTD_SIZE),
        "raw blocks that add up to more": (frame([good], 9), 9, R_ZSTD_SIZE),
        "a claim of 2 GB from 30 bytes": (frame([comp_block(lits10, b"\x00", last=True)], 0x7FFFFFFF), 0x7FFFFFFF, R_ZSTD_SIZE),
        "a claim one above the compressed blocks' bound": (frame([comp_block(lits10, b"\x00", last=True)], 131073), 131073, R_ZSTD_SIZE),
        "a block of type 3": (frame([block(3, 10, b"0123456789", last=True)], 10, fcs=1), 10, R_ZSTD_BLOCK),
        "a block size above 128 KB": (frame([block(0, 131073, bytes(131073), last=True)], 131073, fcs=4), 131073, R_ZSTD_BLOCK),
        "a raw block past the payload": (frame([block(0, 11, b"0123456789", last=True)], 11, fcs=1), 11, R_ZSTD_BLOCK),
        "a compressed block past the payload": (frame([block(2, 40, lits10 + b"\x00", last=True)], 10, fcs=1), 10, R_ZSTD_BLOCK),
        "an RLE block without its byte": (frame([block(1, 10, b"", last=True)], 10, fcs=1), 10, R_ZSTD_BLOCK),
        "no last block": (frame([raw_block(b"0123456789")], 10, fcs=1), 10, R_ZSTD_BLOCK),
        "a block header cut off": (frame([raw_block(b"0123456789")], 10, fcs=1) + b"\x01\x00", 10, R_ZSTD_BLOCK),
        "an empty compressed block": (comp(b"", b"", 0), 0, R_ZSTD_LITERALS),
        "raw literals past the block": (comp(_lit_head(0, 20) + b"0123456789", b"", 20), 20, R_ZSTD_LITERALS),
        "a literals header cut off": (comp(bytes([0 | 3 << 2 | 5 << 4]), b"", 5), 5, R_ZSTD_LITERALS),
        "RLE literals without their byte": (comp(_lit_head(1, 20), b"", 20), 20, R_ZSTD_LITERALS),
        "literals above 128 KB": (comp((0 | 3 << 2 | 131073 << 4).to_bytes(3, "little") + b"ab", b"\x00", 131072, fcs=4), 131072, R_ZSTD_LITERALS),
        "a Huffman section past the block": (comp((2 | 10 << 4 | 900 << 14).to_bytes(3, "little") + b"\x80\x10\x01", b"\x00", 10), 10, R_ZSTD_LITERALS),
        "four streams without a jump table": (comp(huf_section(bytes([0x81, 0x11]) + b"\x01\x01\x01", 8, fmt=1), b"\x00", 8), 8, R_ZSTD_LITERALS),
        "four streams whose sizes pass the section": (comp(huf_section(bytes([0x81, 0x11]) + b"\x09\x00\x09\x00\x09\x00" + b"\x01" * 8, 8, fmt=1), b"\x00", 8), 8, R_ZSTD_LITERALS),
        "weights that add up to no power of two": (comp(huf_section(bytes([0x81, 0x31]) + b"\x01", 4), b"\x00", 4), 4, R_ZSTD_HUFFMAN),
        "a weight of 12": (comp(huf_section(bytes([0x81, 0xC0]) + b"\x01", 4), b"\x00", 4), 4, R_ZSTD_HUFFMAN),
        "all weights zero": (comp(huf_section(bytes([0x82, 0x00]) + b"\x01", 4), b"\x00", 4), 4, R_ZSTD_HUFFMAN),
        "direct weights past the section": (comp(huf_section(bytes([0xFF, 0x11]), 4), b"\x00", 4), 4, R_ZSTD_HUFFMAN),
        "FSE weights with an accuracy of 7": (comp(huf_section(bytes([4, 0x02, 0xFF, 0xFF, 0x01]), 4), b"\x00", 4), 4, R_ZSTD_HUFFMAN),
        "treeless literals in the first block": (comp((3 | 4 << 4 | 1 << 14).to_bytes(3, "little") + b"\x01", b"\x00", 4), 4, R_ZSTD_HUFFMAN),
        "a Huffman stream that ends in a zero byte": (comp(huf_section(bytes([0x81, 0x10]) + b"\x0f\x00", 4), b"\x00", 4), 4, R_ZSTD_BITS),
        "a Huffman stream with bits left over": (comp(huf_section(bytes([0x81, 0x10]) + b"\xff\x01", 4), b"\x00", 4), 4, R_ZSTD_BITS),
        "a Huffman stream that underflows": (comp(huf_section(bytes([0x81, 0x10]) + b"\x03", 4), b"\x00", 4), 4, R_ZSTD_BITS),
        "no sequences section": (comp(lits10, b"", 10), 10, R_ZSTD_SEQUENCES),
        "bytes behind a count of 0": (comp(lits10, b"\x00\x00", 10), 10, R_ZSTD_SEQUENCES),
        "a sequence count cut off": (comp(lits10, b"\xff\x00", 10), 10, R_ZSTD_SEQUENCES),
        "reserved bits in the mode byte": (comp(lits10, bytes([1, 0x55, 0, 0, 0, 1]), 13), 13, R_ZSTD_SEQUENCES),
        "repeat mode without a table": (comp(lits10, bytes([1, 0xD4, 0, 0, 1]), 13), 13, R_ZSTD_SEQUENCES),
        "an RLE symbol outside the alphabet": (comp(lits10, bytes([1, 0x54, 36, 0, 0, 1]), 13), 13, R_ZSTD_SEQUENCES),
        "an RLE offset code of 32": (comp(lits10, bytes([1, 0x54, 0, 32, 0, 1]), 13), 13, R_ZSTD_SEQUENCES),
        "literal lengths beyond the literals": (comp(lits10, seq_rle(11, 2, 0, [(0, 0, 0)])[0], 14), 14, R_ZSTD_SEQUENCES),
        "an FSE accuracy of 20": (comp(lits10, bytes([1, 0x80]) + fse_big + b"\x00\x00\x01", 13), 13, R_ZSTD_FSE),
        "an FSE description cut off": (comp(lits10, bytes([1, 0x80, 0x04]), 13), 13, R_ZSTD_FSE),
        "an FSE description with too many symbols": (comp(lits10, bytes([1, 0x80]) + fwd_bits([(0, 4), (1, 5)] + [(3, 2)] * 13) + b"\x01", 13), 13, R_ZSTD_FSE),
        "a sequence stream that ends in a zero byte": (comp(lits10, bytes([1, 0x54, 0, 0, 0, 0]), 13), 13, R_ZSTD_BITS),
        "no sequence stream": (comp(lits10, bytes([1, 0x54, 0, 0, 0]), 13), 13, R_ZSTD_BITS),
        "a sequence stream with bits left over": (comp(lits10, bytes([1, 0x54, 1, 2, 0, 0x03]), 14), 14, R_ZSTD_BITS),
        "a sequence stream that underflows": (comp(lits10, bytes([1, 0x54, 1, 9, 0, 0x03]), 14), 14, R_ZSTD_BITS),
        "a match past the declared size": (comp(lits10, seq_rle(5, 2, 10, [(0, 0, 0)])[0], 12), 12, R_ZSTD_OUTPUT),
        "literals past the declared size": (comp(lits10, b"\x00", 9, fcs=None), 9, R_ZSTD_OUTPUT),
        "a frame that ends with output missing": (comp(lits10, b"\x00", 12, fcs=None), 12, R_ZSTD_OUTPUT),
        "a match that would pass the later literals": (comp(lits10, seq_rle(5, 2, 0, [(0, 0, 0)])[0], 12), 12, R_ZSTD_OUTPUT),
        "repeat index 3 from an offset of 1": (comp(lits10, seq_rle(0, 1, 0, [(0, 0, 1)])[0], 13), 13, R_ZSTD_OFFSET),
        "an offset one beyond the bytes produced": (comp(lits10, seq_rle(5, 3, 0, [(0, 0, 1)])[0], 13), 13, R_ZSTD_OFFSET),
        "an offset of 2^31": (comp(lits10, seq_rle(5, 31, 0, [(0, 0, 3)])[0], 13), 13, R_ZSTD_OFFSET),
        "a match as the frame's first bytes": (comp(lit_raw(b""), seq_rle(0, 0, 0, [(0, 0, 0)])[0], 3), 3, R_ZSTD_OFFSET),
    }
    return h


def run_frames(exes, which, frames):
    """frames: [(bytes, declared size)] -> per frame (its output bytes or its reason, the forms it used)"""
    path, out_path = str(exes["dir"] / "frames.bin"), str(exes["dir"] / "frames.out")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(frames)))
        for data, declared in frames:
            f.write(struct.pack("<II", len(data), declared) + data)
    assert _finish(subprocess.run([exes[which], "streams", path, out_path], capture_output=True)) == []
    raw, at, res = open(out_path, "rb").read(), 0, []
    for _ in frames:
        reason, forms, n = struct.unpack_from("<III", raw, at)
        at += 12
        res.append((reason if reason else raw[at:at + n], forms))
        at += n
    assert at == len(raw)
    return res


def cpu_model_results(exes, frames, which="plain"):
    return [r for r, _ in run_frames(exes, which, frames)]


def _missing(forms, wanted):
    return [b for b in wanted if not forms >> b & 1]


def test_compressed_frames_equal_the_reference_decoder_and_cover_the_format(exes):
    good = {k: v for k, v in good_frames().items() if k.startswith("level ")}
    codec = pa.Codec("zstd")
    for name, (s, data) in good.items():
        assert codec.decompress(s, decompressed_size=len(data), asbytes=True) == data, name
    for which in BOTH:
        got = run_frames(exes, which, [(s, len(d)) for s, d in good.values()])
        union = 0
        for (name, (_, data)), (g, forms) in zip(good.items(), got):
            assert g == data, (name, g if isinstance(g, int) else len(g))
            union |= forms
        # a different build of the compressor must not quietly test less
        assert _missing(union, COMPRESSOR_FORMS) == [], bin(union)


def test_handmade_frames_cover_what_the_compressor_does_not_emit(exes):
    made = handmade_frames()
    codec = pa.Codec("zstd")
    for name, (s, want) in made.items():
        if name == "matches of 131074 bytes":
            continue                                       # (a block that regenerates more than 128 KB: the reference refuses it)
        assert codec.decompress(s, decompressed_size=len(want), asbytes=True) == want, name        # (the frame says what its name says)
    for which in BOTH:
        got = run_frames(exes, which, [(s, len(w)) for s, w in made.values()])
        union = 0
        for (name, (_, want)), (g, forms) in zip(made.items(), got):
            assert g == want, (name, g if isinstance(g, int) else len(g))
            union |= forms
        assert _missing(union, HANDMADE_FORMS + [F_REP + i for i in range(4)]) == [], bin(union)
    assert len(made["matches of 131074 bytes"][1]) == 100 + 3 * (1 + 131074) + 70


def test_hostile_frames_are_refused_each_with_its_reason(exes):
    hostile = hostile_frames()
    for which in BOTH:
        got = run_frames(exes, which, [(s, declared) for s, declared, _ in hostile.values()])
        for (name, (_, _, reason)), (g, _) in zip(hostile.items(), got):
            assert g == reason, (name, g if isinstance(g, int) else "decoded %d bytes" % len(g))
    # every truncation of good frames: a reason, never a report, and never an output
    good = good_frames()
    cuts = []
    for name in ("level 3: words", "level 19: mixed", "level 1: 4 symbols", "direct weights, 4 stream(s)", "repeat offsets, every index, with and without literals"):
        s, data = good[name]
        cuts += [(s[:k], len(data)) for k in list(range(0, min(len(s), 60))) + [len(s) // 2, len(s) - 5, len(s) - 1]]
    for g, _ in run_frames(exes, "san", cuts):
        assert isinstance(g, int) and R_ZSTD_FRAME <= g <= R_ZSTD_OFFSET, g


def test_random_damage_to_frames_never_reads_or_writes_outside(exes):
    rng = random.Random(13)
    good = good_frames()
    cases = []
    for name in ("level 3: words", "level 9: mixed", "level 19: 4 symbols", "level 1: random int64 prices", "level 3: text 1000", "direct weights, 4 stream(s)",
                 "0x7F05 sequences", "overlapping matches of 64 and 65 bytes at offsets 1 .. 4"):
        s, data = good[name]
        for _ in range(40):
            at = rng.randrange(len(s)) if rng.random() < 0.5 else rng.randrange(min(len(s), 200))
            cases.append((s[:at] + bytes([rng.choice([0x00, 0xFF, 0xFE, 0xF0, 0x01, s[at] ^ 0x04, s[at] ^ 0x80])]) + s[at + 1:], len(data)))
    refused = 0
    for g, _ in run_frames(exes, "san", cases):
        assert isinstance(g, bytes) or R_ZSTD_FRAME <= g <= R_ZSTD_OFFSET      # (no checksum is verified: damage may decode)
        refused += isinstance(g, int)
    assert refused > len(cases) // 4


# ---------------------------------------------------------------- whole files: the page walk at codec set 2
def run_pages(exes, which, path, schema, proj=None, level=1, encodings=1, codecs=2):
    out_path = str(exes["dir"] / "pages.out")
    args = [exes[which], "pages", path, ",".join(_code(f.type) for f in schema), ",".join(map(str, proj)) if proj else "-", str(level), str(encodings), str(codecs), out_path]
    lines = _finish(subprocess.run(args, capture_output=True))
    if lines[0].startswith("NEEDS_HOST"):
        return lines[0], []
    raw, at, res = open(out_path, "rb").read(), 0, []
    while at < len(raw):
        page, reason, n = struct.unpack_from("<III", raw, at)
        at += 12
        res.append((page, reason, raw[at:at + n]))
        at += n
    assert lines == ["PAGES %d %s" % (len(res), lines[0].split()[2])]
    return lines[0], res


def zstd_table(n=6000):
    k = np.arange(n)
    rng = np.random.default_rng(11)
    return pa.table({"i": pa.array(k * 7 % 1000, pa.int64(), mask=k % 5 == 0), "f": pa.array(rng.random(n)), "s": pa.array(["str%d" % (v % 17) for v in k], mask=k % 7 == 0),
                     "p": pa.array(rng.integers(0, 1 << 40, n), pa.int64()), "b": pa.array(k % 3 == 0)})


@pytest.mark.parametrize("page_size", (4096, 1 << 20))
@pytest.mark.parametrize("dictionary", (True, False))
def test_the_pages_of_zstd_files_unpack_to_what_the_reference_unpacks(exes, page_size, dictionary):
    tbl = zstd_table()
    codec = pa.Codec("zstd")
    for level in (1, 9):
        path = str(exes["dir"] / "z.parquet")
        pq.write_table(tbl, path, compression="zstd", compression_level=level, use_dictionary=dictionary, data_page_size=page_size)
        assert pq.ParquetFile(path).metadata.row_group(0).column(0).compression == "ZSTD"
        for col in range(tbl.num_columns):
            data, pages = _pages(path, col)
            want = [codec.decompress(data[pg["payload"]:pg["payload"] + pg["size"]], decompressed_size=pg["h"][2][0], asbytes=True) for pg in pages]
            for which in BOTH:
                head, got = run_pages(exes, which, path, tbl.schema, [col])
                assert head == "PAGES %d 0" % len(pages)
                assert [(p, r) for p, r, _ in got] == [(p, 0) for p in range(len(pages))]
                assert [g for _, _, g in got] == want, col
        head, got = run_pages(exes, "plain", path, tbl.schema)                                  # every column: the slots do not overlap
        assert head.startswith("PAGES ") and all(r == 0 for _, r, _ in got)


def test_the_three_switches_are_independent(exes):
    tbl = zstd_table(800)
    path = str(exes["dir"] / "sw.parquet")

    def answers(**kw):
        return [run_pages(exes, w, path, tbl.schema, **kw)[0] for w in BOTH]
    pq.write_table(tbl, path, compression="zstd")
    for level in (1, 2):                                   # codec set 1 is what it was, whatever the level
        assert answers(level=level, codecs=1) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2
    npages = sum(len(_pages(path, c)[1]) for c in range(tbl.num_columns))
    assert answers(level=1, codecs=2) == ["PAGES %d 0" % npages] * 2
    # SNAPPY stays with the level
    pq.write_table(tbl, path, compression={"i": "snappy", "f": "zstd", "s": "zstd", "p": "NONE", "b": "snappy"})
    assert answers(level=1, codecs=2) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2
    assert answers(level=2, codecs=1) == ["NEEDS_HOST %d 0 1 -1" % R_CODEC] * 2
    head = answers(level=2, codecs=2)
    assert head[0] == head[1] and head[0].split()[0] == "PAGES" and int(head[0].split()[1]) >= 3 and int(head[0].split()[2]) >= 3
    assert answers(level=2, codecs=2, proj=[3, 0, 4]) == ["PAGES 0 %d" % 3] * 2                  # (an unprojected codec is not looked at)
    for codec in ("gzip", "lz4", "brotli"):
        if pa.Codec.is_available(codec):
            pq.write_table(tbl, path, compression=codec)
            assert answers(level=2, codecs=2, encodings=2) == ["NEEDS_HOST %d 0 0 -1" % R_CODEC] * 2, codec
    # data pages V2 need the encoding set as well: the levels stay uncompressed in front
    pq.write_table(tbl, path, compression="zstd", data_page_version="2.0")
    assert all(a.startswith("NEEDS_HOST %d " % R_PAGE_V2) for a in answers(codecs=2))
    codec = pa.Codec("zstd")
    for which in BOTH:
        for col in range(tbl.num_columns):
            head, got = run_pages(exes, which, path, tbl.schema, [col], encodings=2)
            data, pages = _pages(path, col)
            assert head.startswith("PAGES ") and all(r == 0 for _, r, _ in got)
            for (page, _, g), pg in zip(got, [pages[p] for p, _, _ in got]):
                if pg["type"] == 3:
                    lev = pg["h"][8][5][0] + pg["h"][8][6][0]
                    assert g == codec.decompress(data[pg["payload"] + lev:pg["payload"] + pg["size"]], decompressed_size=pg["h"][2][0] - lev, asbytes=True)


def zstd_hostile_table():
    k = np.arange(3000)
    return pa.table({"i": pa.array(k * 7 % 1000, pa.int64(), mask=k % 5 == 0), "s": pa.array(["str%d" % (v % 17) for v in k], mask=k % 7 == 0)})


def damaged_zstd_file(path):
    """the file of zstd_hostile_table() (compression="zstd", use_dictionary=False, data_page_size=4096) with the type of the first
    block of column 0's second page overwritten in place by the reserved type 3. -> (bytes, where: "0 0 1")"""
    data, pages = _pages(path, 0)
    assert len(pages) >= 3 and all(pg["type"] == 0 for pg in pages)
    at = pages[1]["payload"]
    assert data[at:at + 4] == MAGIC
    d = data[at + 4]
    at += 5 + (0 if d & 0x20 else 1) + {0: d >> 5 & 1, 1: 2, 2: 4, 3: 8}[d >> 6]
    return data[:at] + bytes([data[at] | 6]) + data[at + 1:], "0 0 1"


def test_a_zstd_page_damaged_in_place(exes):
    tbl = zstd_hostile_table()
    path = str(exes["dir"] / "zstd_hostile.parquet")
    pq.write_table(tbl, path, compression="zstd", use_dictionary=False, data_page_size=4096)
    data, where = damaged_zstd_file(path)
    bad = str(exes["dir"] / "zstd_bad.parquet")
    with open(bad, "wb") as f:
        f.write(data)
    for w in BOTH:
        assert run_pages(exes, w, bad, tbl.schema)[0] == "NEEDS_HOST %d %s" % (R_ZSTD_BLOCK, where)
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
        assert all(r == 0 or R_ZSTD_FRAME <= r <= R_ZSTD_OFFSET for _, r, _ in got)
