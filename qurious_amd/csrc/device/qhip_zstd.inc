// qhip_zstd.inc — the device Zstandard decoder (kernels_parquet.hip k_pq_unzstd; parquet_meta.hpp, parquet.cpp; DESIGN §3.9,
// codec set 2): a complete decoder of one Zstandard frame (RFC 8878) without a dictionary. The frame and block header readers
// and the size walk the host makes before anything is reserved; the literals-section header; the FSE distribution reader and
// table builder; the Huffman weight reader and table builder; the backward bit reader; the per-sequence decode with the repeat
// offsets; the block walk itself (qh_zstd_frame), and every check that comes before an access.
//
// One text for two compilers, as qhip_snappy.inc is: included by kernels_parquet.hip for hipcc and, as plain host C++, by
// parquet_meta.hpp and tests/cpp/parquet_zstd_tests.cpp. Self-contained: builtin integer types only, no #include. The walk is
// wave-uniform: every lane parses the same bytes and builds the same tables (all lanes store the same value to the same LDS
// word). Where the lanes differ the text says QH_ZS_LANES(l): the lane's own index for hipcc, a loop over 64 lanes for a host
// compiler; a step whose lanes all load before any of them stores keeps the loaded bytes in `got`, one per lane.
//
// The loops of the table builders carry `unroll 1`: they run once per block at the most, and unrolled their loads in flight cost
// the kernel more than half its registers (234 against 96 VGPRs) and with them half its resident wavefronts.
//
// All lengths, counts, accuracy logs, weights and offsets are untrusted. Positions inside a page fit 32 bits. The content
// checksum of a frame is skipped, not verified. Window_Size is not enforced: an offset may reach back to the page's first byte
// and never behind it.
#ifndef QHIP_ZSTD_INC
#define QHIP_ZSTD_INC

typedef unsigned char zs_u8;
typedef unsigned short zs_u16;
typedef short zs_i16;
typedef unsigned int zs_u32;
typedef int zs_i32;
typedef unsigned long long zs_u64;

#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define QH_ZS_HD __host__ __device__ __forceinline__
#define QH_ZS_DEV __device__ __forceinline__
#define QH_ZS_LANES(l) for (zs_u32 l = lane, qh_zs_once = 1; qh_zs_once; qh_zs_once = 0)
#define QH_ZS_NL 1
#define QH_ZS_SLOT(l) 0
#define QH_ZS_ANY(x) (__builtin_amdgcn_ballot_w64((x) != 0) != 0)
#define QH_ZS_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")
#else
#define QH_ZS_HD static inline
#define QH_ZS_DEV static inline
#define QH_ZS_LANES(l) for (zs_u32 l = 0; l < 64; ++l)
#define QH_ZS_NL 64
#define QH_ZS_SLOT(l) (l)
#define QH_ZS_ANY(x) ((x) != 0)
#define QH_ZS_FENCE() ((void)0)
#endif
#ifndef QH_ZS_FORM   // (the CPU test records which forms of the format a stream used)
#define QH_ZS_FORM(bit) ((void)0)
#endif

// why a frame is refused (the Parquet reasons QH_PQ_R_ZSTD_* are QH_PQ_R_ZSTD_BASE + these)
#define QH_ZSTD_OK 0
#define QH_ZSTD_E_FRAME 1       // the frame header: magic, a dictionary id, the reserved bit, a skippable frame, bytes behind the last block
#define QH_ZSTD_E_SIZE 2        // Frame_Content_Size or the blocks' bound against the declared uncompressed size
#define QH_ZSTD_E_BLOCK 3       // a block header: cut off, the reserved type, above 128 KB, past the payload, no last block
#define QH_ZSTD_E_LITERALS 4    // the literals section: cut off, above 128 KB, stream sizes that do not fit
#define QH_ZSTD_E_HUFFMAN 5     // the Huffman tree description, or a treeless section without an earlier tree
#define QH_ZSTD_E_FSE 6         // an FSE table description
#define QH_ZSTD_E_SEQUENCES 7   // the sequences section: cut off, reserved bits, a repeat mode without a table, literal lengths beyond the literals
#define QH_ZSTD_E_BITS 8        // a backward bit stream that is empty, ends in a zero byte, underflows or does not end exactly at its start
#define QH_ZSTD_E_OUTPUT 9      // output past the declared size, or the frame ends with output missing
#define QH_ZSTD_E_OFFSET 10     // a match offset of 0, or one beyond the bytes produced
#define QH_ZSTD_E_COUNT 11

#define QH_ZSTD_BLOCK_MAX 131072u

// the forms of the format (QH_ZS_FORM)
#define QH_ZSF_BLOCK 0      // + block type 0..2
#define QH_ZSF_LIT 3        // + literals type 0..3
#define QH_ZSF_STREAMS1 7
#define QH_ZSF_STREAMS4 8
#define QH_ZSF_WEIGHTS_DIRECT 9
#define QH_ZSF_WEIGHTS_FSE 10
#define QH_ZSF_LL 11        // + mode 0..3
#define QH_ZSF_OF 15
#define QH_ZSF_ML 19
#define QH_ZSF_REP 23       // + repeat index 0..3
#define QH_ZSF_COUNT3 27    // the 3-byte sequence count
#define QH_ZSF_LL0 28       // a repeat code behind a literal length of 0
#define QH_ZSF_COUNT 29

// The tables of one page, in LDS on the device (10 148 bytes, so that 16 wavefronts fit a CU's 160 KB): they persist across the
// blocks of a frame (treeless literals, repeat mode). An FSE cell: symbol | bits to read << 8 | base of the next state << 16.
// A Huffman cell: symbol | code length << 8. llc / mlc: the code tables above, copied once per frame so that a sequence reads
// no table in global memory. wt, the FSE table of the Huffman weights, is done with before the Huffman table is filled and
// lies in its first bytes.
typedef struct qh_zs_tables {
  zs_u32 ll[512], ml[512], of[256];
  zs_u32 llc[36], mlc[53];
  union {
    zs_u16 huf[2048];
    zs_u32 wt[64];
  };
  zs_i16 norm[64];
  zs_u16 next[64];
  zs_u32 rank[16];
  zs_u8 w[256];
} qh_zs_tables;

// value and extra bits of the literal-length and match-length codes: base | bits << 24
static const zs_u32 qh_zs_ll_code[36] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
    16 | 1u << 24, 18 | 1u << 24, 20 | 1u << 24, 22 | 1u << 24, 24 | 2u << 24, 28 | 2u << 24, 32 | 3u << 24, 40 | 3u << 24, 48 | 4u << 24, 64 | 6u << 24,
    128 | 7u << 24, 256 | 8u << 24, 512 | 9u << 24, 1024 | 10u << 24, 2048 | 11u << 24, 4096 | 12u << 24, 8192 | 13u << 24, 16384 | 14u << 24, 32768 | 15u << 24,
    65536 | 16u << 24};
static const zs_u32 qh_zs_ml_code[53] = {
    3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
    35 | 1u << 24, 37 | 1u << 24, 39 | 1u << 24, 41 | 1u << 24, 43 | 2u << 24, 47 | 2u << 24, 51 | 3u << 24, 59 | 3u << 24, 67 | 4u << 24, 83 | 4u << 24, 99 | 5u << 24,
    131 | 7u << 24, 259 | 8u << 24, 515 | 9u << 24, 1027 | 10u << 24, 2051 | 11u << 24, 4099 | 12u << 24, 8195 | 13u << 24, 16387 | 14u << 24, 32771 | 15u << 24,
    65539 | 16u << 24};
// the predefined distributions (accuracy 6, 6, 5)
static const zs_i16 qh_zs_ll_default[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
static const zs_i16 qh_zs_ml_default[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                            1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
static const zs_i16 qh_zs_of_default[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};

QH_ZS_HD zs_u32 qh_zs_bitlen(zs_u32 x) { return x ? 32u - (zs_u32)__builtin_clz(x) : 0u; }   // (bits needed to write x)

// ---------------------------------------------------------------- the host's part: before anything is reserved
// The frame at s[0 .. len) that is to fill `declared` bytes: its header, then the chain of 3-byte block headers, which costs
// nothing and gives the bound on what the frame can produce. *start: where the first block header lies.
QH_ZS_HD int qh_zstd_check_frame(const zs_u8* s, zs_u64 len, zs_u64 declared, zs_u32* start) {
  if (len < 5) return QH_ZSTD_E_FRAME;
  const zs_u32 magic = (zs_u32)s[0] | (zs_u32)s[1] << 8 | (zs_u32)s[2] << 16 | (zs_u32)s[3] << 24;
  if (magic != 0xFD2FB528u) return QH_ZSTD_E_FRAME;   // (a skippable frame, 0x184D2A5x, among the rest)
  const zs_u32 d = s[4];
  const zs_u32 fcs_flag = d >> 6, single = (d >> 5) & 1u, checksum = (d >> 2) & 1u;
  if ((d & 8u) || (d & 3u)) return QH_ZSTD_E_FRAME;   // the reserved bit; a dictionary id
  zs_u64 at = 5;
  if (!single) at += 1;   // Window_Descriptor: not enforced
  const zs_u32 fcs_bytes = fcs_flag == 0 ? single : fcs_flag == 1 ? 2u : fcs_flag == 2 ? 4u : 8u;
  if (at + fcs_bytes > len) return QH_ZSTD_E_FRAME;
  if (fcs_bytes) {
    zs_u64 fcs = 0;
    for (zs_u32 i = 0; i < fcs_bytes; ++i) fcs |= (zs_u64)s[at + i] << (8 * i);
    if (fcs_bytes == 2) fcs += 256;
    if (fcs != declared) return QH_ZSTD_E_SIZE;
  }
  at += fcs_bytes;
  *start = (zs_u32)at;
  zs_u64 bound = 0, exact = 0;
  int compressed = 0;
  for (;;) {
    if (len - at < 3) return QH_ZSTD_E_BLOCK;
    const zs_u32 h = (zs_u32)s[at] | (zs_u32)s[at + 1] << 8 | (zs_u32)s[at + 2] << 16;
    const zs_u32 type = (h >> 1) & 3u, size = h >> 3;
    at += 3;
    if (type == 3 || size > QH_ZSTD_BLOCK_MAX) return QH_ZSTD_E_BLOCK;
    const zs_u64 body = type == 1 ? 1u : size;
    if (body > len - at) return QH_ZSTD_E_BLOCK;
    at += body;
    if (type == 2) { compressed = 1; bound += QH_ZSTD_BLOCK_MAX; }
    else { bound += size; exact += size; }
    if (h & 1u) break;
  }
  if (len - at != (checksum ? 4u : 0u)) return QH_ZSTD_E_FRAME;   // (a second frame, or anything else behind the last block)
  if (declared > bound || (!compressed && declared != exact)) return QH_ZSTD_E_SIZE;
  return QH_ZSTD_OK;
}

// ---------------------------------------------------------------- bits
// A backward bit stream p[0 .. len): its last byte is not zero and that byte's highest set bit is the end mark. `pos`: the bits
// still unread, which are bits [0, pos) of the stream taken as one little-endian number. A read takes the n bits below pos.
// Bits below bit 0 read as zeros and leave pos negative: the caller checks pos. The window holds bits [wbit, wbit + 64).
typedef struct qh_zs_bits {
  const zs_u8* p;
  zs_u32 len;
  zs_i32 pos, wbit;
  zs_u64 win;
} qh_zs_bits;

QH_ZS_HD zs_u64 qh_zs_load64(const zs_u8* p, zs_u32 len, zs_i32 byte) {
  zs_u64 v = 0;
  if (byte >= 0 && (zs_u32)byte + 8 <= len) { __builtin_memcpy(&v, p + byte, 8); return v; }
  for (zs_i32 i = 0; i < 8; ++i) {
    const zs_i32 b = byte + i;
    if (b >= 0 && (zs_u32)b < len) v |= (zs_u64)p[b] << (8 * i);
  }
  return v;
}
QH_ZS_HD int qh_zs_bits_init(qh_zs_bits* r, const zs_u8* p, zs_u32 len) {
  if (len < 1 || len > QH_ZSTD_BLOCK_MAX || p[len - 1] == 0) return QH_ZSTD_E_BITS;
  r->p = p; r->len = len;
  r->pos = (zs_i32)(8 * (len - 1) + qh_zs_bitlen(p[len - 1]) - 1);
  r->wbit = 0x40000000;   // (no window yet)
  r->win = 0;
  return QH_ZSTD_OK;
}
// the n (0 .. 32) bits below pos, not consumed
QH_ZS_HD zs_u32 qh_zs_peek(qh_zs_bits* r, zs_u32 n) {
  if (!n) return 0;
  const zs_i32 lo = r->pos - (zs_i32)n;
  if (lo < r->wbit || r->pos > r->wbit + 64) {
    // (pos may be far below 0 in a stream that underflowed: the window is then all zeros)
    zs_i32 top = r->pos < -64 ? -64 : r->pos;
    top = (top + 7) >> 3;   // (an arithmetic shift: floor)
    r->wbit = 8 * (top - 8);
    r->win = qh_zs_load64(r->p, r->len, top - 8);
    if (r->pos < -64) return 0;
  }
  return (zs_u32)((r->win >> (lo - r->wbit)) & ((1ull << n) - 1ull));
}
QH_ZS_HD zs_u32 qh_zs_read(qh_zs_bits* r, zs_u32 n) {
  const zs_u32 v = qh_zs_peek(r, n);
  r->pos -= (zs_i32)n;
  return v;
}

// 32 forward bits (least significant first) that begin at bit `bp` of p[0 .. avail): bytes behind avail read as zeros
QH_ZS_HD zs_u32 qh_zs_fwd(const zs_u8* p, zs_u32 avail, zs_u32 bp) {
  zs_u64 v = 0;
  const zs_u32 b = bp >> 3;
  for (zs_u32 i = 0; i < 5; ++i)
    if (b + i < avail) v |= (zs_u64)p[b + i] << (8 * i);
  return (zs_u32)(v >> (bp & 7u));
}

// ---------------------------------------------------------------- FSE
// The description at p[0 .. avail) of a distribution over at most `alphabet` symbols with an accuracy of at most max_al ->
// T->norm[0 .. *nsym), *al, *used bytes.
QH_ZS_HD int qh_zs_fse_read(const zs_u8* p, zs_u32 avail, zs_u32 max_al, zs_u32 alphabet, qh_zs_tables* T, zs_u32* al_out, zs_u32* nsym, zs_u32* used) {
  if (avail < 1) return QH_ZSTD_E_FSE;
  const zs_u32 al = (p[0] & 15u) + 5;
  if (al > max_al) return QH_ZSTD_E_FSE;
  zs_u32 bp = 4, sym = 0;
  zs_i32 remaining = (zs_i32)(1u << al);
  while (remaining > 0) {
    if (sym >= alphabet || bp > avail * 8) return QH_ZSTD_E_FSE;
    const zs_u32 max = (zs_u32)remaining + 1, nb = qh_zs_bitlen(max), low = (1u << nb) - 1 - max;
    const zs_u32 bits = qh_zs_fwd(p, avail, bp);
    zs_u32 v = bits & ((1u << (nb - 1)) - 1);
    if (v < low) bp += nb - 1;
    else {
      v = bits & ((1u << nb) - 1);
      bp += nb;
      if (v >= (1u << (nb - 1))) v -= low;
    }
    const zs_i32 prob = (zs_i32)v - 1;
    remaining -= prob < 0 ? 1 : prob;
    if (remaining < 0) return QH_ZSTD_E_FSE;
    T->norm[sym++] = (zs_i16)prob;
    if (prob == 0) {
      for (;;) {
        const zs_u32 rep = qh_zs_fwd(p, avail, bp) & 3u;
        bp += 2;
        if (sym + rep > alphabet) return QH_ZSTD_E_FSE;
        for (zs_u32 i = 0; i < rep; ++i) T->norm[sym++] = 0;
        if (rep != 3) break;
      }
    }
  }
  const zs_u32 bytes = (bp + 7) >> 3;
  if (bytes > avail) return QH_ZSTD_E_FSE;
  *al_out = al; *nsym = sym; *used = bytes;
  return QH_ZSTD_OK;
}

// T->norm[0 .. nsym) (sums to 2^al when -1 counts as 1) -> the decode table tab[0 .. 2^al)
QH_ZS_HD int qh_zs_fse_build(qh_zs_tables* T, zs_u32 nsym, zs_u32 al, zs_u32* tab) {
  const zs_u32 size = 1u << al, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
  zs_u32 high = size - 1, total = 0;
#pragma GCC unroll 1
  for (zs_u32 s = 0; s < nsym; ++s) {
    const zs_i32 n = T->norm[s];
    if (n == -1) { tab[high--] = s; T->next[s] = 1; total += 1; }
    else { T->next[s] = (zs_u16)n; total += (zs_u32)n; }
  }
  if (total != size) return QH_ZSTD_E_FSE;
  zs_u32 pos = 0;
#pragma GCC unroll 1
  for (zs_u32 s = 0; s < nsym; ++s) {
    const zs_i32 n = T->norm[s];
    for (zs_i32 i = 0; i < n; ++i) {
      tab[pos] = s;
      do pos = (pos + step) & mask; while (pos > high);
    }
  }
  if (pos != 0) return QH_ZSTD_E_FSE;
#pragma GCC unroll 1
  for (zs_u32 i = 0; i < size; ++i) {
    const zs_u32 s = tab[i], x = T->next[s];
    T->next[s] = (zs_u16)(x + 1);
    const zs_u32 nbits = al - (qh_zs_bitlen(x) - 1), base = (x << nbits) - size;
    tab[i] = s | nbits << 8 | base << 16;
  }
  return QH_ZSTD_OK;
}

QH_ZS_HD int qh_zs_fse_default(qh_zs_tables* T, const zs_i16* norm, zs_u32 nsym, zs_u32 al, zs_u32* tab) {
#pragma GCC unroll 1
  for (zs_u32 s = 0; s < nsym; ++s) T->norm[s] = norm[s];   // (not unrolled: 53 loads in flight would cost the kernel its registers)
  return qh_zs_fse_build(T, nsym, al, tab);
}

// One of the three tables of a sequences section. mode: 0 predefined, 1 RLE, 2 a description, 3 the table of the block before.
// *at: where the section's next byte lies in b[0 .. bs). which: 0 LL, 1 OF, 2 ML.
QH_ZS_HD int qh_zs_seq_table(zs_u32 which, zs_u32 mode, const zs_u8* b, zs_u32 bs, zs_u32* at, qh_zs_tables* T, zs_u32* al, zs_u32* have) {
  zs_u32* tab = which == 0 ? T->ll : which == 1 ? T->of : T->ml;
  const zs_u32 alphabet = which == 0 ? 36u : which == 1 ? 32u : 53u, max_al = which == 1 ? 8u : 9u;
  int bad = QH_ZSTD_OK;
  if (mode == 0) {
    if (which == 0) bad = qh_zs_fse_default(T, qh_zs_ll_default, 36, 6, tab);
    else if (which == 1) bad = qh_zs_fse_default(T, qh_zs_of_default, 29, 5, tab);
    else bad = qh_zs_fse_default(T, qh_zs_ml_default, 53, 6, tab);
    *al = which == 1 ? 5u : 6u;
  } else if (mode == 1) {
    if (*at >= bs) return QH_ZSTD_E_SEQUENCES;
    const zs_u32 s = b[*at];
    *at += 1;
    if (s >= alphabet) return QH_ZSTD_E_SEQUENCES;
    tab[0] = s;   // (one cell: no bits, the state stays 0)
    *al = 0;
  } else if (mode == 2) {
    zs_u32 nsym = 0, used = 0;
    bad = qh_zs_fse_read(b + *at, bs - *at, max_al, alphabet, T, al, &nsym, &used);
    if (bad) return bad;
    *at += used;
    bad = qh_zs_fse_build(T, nsym, *al, tab);
  } else {
    return *have ? QH_ZSTD_OK : QH_ZSTD_E_SEQUENCES;
  }
  if (!bad) *have = 1;
  return bad;
}

// ---------------------------------------------------------------- Huffman
// The tree description at p[0 .. avail) -> T->huf, *maxbits, *used bytes. The weights are direct 4-bit values or an FSE stream
// of two interleaved states; the last weight is implied.
QH_ZS_DEV int qh_zs_huf_read(const zs_u8* p, zs_u32 avail, qh_zs_tables* T, zs_u32 lane, zs_u32* maxbits_out, zs_u32* used) {
  (void)lane;
  if (avail < 1) return QH_ZSTD_E_HUFFMAN;
  const zs_u32 hb = p[0];
  zs_u32 n = 0;
  if (hb >= 128) {
    QH_ZS_FORM(QH_ZSF_WEIGHTS_DIRECT);
    n = hb - 127;
    const zs_u32 bytes = (n + 1) >> 1;
    if (1 + bytes > avail) return QH_ZSTD_E_HUFFMAN;
#pragma GCC unroll 1
    for (zs_u32 i = 0; i < n; ++i) {
      const zs_u32 v = p[1 + (i >> 1)];
      T->w[i] = (zs_u8)((i & 1u) ? (v & 15u) : (v >> 4));
    }
    *used = 1 + bytes;
  } else {
    QH_ZS_FORM(QH_ZSF_WEIGHTS_FSE);
    if (hb < 2 || 1 + hb > avail) return QH_ZSTD_E_HUFFMAN;
    zs_u32 al = 0, nsym = 0, d = 0;
    if (qh_zs_fse_read(p + 1, hb, 6, 12, T, &al, &nsym, &d)) return QH_ZSTD_E_HUFFMAN;
    if (qh_zs_fse_build(T, nsym, al, T->wt)) return QH_ZSTD_E_HUFFMAN;
    qh_zs_bits r;
    if (d >= hb || qh_zs_bits_init(&r, p + 1 + d, hb - d)) return QH_ZSTD_E_HUFFMAN;
    zs_u32 s1 = qh_zs_read(&r, al), s2 = qh_zs_read(&r, al);
    if (r.pos < 0) return QH_ZSTD_E_HUFFMAN;
    for (;;) {
      if (n >= 254) return QH_ZSTD_E_HUFFMAN;
      zs_u32 e = T->wt[s1];
      T->w[n++] = (zs_u8)(e & 255u);
      s1 = (e >> 16) + qh_zs_read(&r, (e >> 8) & 255u);
      if (r.pos < 0) { T->w[n++] = (zs_u8)(T->wt[s2] & 255u); break; }
      e = T->wt[s2];
      T->w[n++] = (zs_u8)(e & 255u);
      s2 = (e >> 16) + qh_zs_read(&r, (e >> 8) & 255u);
      if (r.pos < 0) { T->w[n++] = (zs_u8)(T->wt[s1] & 255u); break; }
    }
    *used = 1 + hb;
  }
  if (n > 255) return QH_ZSTD_E_HUFFMAN;   // (the implied weight follows: 256 symbols at the most)
  zs_u32 total = 0;
#pragma GCC unroll 1
  for (zs_u32 i = 0; i < 16; ++i) T->rank[i] = 0;
#pragma GCC unroll 1
  for (zs_u32 i = 0; i < n; ++i) {
    const zs_u32 w = T->w[i];
    if (w > 11) return QH_ZSTD_E_HUFFMAN;
    if (w) { total += 1u << (w - 1); T->rank[w] = T->rank[w] + 1; }
  }
  if (total == 0) return QH_ZSTD_E_HUFFMAN;
  const zs_u32 maxbits = qh_zs_bitlen(total);
  if (maxbits > 11) return QH_ZSTD_E_HUFFMAN;
  const zs_u32 rest = (1u << maxbits) - total;
  if (rest & (rest - 1)) return QH_ZSTD_E_HUFFMAN;
  const zs_u32 wl = qh_zs_bitlen(rest);   // log2(rest) + 1
  T->w[n++] = (zs_u8)wl;
  T->rank[wl] = T->rank[wl] + 1;
  // rank[w] becomes the first cell of weight w: ascending weight, 2^(w-1) cells per symbol
  zs_u32 cell = 0;
#pragma GCC unroll 1
  for (zs_u32 w = 1; w <= 11; ++w) {
    const zs_u32 c = T->rank[w];
    T->rank[w] = cell;
    cell += c << (w - 1);
  }
#pragma GCC unroll 1
  for (zs_u32 s = 0; s < n; ++s) {
    const zs_u32 w = T->w[s];
    if (!w) continue;
    const zs_u32 first = T->rank[w], cells = 1u << (w - 1);
    const zs_u16 e = (zs_u16)(s | (maxbits + 1 - w) << 8);
    T->rank[w] = first + cells;
    QH_ZS_LANES(l) for (zs_u32 j = l; j < cells; j += 64) T->huf[first + j] = e;
  }
  *maxbits_out = maxbits;
  return QH_ZSTD_OK;
}

// n bytes from s to d, which may overlap where d <= s: strides of 256 in ascending order, four loads in flight per lane, and the
// lanes of a stride all load before any of them stores, so a stride never reads what it or an earlier one stored.
QH_ZS_DEV void qh_zs_copy(zs_u8* d, const zs_u8* s, zs_u32 n, zs_u32 lane) {
  (void)lane;
  for (zs_u32 i0 = 0; i0 < n; i0 += 256) {
    zs_u8 got[4 * QH_ZS_NL] = {0};
    QH_ZS_LANES(l) {
#pragma GCC unroll 4
      for (zs_u32 k = 0; k < 4; ++k) if (i0 + 64 * k + l < n) got[4 * QH_ZS_SLOT(l) + k] = s[i0 + 64 * k + l];
    }
    QH_ZS_LANES(l) {
#pragma GCC unroll 4
      for (zs_u32 k = 0; k < 4; ++k) if (i0 + 64 * k + l < n) d[i0 + 64 * k + l] = got[4 * QH_ZS_SLOT(l) + k];
    }
  }
}

// ---------------------------------------------------------------- the walk
// One frame src[0 .. n_in), whose header the host has checked (qh_zstd_check_frame: the blocks begin at `start`), into
// dst[0 .. n_out). T: the tables, this wavefront's own.
//
// Literals are consumed where they lie: raw literals in the input, an RLE byte as it is. Huffman literals are decoded, four
// lanes to four streams, into the tail of the page's own slot, dst[n_out - L, n_out): before that L <= n_out - op is checked,
// and every sequence is checked to leave op <= (n_out - L) + the literals consumed, which in a sound stream is the match bytes
// and blocks still to come and stands for the check against the slot's end. A literal run then moves forward onto or below
// itself in ascending strides whose lanes all load before they store.
// A match takes 64 bytes per step, byte l of a step at op from op - offset + (l mod offset): bytes that earlier steps stored,
// read back from global memory under the rule k_pq_unsnap rests on (same-wavefront program order; the fence keeps the compiler
// to it). So dst is neither const nor restrict.
QH_ZS_DEV zs_u32 qh_zstd_frame(const zs_u8* src, zs_u32 n_in, zs_u32 start, zs_u8* dst, zs_u32 n_out, qh_zs_tables* T, zs_u32 lane) {
  (void)lane;
  zs_u32 ip = start, op = 0;
  zs_u32 rep0 = 1, rep1 = 4, rep2 = 8;
  zs_u32 have_huf = 0, huf_bits = 0, have_ll = 0, have_of = 0, have_ml = 0, al_ll = 0, al_of = 0, al_ml = 0;
  if (ip > n_in) return QH_ZSTD_E_BLOCK;
  QH_ZS_LANES(l) {
    if (l < 36) T->llc[l] = qh_zs_ll_code[l];
    if (l < 53) T->mlc[l] = qh_zs_ml_code[l];
  }
  QH_ZS_FENCE();
  for (;;) {
    if (n_in - ip < 3) return QH_ZSTD_E_BLOCK;
    const zs_u32 h = (zs_u32)src[ip] | (zs_u32)src[ip + 1] << 8 | (zs_u32)src[ip + 2] << 16;
    const zs_u32 type = (h >> 1) & 3u, bs = h >> 3;
    ip += 3;
    if (type == 3 || bs > QH_ZSTD_BLOCK_MAX) return QH_ZSTD_E_BLOCK;
    QH_ZS_FORM(QH_ZSF_BLOCK + type);
    if (type == 0) {
      if (bs > n_in - ip) return QH_ZSTD_E_BLOCK;
      if (bs > n_out - op) return QH_ZSTD_E_OUTPUT;
      qh_zs_copy(dst + op, src + ip, bs, lane);
      ip += bs; op += bs;
    } else if (type == 1) {
      if (1 > n_in - ip) return QH_ZSTD_E_BLOCK;
      if (bs > n_out - op) return QH_ZSTD_E_OUTPUT;
      const zs_u8 v = src[ip];
      QH_ZS_LANES(l) for (zs_u32 i = l; i < bs; i += 64) dst[op + i] = v;
      ip += 1; op += bs;
    } else {
      if (bs > n_in - ip) return QH_ZSTD_E_BLOCK;
      const zs_u8* b = src + ip;
      ip += bs;
      // ---- the literals section
      if (bs < 1) return QH_ZSTD_E_LITERALS;
      const zs_u32 lt = b[0] & 3u, sf = (b[0] >> 2) & 3u;
      QH_ZS_FORM(QH_ZSF_LIT + lt);
      zs_u32 L = 0, at = 0;          // regenerated size; where the sequences section begins
      const zs_u8* lit = b;          // raw: the literals in the input
      zs_u32 lit_rle = 0;
      if (lt < 2) {
        const zs_u32 hdr = sf == 1 ? 2u : sf == 3 ? 3u : 1u;
        if (hdr > bs) return QH_ZSTD_E_LITERALS;
        L = hdr == 1 ? (zs_u32)b[0] >> 3 : hdr == 2 ? ((zs_u32)b[0] >> 4) + ((zs_u32)b[1] << 4) : ((zs_u32)b[0] >> 4) + ((zs_u32)b[1] << 4) + ((zs_u32)b[2] << 12);
        if (L > QH_ZSTD_BLOCK_MAX) return QH_ZSTD_E_LITERALS;
        const zs_u32 body = lt == 0 ? L : 1u;
        if (body > bs - hdr) return QH_ZSTD_E_LITERALS;
        lit = b + hdr;
        if (lt == 1) lit_rle = b[hdr];
        at = hdr + body;
        if (L > n_out - op) return QH_ZSTD_E_OUTPUT;
      } else {
        const zs_u32 hdr = sf < 2 ? 3u : sf + 2, nb = sf < 2 ? 10u : sf == 2 ? 14u : 18u;
        if (hdr > bs) return QH_ZSTD_E_LITERALS;
        zs_u64 v = 0;
        for (zs_u32 i = 0; i < hdr; ++i) v |= (zs_u64)b[i] << (8 * i);
        v >>= 4;
        L = (zs_u32)(v & ((1u << nb) - 1));
        const zs_u32 comp = (zs_u32)((v >> nb) & ((1u << nb) - 1));
        if (L > QH_ZSTD_BLOCK_MAX || comp > bs - hdr) return QH_ZSTD_E_LITERALS;
        if (L > n_out - op) return QH_ZSTD_E_OUTPUT;
        at = hdr + comp;
        zs_u32 tree = 0;
        if (lt == 2) {
          const int bad = qh_zs_huf_read(b + hdr, comp, T, lane, &huf_bits, &tree);
          if (bad) return (zs_u32)bad;
          have_huf = 1;
        } else if (!have_huf) return QH_ZSTD_E_HUFFMAN;
        const zs_u8* sb = b + hdr + tree;
        const zs_u32 sl = comp - tree, nstreams = sf == 0 ? 1u : 4u;
        QH_ZS_FORM(sf == 0 ? QH_ZSF_STREAMS1 : QH_ZSF_STREAMS4);
        zs_u32 s1 = 0, s2 = 0, s3 = 0, seg = L;
        if (nstreams == 4) {
          if (sl < 6) return QH_ZSTD_E_LITERALS;
          s1 = (zs_u32)sb[0] | (zs_u32)sb[1] << 8; s2 = (zs_u32)sb[2] | (zs_u32)sb[3] << 8; s3 = (zs_u32)sb[4] | (zs_u32)sb[5] << 8;
          if (s1 + s2 + s3 > sl - 6) return QH_ZSTD_E_LITERALS;
          seg = (L + 3) >> 2;
          if (3 * seg > L) return QH_ZSTD_E_LITERALS;
        }
        // (the tables are complete before a lane reads them, the tail of the slot holds nothing yet that is needed)
        QH_ZS_FENCE();
        zs_u8* tail = dst + (n_out - L);
        const zs_u32 mask_bits = huf_bits;
        zs_u32 bad_bits = 0;
        QH_ZS_LANES(l) {
          if (l < nstreams) {
            zs_u32 from = 0, len = sl, first = 0, count = L;
            if (nstreams == 4) {
              from = 6 + (l > 0 ? s1 : 0u) + (l > 1 ? s2 : 0u) + (l > 2 ? s3 : 0u);
              len = l == 0 ? s1 : l == 1 ? s2 : l == 2 ? s3 : sl - 6 - s1 - s2 - s3;
              first = l * seg;
              count = l == 3 ? L - 3 * seg : seg;
            }
            qh_zs_bits r;
            if (qh_zs_bits_init(&r, sb + from, len)) bad_bits |= 1u;
            else {
              for (zs_u32 i = 0; i < count && r.pos >= 0; ++i) {
                const zs_u32 e = T->huf[qh_zs_peek(&r, mask_bits)];
                r.pos -= (zs_i32)(e >> 8);
                tail[first + i] = (zs_u8)e;
              }
              if (r.pos != 0) bad_bits |= 1u;
            }
          }
        }
        if (QH_ZS_ANY(bad_bits)) return QH_ZSTD_E_BITS;
        lit = tail;
        QH_ZS_FENCE();
      }
      const zs_u32 lb = n_out - L;   // op may not pass lb + the literals consumed
      zs_u32 lc = 0;
      // ---- the sequences section
      if (at >= bs) return QH_ZSTD_E_SEQUENCES;
      zs_u32 nseq = b[at++];
      if (nseq >= 128) {
        if (nseq < 255) {
          if (at >= bs) return QH_ZSTD_E_SEQUENCES;
          nseq = ((nseq - 128) << 8) + b[at++];
        } else {
          if (bs - at < 2) return QH_ZSTD_E_SEQUENCES;
          QH_ZS_FORM(QH_ZSF_COUNT3);
          nseq = (zs_u32)b[at] + ((zs_u32)b[at + 1] << 8) + 0x7F00u;
          at += 2;
        }
      }
      if (nseq == 0) {
        if (at != bs) return QH_ZSTD_E_SEQUENCES;
      } else {
        if (at >= bs) return QH_ZSTD_E_SEQUENCES;
        const zs_u32 modes = b[at++];
        if (modes & 3u) return QH_ZSTD_E_SEQUENCES;
        QH_ZS_FORM(QH_ZSF_LL + (modes >> 6));
        QH_ZS_FORM(QH_ZSF_OF + ((modes >> 4) & 3u));
        QH_ZS_FORM(QH_ZSF_ML + ((modes >> 2) & 3u));
        int bad = qh_zs_seq_table(0, modes >> 6, b, bs, &at, T, &al_ll, &have_ll);
        if (!bad) bad = qh_zs_seq_table(1, (modes >> 4) & 3u, b, bs, &at, T, &al_of, &have_of);
        if (!bad) bad = qh_zs_seq_table(2, (modes >> 2) & 3u, b, bs, &at, T, &al_ml, &have_ml);
        if (bad) return (zs_u32)bad;
        qh_zs_bits r;
        if (at > bs || qh_zs_bits_init(&r, b + at, bs - at)) return QH_ZSTD_E_BITS;
        zs_u32 st_ll = qh_zs_read(&r, al_ll), st_of = qh_zs_read(&r, al_of), st_ml = qh_zs_read(&r, al_ml);
        if (r.pos < 0) return QH_ZSTD_E_BITS;
        for (zs_u32 q = 0; q < nseq; ++q) {
          const zs_u32 e_ll = T->ll[st_ll], e_of = T->of[st_of], e_ml = T->ml[st_ml];
          const zs_u32 of_code = e_of & 255u, c_ml = T->mlc[e_ml & 255u], c_ll = T->llc[e_ll & 255u];
          const zs_u32 ov = (1u << of_code) + qh_zs_read(&r, of_code);
          const zs_u32 mlen = (c_ml & 0xFFFFFFu) + qh_zs_read(&r, c_ml >> 24);
          const zs_u32 llen = (c_ll & 0xFFFFFFu) + qh_zs_read(&r, c_ll >> 24);
          if (q + 1 < nseq) {
            st_ll = (e_ll >> 16) + qh_zs_read(&r, (e_ll >> 8) & 255u);
            st_ml = (e_ml >> 16) + qh_zs_read(&r, (e_ml >> 8) & 255u);
            st_of = (e_of >> 16) + qh_zs_read(&r, (e_of >> 8) & 255u);
          }
          if (r.pos < 0) return QH_ZSTD_E_BITS;
          zs_u32 offset;
          if (ov > 3) { offset = ov - 3; rep2 = rep1; rep1 = rep0; rep0 = offset; }
          else {
            const zs_u32 idx = ov - 1 + (llen == 0 ? 1u : 0u);
            QH_ZS_FORM(QH_ZSF_REP + idx);
            if (llen == 0) QH_ZS_FORM(QH_ZSF_LL0);
            if (idx == 0) offset = rep0;
            else {
              offset = idx == 1 ? rep1 : idx == 2 ? rep2 : rep0 - 1;
              if (offset == 0) return QH_ZSTD_E_OFFSET;
              if (idx != 1) rep2 = rep1;
              rep1 = rep0; rep0 = offset;
            }
          }
          // before a byte of the sequence is read or written
          if (llen > L - lc) return QH_ZSTD_E_SEQUENCES;
          if (op + mlen > lb + lc) return QH_ZSTD_E_OUTPUT;   // (op <= n_out < 2^31, mlen < 2^18: no overflow)
          if (offset > op + llen) return QH_ZSTD_E_OFFSET;
          if (llen) {
            if (lt == 1) { QH_ZS_LANES(l) for (zs_u32 i = l; i < llen; i += 64) dst[op + i] = (zs_u8)lit_rle; }
            else {
              qh_zs_copy(dst + op, lit + lc, llen, lane);
            }
            op += llen; lc += llen;
            QH_ZS_FENCE();
          }
          for (zs_u32 m0 = 0; m0 < mlen; m0 += 64) {
            const zs_u32 n = mlen - m0 < 64 ? mlen - m0 : 64u, from = op - offset;
            zs_u8 got[QH_ZS_NL] = {0};
            if (offset >= 64) { QH_ZS_LANES(l) if (l < n) got[QH_ZS_SLOT(l)] = dst[from + l]; }
            else { QH_ZS_LANES(l) if (l < n) got[QH_ZS_SLOT(l)] = dst[from + l % offset]; }
            QH_ZS_LANES(l) if (l < n) dst[op + l] = got[QH_ZS_SLOT(l)];
            op += n;
            QH_ZS_FENCE();
          }
        }
        if (r.pos != 0) return QH_ZSTD_E_BITS;
      }
      // ---- the literals behind the last sequence (op + L - lc <= n_out: the sequences kept op <= lb + lc)
      const zs_u32 rest = L - lc;
      if (rest) {
        if (lt == 1) { QH_ZS_LANES(l) for (zs_u32 i = l; i < rest; i += 64) dst[op + i] = (zs_u8)lit_rle; }
        else {
          qh_zs_copy(dst + op, lit + lc, rest, lane);
        }
        op += rest;
      }
    }
    QH_ZS_FENCE();
    if (h & 1u) break;
  }
  return op != n_out ? (zs_u32)QH_ZSTD_E_OUTPUT : (zs_u32)QH_ZSTD_OK;
}

#endif  // QHIP_ZSTD_INC
