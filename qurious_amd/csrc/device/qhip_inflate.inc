// qhip_inflate.inc — the device DEFLATE decoder (kernels_parquet.hip k_pq_ungzip; parquet_meta.hpp, parquet.cpp; DESIGN §3.9,
// the gzip switch): a complete decoder of one gzip member (RFC 1952) around one DEFLATE stream (RFC 1951). The member-header
// check the host makes before anything is reserved (qh_gzip_check_member); the forward bit reader; the cooperative builder of a
// canonical Huffman code's decode tables; the code-length reader of a dynamic block with its repeat codes; the symbol walk
// (qh_inflate_member) over stored, fixed and dynamic blocks, and every check that comes before an access.
//
// One text for two compilers, as qhip_zstd.inc is: included by kernels_parquet.hip for hipcc and, as plain host C++, by
// parquet_meta.hpp and tests/cpp/parquet_gzip_tests.cpp. Self-contained: builtin integer types only, no #include. The walk is
// wave-uniform: every lane parses the same bits and follows the same symbols. Where the lanes differ the text says
// QH_INFL_LANES(l): the lane's own index for hipcc, a loop over 64 lanes for a host compiler.
//
// A code's tables (qh_infl_tables, LDS on the device): a primary table indexed by the next 10 (literal/length) or 9 (distance)
// bits, whose cell says what the symbol means, and for longer codes the canonical description — per length the first code, the
// count and where the length's symbols begin in a list sorted by (length, symbol). The builder spreads its work over the lanes:
// lane L counts and places the symbols of length L, then the lanes take a symbol each and fill its cells.
//
// All lengths, counts and distances are untrusted. Positions inside a page fit 32 bits. The member's CRC32 is skipped, not
// verified. The 32 KB window is not enforced: a distance may reach back to the page's first byte and never behind it.
#ifndef QHIP_INFLATE_INC
#define QHIP_INFLATE_INC

typedef unsigned char infl_u8;
typedef unsigned short infl_u16;
typedef unsigned int infl_u32;
typedef int infl_i32;
typedef unsigned long long infl_u64;

#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define QH_INFL_HD __host__ __device__ __forceinline__
#define QH_INFL_DEV __device__ __forceinline__
#define QH_INFL_LANES(l) for (infl_u32 l = lane, qh_infl_once = 1; qh_infl_once; qh_infl_once = 0)
#define QH_INFL_NL 1
#define QH_INFL_SLOT(l) 0
#define QH_INFL_PUT(arr, idx, v) do { if (lane == (idx)) (arr)[0] = (v); } while (0)
#define QH_INFL_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")
#else
#define QH_INFL_HD static inline
#define QH_INFL_DEV static inline
#define QH_INFL_LANES(l) for (infl_u32 l = 0; l < 64; ++l)
#define QH_INFL_NL 64
#define QH_INFL_SLOT(l) (l)
#define QH_INFL_PUT(arr, idx, v) ((arr)[idx] = (v))
#define QH_INFL_FENCE() ((void)0)
#endif
#ifndef QH_INFL_FORM   // (the CPU test records which forms of the format a stream used)
#define QH_INFL_FORM(bit) ((void)0)
#endif

// why a member is refused (the Parquet reasons QH_PQ_R_GZIP_* are QH_PQ_R_GZIP_BASE + these)
#define QH_INFL_OK 0
#define QH_INFL_E_MEMBER 1      // the member header: magic, CM, a reserved FLG bit, an optional field cut off, no room for a body and the trailer
#define QH_INFL_E_SIZE 2        // ISIZE against the declared size mod 2^32, or a declared size above 1032 x the body's bytes
#define QH_INFL_E_BLOCK 3       // a block header: BTYPE 3, or a stored block whose LEN and NLEN do not match
#define QH_INFL_E_LENGTHS 4     // the code lengths of a dynamic block: HLIT above 286, HDIST above 30, a code-length code that is over-subscribed or incomplete, a repeat with no previous length or past the count
#define QH_INFL_E_CODE 5        // a literal/length or distance code that is over-subscribed or incomplete, or has no end-of-block code
#define QH_INFL_E_SYMBOL 6      // bits that are no code of an incomplete code, literal/length symbol 286 or 287, distance symbol 30 or 31
#define QH_INFL_E_DISTANCE 7    // a distance of 0, or one beyond the bytes produced
#define QH_INFL_E_OUTPUT 8      // output past the declared size, or a final block that ends with output missing
#define QH_INFL_E_INPUT 9       // the input ends inside a block header, a code length, a symbol or a stored block
#define QH_INFL_E_TRAILER 10    // bytes between the end of the final block, byte aligned, and the trailer: a second member among the rest
#define QH_INFL_E_COUNT 11

// the forms of the format (QH_INFL_FORM)
#define QH_INFLF_BTYPE 0       // + block type 0..2
#define QH_INFLF_REPEAT 3      // + code-length symbol 16..18 - 16
#define QH_INFLF_LEN258 6      // a match of the longest length
#define QH_INFLF_DIST32K 7     // a distance of 32768
#define QH_INFLF_LONG 8        // a code longer than its primary table's width
#define QH_INFLF_COUNT 9

#define QH_INFL_LIT_BITS 10u
#define QH_INFL_DIST_BITS 9u
#define QH_INFL_CL_BITS 7u

// A cell: value | code length << 16 | extra bits << 20 | type << 24. value: the literal, the base of a length or distance, the
// code-length symbol. A code length of 0: no code of the primary width begins with these bits.
#define QH_INFL_T_LITERAL 0u
#define QH_INFL_T_BASE 1u
#define QH_INFL_T_END 2u
#define QH_INFL_T_BAD 3u

// the canonical description of one code
typedef struct qh_infl_code {
  infl_u16 count[16], first[16], offs[16];
} qh_infl_code;

// The tables of one page, in LDS on the device (7 316 bytes). The 7-bit table of a dynamic block's code-length code is done
// with before the literal/length table is filled and lies in its first cells, its description in `lc`.
typedef struct qh_infl_tables {
  infl_u32 lit[1u << QH_INFL_LIT_BITS];
  infl_u32 dist[1u << QH_INFL_DIST_BITS];
  infl_u16 lit_sorted[288], dist_sorted[32];
  qh_infl_code lc, dc;
  infl_u8 lens[320];   // literal/length lengths, the distance lengths right behind them
  infl_u8 cl[20];
} qh_infl_tables;

// the order in which a dynamic block gives the lengths of the code-length code
static const infl_u8 qh_infl_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---------------------------------------------------------------- the host's part: before anything is reserved
// The member at s[0 .. len) that is to fill `declared` bytes: its header with the optional fields, room for a body and the
// trailer, ISIZE, and the bound on what the body can produce (a length/distance pair takes at least 2 bits and yields at most
// 258 bytes). *start: where the first DEFLATE block begins. A zlib (RFC 1950) wrapper fails at the magic.
QH_INFL_HD int qh_gzip_check_member(const infl_u8* s, infl_u64 len, infl_u64 declared, infl_u32* start) {
  if (len < 10 || len > 0x7FFFFFFFull) return QH_INFL_E_MEMBER;
  if (s[0] != 0x1F || s[1] != 0x8B || s[2] != 8 || (s[3] & 0xE0u)) return QH_INFL_E_MEMBER;
  const infl_u32 flg = s[3];
  infl_u64 at = 10;
  if (flg & 4u) {   // FEXTRA
    if (len - at < 2) return QH_INFL_E_MEMBER;
    const infl_u64 xlen = (infl_u64)s[at] | (infl_u64)s[at + 1] << 8;
    at += 2;
    if (xlen > len - at) return QH_INFL_E_MEMBER;
    at += xlen;
  }
  for (infl_u32 bit = 8u; bit <= 16u; bit <<= 1) {   // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    for (;;) {
      if (at >= len) return QH_INFL_E_MEMBER;
      if (s[at++] == 0) break;
    }
  }
  if (flg & 2u) {   // FHCRC
    if (len - at < 2) return QH_INFL_E_MEMBER;
    at += 2;
  }
  if (len - at < 9) return QH_INFL_E_MEMBER;
  const infl_u64 body = len - at - 8;
  const infl_u32 isize = (infl_u32)s[len - 4] | (infl_u32)s[len - 3] << 8 | (infl_u32)s[len - 2] << 16 | (infl_u32)s[len - 1] << 24;
  if (isize != (infl_u32)(declared & 0xFFFFFFFFull)) return QH_INFL_E_SIZE;
  if (declared > 1032ull * body) return QH_INFL_E_SIZE;
  *start = (infl_u32)at;
  return QH_INFL_OK;
}

// ---------------------------------------------------------------- bits
// A forward bit stream over p[0 .. end), least significant bit first. win holds nbits unread bits (and, above them, bits of the
// bytes that follow, which the next refill ors in again); ip: the first byte not yet counted in nbits; ahead: the 8 bytes at
// ip, loaded when ip was set, so that a refill waits for no load of its own. Bytes behind `end` read as zeros: the walk asks
// qh_infl_past() before it follows what it read. Between two refills at most 56 bits are taken.
typedef struct qh_infl_bits {
  const infl_u8* p;
  infl_u32 end, ip, nbits;
  infl_u64 win, ahead;
} qh_infl_bits;

QH_INFL_HD infl_u64 qh_infl_load64(const infl_u8* p, infl_u32 end, infl_u32 at) {
  infl_u64 v = 0;
  if (at <= end && end - at >= 8) { __builtin_memcpy(&v, p + at, 8); return v; }
  for (infl_u32 i = 0; i < 8; ++i)
    if (at + i < end) v |= (infl_u64)p[at + i] << (8 * i);
  return v;
}
QH_INFL_HD void qh_infl_bits_at(qh_infl_bits* r, infl_u32 at) {
  r->ip = at; r->nbits = 0; r->win = 0;
  r->ahead = qh_infl_load64(r->p, r->end, at);
}
QH_INFL_HD void qh_infl_refill(qh_infl_bits* r) {
  r->win |= r->ahead << r->nbits;
  r->ip += (63u - r->nbits) >> 3;
  r->nbits |= 56u;
  r->ahead = qh_infl_load64(r->p, r->end, r->ip);
}
QH_INFL_HD infl_u32 qh_infl_take(qh_infl_bits* r, infl_u32 n) {   // n <= 16
  const infl_u32 v = (infl_u32)r->win & ((1u << n) - 1u);
  r->win >>= n;
  r->nbits -= n;
  return v;
}
// whether bits behind the input's end have been taken
QH_INFL_HD int qh_infl_past(const qh_infl_bits* r) { return r->ip > r->end + (r->nbits >> 3); }

QH_INFL_HD infl_u32 qh_infl_rev16(infl_u32 x) {   // the 16 low bits, reversed
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bitreverse32(x) >> 16;
#else
  x = (x & 0x5555u) << 1 | (x >> 1 & 0x5555u);
  x = (x & 0x3333u) << 2 | (x >> 2 & 0x3333u);
  x = (x & 0x0F0Fu) << 4 | (x >> 4 & 0x0F0Fu);
  return (x & 0x00FFu) << 8 | (x >> 8 & 0x00FFu);
#endif
}

// ---------------------------------------------------------------- tables
// what symbol `sym` of a code of kind 0 (code lengths), 1 (literal/length) or 2 (distance) means, as a cell
QH_INFL_HD infl_u32 qh_infl_cell(infl_u32 kind, infl_u32 sym, infl_u32 len) {
  const infl_u32 l = len << 16;
  if (kind == 0) return sym | l;
  if (kind == 1) {
    if (sym < 256) return sym | l;
    if (sym == 256) return l | QH_INFL_T_END << 24;
    if (sym > 285) return l | QH_INFL_T_BAD << 24;
    if (sym == 285) return 258u | l | QH_INFL_T_BASE << 24;
    const infl_u32 i = sym - 257;
    if (i < 8) return (3u + i) | l | QH_INFL_T_BASE << 24;
    const infl_u32 eb = (i >> 2) - 1;
    return (3u + ((4u + (i & 3u)) << eb)) | l | eb << 20 | QH_INFL_T_BASE << 24;
  }
  if (sym > 29) return l | QH_INFL_T_BAD << 24;
  if (sym < 4) return (1u + sym) | l | QH_INFL_T_BASE << 24;
  const infl_u32 eb = (sym >> 1) - 1;
  return (1u + ((2u + (sym & 1u)) << eb)) | l | eb << 20 | QH_INFL_T_BASE << 24;
}

// lens[0 .. n) (each 0 .. 15) -> the code's description c, its symbols sorted by (length, symbol), and the primary table
// tab[0 .. 2^tbits). Returns 0, 1 for an over-subscribed code, 2 for an incomplete one (whose tables are built all the same:
// the bits that are no code find no cell); *maxlen: the longest length.
QH_INFL_DEV int qh_infl_build(const infl_u8* lens, infl_u32 n, infl_u32 kind, infl_u32* tab, infl_u32 tbits, infl_u16* sorted, qh_infl_code* c, infl_u32 lane,
                              infl_u32* maxlen) {
  (void)lane;
  // lane L counts the symbols of length L
  QH_INFL_LANES(l) {
    if (l < 16) {
      infl_u32 k = 0;
      if (l)
        for (infl_u32 s = 0; s < n; ++s) k += lens[s] == l ? 1u : 0u;
      c->count[l] = (infl_u16)k;
    }
  }
  QH_INFL_FENCE();
  infl_i32 left = 1;
  infl_u32 code = 0, off = 0, mx = 0;
#pragma GCC unroll 1
  for (infl_u32 len = 1; len <= 15; ++len) {
    const infl_u32 cnt = c->count[len];
    left = 2 * left - (infl_i32)cnt;
    if (left < 0) return 1;
    c->first[len] = (infl_u16)code;   // (at most 2^len, as left >= 0)
    c->offs[len] = (infl_u16)off;
    code = (code + cnt) << 1;
    off += cnt;
    if (cnt) mx = len;
  }
  *maxlen = mx;
  QH_INFL_FENCE();
  // lane L places the symbols of length L; the lanes clear the primary table
  QH_INFL_LANES(l) {
    if (l >= 1 && l < 16) {
      infl_u32 o = c->offs[l];
      for (infl_u32 s = 0; s < n; ++s)
        if (lens[s] == l) sorted[o++] = (infl_u16)s;
    }
    for (infl_u32 e = l; e < (1u << tbits); e += 64) tab[e] = 0;
  }
  QH_INFL_FENCE();
  // a symbol per lane: its code, bit-reversed as the stream holds it, and every cell whose low bits are that code
  QH_INFL_LANES(l) {
    for (infl_u32 i = l; i < off; i += 64) {
      const infl_u32 sym = sorted[i], len = lens[sym];
      if (len > tbits) continue;
      const infl_u32 cd = (infl_u32)c->first[len] + (i - (infl_u32)c->offs[len]);
      const infl_u32 cell = qh_infl_cell(kind, sym, len);
      for (infl_u32 k = qh_infl_rev16(cd) >> (16 - len); k < (1u << tbits); k += 1u << len) tab[k] = cell;
    }
  }
  QH_INFL_FENCE();
  return left > 0 ? 2 : 0;
}

// the symbol of a code longer than the primary table's width, which the next 15 bits `bits` begin with: the cell, or one of
// type BAD and length 0 when they begin no code
QH_INFL_HD infl_u32 qh_infl_long(infl_u32 bits, infl_u32 kind, infl_u32 tbits, const infl_u16* sorted, const qh_infl_code* c) {
  const infl_u32 rev = qh_infl_rev16(bits & 0x7FFFu) >> 1;   // 15 bits, the first of the stream on top
#pragma GCC unroll 1
  for (infl_u32 len = tbits + 1; len <= 15; ++len) {
    const infl_u32 d = (rev >> (15 - len)) - (infl_u32)c->first[len];
    if (d < (infl_u32)c->count[len]) {
      QH_INFL_FORM(QH_INFLF_LONG);
      return qh_infl_cell(kind, sorted[(infl_u32)c->offs[len] + d], len);
    }
  }
  return QH_INFL_T_BAD << 24;
}

// ---------------------------------------------------------------- the walk
// One member src[0 .. n_in), whose header the host has checked (qh_gzip_check_member: the DEFLATE stream begins at `start`, the
// last 8 bytes are the trailer), into dst[0 .. n_out). T: the tables, this wavefront's own.
//
// Literals are gathered, the k-th pending one in lane k, and stored together, up to 64 at a time: when 64 are pending, and
// before a match or the end of a block. A match takes 64 bytes per step, byte l of a step at op from op - distance + (l mod
// distance): bytes that earlier steps or the literals' store wrote, read back from global memory under the rule k_pq_unsnap
// rests on (same-wavefront program order; the fence keeps the compiler to it). So dst is neither const nor restrict.
QH_INFL_DEV infl_u32 qh_inflate_member(const infl_u8* src, infl_u32 n_in, infl_u32 start, infl_u8* dst, infl_u32 n_out, qh_infl_tables* T, infl_u32 lane) {
  (void)lane;
  if (start > n_in || n_in - start < 9) return QH_INFL_E_MEMBER;
  qh_infl_bits r;
  r.p = src; r.end = n_in - 8;
  qh_infl_bits_at(&r, start);
  infl_u32 op = 0, np = 0, fixed_built = 0;
  infl_u8 pend[QH_INFL_NL] = {0};
  for (;;) {
    qh_infl_refill(&r);
    const infl_u32 hdr = qh_infl_take(&r, 3), type = hdr >> 1;
    if (qh_infl_past(&r)) return QH_INFL_E_INPUT;
    if (type == 3) return QH_INFL_E_BLOCK;
    QH_INFL_FORM(QH_INFLF_BTYPE + type);
    if (type == 0) {
      // ---- a stored block: LEN and NLEN at the next byte boundary, then the bytes, spread over the lanes
      (void)qh_infl_take(&r, r.nbits & 7u);
      const infl_u32 pos = r.ip - (r.nbits >> 3);
      if (pos > r.end || r.end - pos < 4) return QH_INFL_E_INPUT;
      const infl_u32 len = (infl_u32)src[pos] | (infl_u32)src[pos + 1] << 8, nlen = (infl_u32)src[pos + 2] | (infl_u32)src[pos + 3] << 8;
      if ((len ^ nlen) != 0xFFFFu) return QH_INFL_E_BLOCK;
      if (len > r.end - pos - 4) return QH_INFL_E_INPUT;
      if (len > n_out - op) return QH_INFL_E_OUTPUT;
      QH_INFL_LANES(l) for (infl_u32 i = l; i < len; i += 64) dst[op + i] = src[pos + 4 + i];
      op += len;
      qh_infl_bits_at(&r, pos + 4 + len);
    } else {
      if (type == 1) {
        // ---- the fixed code: built once per member at the most
        if (!fixed_built) {
          QH_INFL_LANES(l) {
            for (infl_u32 s = l; s < 288; s += 64) T->lens[s] = (infl_u8)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            if (l < 32) T->lens[288 + l] = 5;
          }
          QH_INFL_FENCE();
          infl_u32 mx = 0;
          (void)qh_infl_build(T->lens, 288, 1, T->lit, QH_INFL_LIT_BITS, T->lit_sorted, &T->lc, lane, &mx);
          (void)qh_infl_build(T->lens + 288, 32, 2, T->dist, QH_INFL_DIST_BITS, T->dist_sorted, &T->dc, lane, &mx);
          fixed_built = 1;
        }
      } else {
        // ---- a dynamic block: the code-length code, then the lengths of both codes as one list
        fixed_built = 0;
        const infl_u32 hlit = qh_infl_take(&r, 5) + 257, hdist = qh_infl_take(&r, 5) + 1, hclen = qh_infl_take(&r, 4) + 4;
        if (qh_infl_past(&r)) return QH_INFL_E_INPUT;
        if (hlit > 286 || hdist > 30) return QH_INFL_E_LENGTHS;
        QH_INFL_LANES(l) if (l < 19) T->cl[l] = 0;
        QH_INFL_FENCE();
#pragma GCC unroll 1
        for (infl_u32 i = 0; i < hclen; ++i) {
          qh_infl_refill(&r);
          T->cl[qh_infl_cl_order[i]] = (infl_u8)qh_infl_take(&r, 3);
        }
        if (qh_infl_past(&r)) return QH_INFL_E_INPUT;
        QH_INFL_FENCE();
        infl_u32 mx = 0;
        if (qh_infl_build(T->cl, 19, 0, T->lit, QH_INFL_CL_BITS, T->lit_sorted, &T->lc, lane, &mx)) return QH_INFL_E_LENGTHS;
        const infl_u32 n = hlit + hdist;
        infl_u32 i = 0, prev = 0;
        while (i < n) {
          qh_infl_refill(&r);
          const infl_u32 e = T->lit[(infl_u32)r.win & ((1u << QH_INFL_CL_BITS) - 1u)], sym = e & 31u;
          if (!(e >> 16)) return QH_INFL_E_LENGTHS;   // (a complete code leaves no such cell)
          (void)qh_infl_take(&r, e >> 16);
          if (sym < 16) {
            T->lens[i++] = (infl_u8)sym;
            prev = sym;
          } else {
            QH_INFL_FORM(QH_INFLF_REPEAT + sym - 16);
            infl_u32 rep, v = 0;
            if (sym == 16) {
              if (i == 0) return QH_INFL_E_LENGTHS;
              v = prev;
              rep = 3 + qh_infl_take(&r, 2);
            } else if (sym == 17) rep = 3 + qh_infl_take(&r, 3);
            else rep = 11 + qh_infl_take(&r, 7);
            if (rep > n - i) return QH_INFL_E_LENGTHS;
            QH_INFL_LANES(l) for (infl_u32 j = l; j < rep; j += 64) T->lens[i + j] = (infl_u8)v;
            i += rep;
            prev = v;
          }
          if (qh_infl_past(&r)) return QH_INFL_E_INPUT;
        }
        QH_INFL_FENCE();
        if (T->lens[256] == 0) return QH_INFL_E_CODE;
        if (qh_infl_build(T->lens, hlit, 1, T->lit, QH_INFL_LIT_BITS, T->lit_sorted, &T->lc, lane, &mx)) return QH_INFL_E_CODE;
        const int bad = qh_infl_build(T->lens + hlit, hdist, 2, T->dist, QH_INFL_DIST_BITS, T->dist_sorted, &T->dc, lane, &mx);
        // (zlib's one allowance: a distance code of a single code of length 1, or of none, may be incomplete)
        if (bad == 1 || (bad == 2 && mx > 1)) return QH_INFL_E_CODE;
      }
      // ---- the symbols of the block
      for (;;) {
        qh_infl_refill(&r);
        infl_u32 e = T->lit[(infl_u32)r.win & ((1u << QH_INFL_LIT_BITS) - 1u)];
        if (!(e >> 16 & 15u)) e = qh_infl_long((infl_u32)r.win, 1, QH_INFL_LIT_BITS, T->lit_sorted, &T->lc);
        infl_u32 kind = e >> 24;
        if (kind == QH_INFL_T_BAD) return qh_infl_past(&r) ? QH_INFL_E_INPUT : QH_INFL_E_SYMBOL;
        (void)qh_infl_take(&r, e >> 16 & 15u);
        if (kind == QH_INFL_T_LITERAL) {
          if (qh_infl_past(&r)) return QH_INFL_E_INPUT;
          if (np >= n_out - op) return QH_INFL_E_OUTPUT;
          QH_INFL_PUT(pend, np, (infl_u8)e);
          if (++np == 64) {
            QH_INFL_LANES(l) dst[op + l] = pend[QH_INFL_SLOT(l)];
            op += 64; np = 0;
          }
          continue;
        }
        if (np) {   // before anything may read them, and at the end of the block
          QH_INFL_LANES(l) if (l < np) dst[op + l] = pend[QH_INFL_SLOT(l)];
          op += np; np = 0;
          QH_INFL_FENCE();
        }
        if (kind == QH_INFL_T_END) {
          if (qh_infl_past(&r)) return QH_INFL_E_INPUT;
          break;
        }
        const infl_u32 mlen = (e & 0xFFFFu) + qh_infl_take(&r, e >> 20 & 15u);
        infl_u32 d = T->dist[(infl_u32)r.win & ((1u << QH_INFL_DIST_BITS) - 1u)];
        if (!(d >> 16 & 15u)) d = qh_infl_long((infl_u32)r.win, 2, QH_INFL_DIST_BITS, T->dist_sorted, &T->dc);
        kind = d >> 24;
        if (kind == QH_INFL_T_BAD) return qh_infl_past(&r) ? QH_INFL_E_INPUT : QH_INFL_E_SYMBOL;
        (void)qh_infl_take(&r, d >> 16 & 15u);
        const infl_u32 distance = (d & 0xFFFFu) + qh_infl_take(&r, d >> 20 & 15u);
        // before a byte of the match is read or written
        if (qh_infl_past(&r)) return QH_INFL_E_INPUT;
        if (distance == 0 || distance > op) return QH_INFL_E_DISTANCE;
        if (mlen > n_out - op) return QH_INFL_E_OUTPUT;
        if (mlen == 258) QH_INFL_FORM(QH_INFLF_LEN258);
        if (distance == 32768) QH_INFL_FORM(QH_INFLF_DIST32K);
        for (infl_u32 m0 = 0; m0 < mlen; m0 += 64) {
          const infl_u32 cnt = mlen - m0 < 64 ? mlen - m0 : 64u, from = op - distance;
          infl_u8 got[QH_INFL_NL] = {0};
          if (distance >= 64) { QH_INFL_LANES(l) if (l < cnt) got[QH_INFL_SLOT(l)] = dst[from + l]; }
          else { QH_INFL_LANES(l) if (l < cnt) got[QH_INFL_SLOT(l)] = dst[from + l % distance]; }
          QH_INFL_LANES(l) if (l < cnt) dst[op + l] = got[QH_INFL_SLOT(l)];
          op += cnt;
          QH_INFL_FENCE();
        }
      }
    }
    if (hdr & 1u) break;
  }
  // ---- behind the final block: nothing but the rest of its last byte, then the trailer
  if (op != n_out) return QH_INFL_E_OUTPUT;
  if (r.ip - (r.nbits >> 3) != r.end) return QH_INFL_E_TRAILER;
  return QH_INFL_OK;
}

#endif  // QHIP_INFLATE_INC
