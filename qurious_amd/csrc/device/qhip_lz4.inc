// qhip_lz4.inc — the device LZ4 block decoder of the lz4 switch (kernels_parquet.hip k_pq_unlz4; parquet_meta.hpp, parquet.cpp;
// DESIGN §3.9): the size check the host makes before anything is reserved, the rule that tells Hadoop's length frames from a
// bare block, and the whole block decoder.
//
// One text for two compilers, as qhip_snappy.inc and qhip_inflate.inc are: included by kernels_parquet.hip for hipcc and, as
// plain host C++, by parquet_meta.hpp and tests/cpp/parquet_lz4_tests.cpp. Self-contained: builtin integer types only, no
// #include. QH_LZ4_LANES(l): the lane's own index for hipcc, a loop over 64 lanes for a host compiler.
//
// An LZ4 block is a run of sequences. A token byte opens each: its high nibble is the literal length, its low nibble the match
// length minus 4; a nibble of 15 is extended by the bytes that follow, each added, until one is below 255. Behind the token and
// the literal length's extension lie the literals, then a 2-byte little-endian offset, then the match length's extension. A
// match repeats bytes that begin `offset` bytes behind the output position; with offset < length it overlaps itself. The last
// sequence ends after its literals. Every length and offset is untrusted.
//
// What is accepted. A block is accepted when every sequence stays inside input and output and the input and the output end
// together behind a literal run (which may be empty: a last token of 0). The encoder-side end-of-block restrictions — the last
// 5 bytes are literals, the last match begins at least 12 bytes before the end — are NOT enforced: they bind a compressor, and
// a decoder that checks every access is safe without them. A block that ends behind a match is refused. A declared size of 0
// is accepted with the one-byte block 00 (what liblz4 and pa.Codec("lz4_raw").compress(b"") emit) and with no input at all;
// no input with a declared size above 0 is refused.
#ifndef QHIP_LZ4_INC
#define QHIP_LZ4_INC
#ifndef QH_PQ_HD
#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define QH_PQ_HD __host__ __device__
#else
#define QH_PQ_HD
#endif
#endif

#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define QH_LZ4_DEV __device__ __forceinline__
#define QH_LZ4_LANES(l) for (lz4_u32 l = lane, qh_lz4_once = 1; qh_lz4_once; qh_lz4_once = 0)
#define QH_LZ4_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")
#else
#define QH_LZ4_DEV static inline
#define QH_LZ4_LANES(l) for (lz4_u32 l = 0; l < 64; ++l)
#define QH_LZ4_FENCE() ((void)0)
#endif
// (a byte every lane read from the same LDS cell is one value: saying so keeps the walk's positions and lengths in scalar
// registers and its branches scalar)
#if defined(__HIP_DEVICE_COMPILE__)
#define QH_LZ4_SYNC() __syncthreads()
#define QH_LZ4_UNIFORM(x) ((lz4_u32)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define QH_LZ4_SYNC() ((void)0)
#define QH_LZ4_UNIFORM(x) ((lz4_u32)(x))
#endif
#ifndef QH_LZ4_FORM   // (the CPU test records which forms of the format a block used)
#define QH_LZ4_FORM(bit) ((void)0)
#endif

typedef unsigned char lz4_u8;
typedef unsigned int lz4_u32;
typedef unsigned long long lz4_u64;

// why a block is refused (the Parquet reasons QH_PQ_R_LZ4_* are QH_PQ_R_LZ4_BASE + these)
#define QH_LZ4_OK 0
#define QH_LZ4_E_SIZE 1      // the declared size exceeds 255 times the compressed size: no block expands further
#define QH_LZ4_E_FRAME 2     // Hadoop framing: the frames tile the page, but one has no bytes for the output it declares
#define QH_LZ4_E_CUT 3       // the input ends inside a length's extension or an offset
#define QH_LZ4_E_LITERAL 4   // a literal run reaches past the input
#define QH_LZ4_E_OUTPUT 5    // a literal run or a match reaches past the declared size
#define QH_LZ4_E_OFFSET 6    // a match offset of 0, or one beyond the bytes produced so far
#define QH_LZ4_E_END 7       // input left behind a full output; the input ends with output missing, or behind a match
#define QH_LZ4_E_COUNT 8

// the forms of the format (QH_LZ4_FORM)
#define QH_LZ4F_LITEXT 0     // a literal length of 15 or more: extended
#define QH_LZ4F_MATCHEXT 1   // a match length of 19 or more: extended
#define QH_LZ4F_OVERLAP 2    // a match that overlaps itself with an offset below 64
#define QH_LZ4F_FAR 3        // an offset of 64 or more
#define QH_LZ4F_LONG 4       // a match longer than 64 bytes
#define QH_LZ4F_LAST 5       // a final sequence without a match
#define QH_LZ4F_EMPTY 6      // the empty block: a declared size of 0
#define QH_LZ4F_COUNT 7

#define QH_LZ4_TILE 1024u    // bytes of input staged at a time (the kernel's LDS tile)

// What the host checks of a block of `len` bytes before it reserves `declared` bytes for its output: each input byte adds at
// most 255 output bytes (a byte of a length's extension), so no block expands more than 255 times. (both below 2^32)
QH_PQ_HD inline int qh_lz4_check_sizes(lz4_u64 len, lz4_u64 declared) { return declared > 255 * len ? QH_LZ4_E_SIZE : QH_LZ4_OK; }

QH_PQ_HD inline lz4_u32 qh_lz4_be32(const lz4_u8* p) { return ((lz4_u32)p[0] << 24) | ((lz4_u32)p[1] << 16) | ((lz4_u32)p[2] << 8) | (lz4_u32)p[3]; }

// The legacy codec id (Parquet's LZ4, 5). Hadoop writers put frames of BE32 uncompressed size, BE32 compressed size, block
// around the blocks; old Arrow writers wrote one bare block under the same id. Arrow's reader decompresses the frames and falls
// back to a bare block when that fails; here the host decides by arithmetic on what it can see without decompressing. The frame
// that begins at s[*pos]: 1 and its sizes when its 8 bytes and its block lie inside s[0 .. len), with *pos moved behind it; 0
// otherwise. Nothing at or behind s[len] is read.
QH_PQ_HD inline int qh_lz4_hadoop_next(const lz4_u8* s, lz4_u64 len, lz4_u64* pos, lz4_u32* usize, lz4_u32* csize) {
  if (*pos > len || len - *pos < 8) return 0;
  const lz4_u32 u = qh_lz4_be32(s + *pos), c = qh_lz4_be32(s + *pos + 4);
  if ((lz4_u64)c > len - *pos - 8) return 0;
  *usize = u; *csize = c; *pos += 8 + (lz4_u64)c;
  return 1;
}
// 1 when s[0 .. len) is Hadoop-framed: one frame or more tile it exactly and their uncompressed sizes add up to `declared`;
// *frames: how many. 0: one bare block. *bad (meaningful at 1): QH_LZ4_OK, or why a frame is refused before anything is
// reserved — QH_LZ4_E_FRAME for one without bytes that declares output, QH_LZ4_E_SIZE for one above the 255x bound.
// A bare block whose first bytes happen to tile is taken for frames; the decoder then refuses it, never decodes it wrongly
// without notice, and the page goes to the host path.
QH_PQ_HD inline int qh_lz4_hadoop_scan(const lz4_u8* s, lz4_u64 len, lz4_u64 declared, lz4_u32* frames, int* bad) {
  lz4_u64 pos = 0, sum = 0;
  lz4_u32 count = 0, u = 0, c = 0;
  int why = QH_LZ4_OK;
  while (pos < len) {
    if (!qh_lz4_hadoop_next(s, len, &pos, &u, &c)) return 0;
    sum += u;
    if (sum > declared) return 0;
    ++count;
    if (!why && c == 0 && u != 0) why = QH_LZ4_E_FRAME;
    if (!why) why = qh_lz4_check_sizes(c, u);
  }
  if (count == 0 || sum != declared) return 0;
  *frames = count; *bad = why;
  return 1;
}

// Where byte i (< length) of a match at output position op comes from: qh_snap_copy_src's rule. The source pattern is the
// `offset` bytes in front of op, repeated — every index it names is below op, so every byte of a match of any length is one that
// earlier sequences stored and none that this match stores. That holds for offset 1 and for offsets that do not divide 64.
QH_PQ_HD inline lz4_u32 qh_lz4_copy_src(lz4_u32 op, lz4_u32 offset, lz4_u32 i) { return op - offset + (i % offset); }

// Input byte ip (< n_in), through the tile: tile[0 .. QH_LZ4_TILE) holds src[*tbase ..] as far as the input goes. The walk
// only moves forward, so a byte outside the tile moves the tile: lane l takes bytes l, l + 64, ...
QH_LZ4_DEV lz4_u32 qh_lz4_fetch(const lz4_u8* src, lz4_u32 n_in, lz4_u8* tile, lz4_u32* tbase, lz4_u32 ip, lz4_u32 lane) {
  (void)lane;
  if (ip - *tbase >= QH_LZ4_TILE) {
    const lz4_u32 base = ip & ~63u;
    QH_LZ4_SYNC();
    QH_LZ4_LANES(l) for (lz4_u32 j = l; j < QH_LZ4_TILE; j += 64) if (base + j < n_in) tile[j] = src[base + j];
    QH_LZ4_SYNC();
    *tbase = base;
  }
  return QH_LZ4_UNIFORM(tile[ip - *tbase]);
}

// n bytes from s to d, spread over the lanes, four loads in flight per lane. s[0 .. n) holds nothing this call stores.
QH_LZ4_DEV void qh_lz4_spread(const lz4_u8* s, lz4_u8* d, lz4_u32 n, lz4_u32 lane) {
  (void)lane;
  QH_LZ4_LANES(l) for (lz4_u32 i = l; i < n; i += 256) {
    const bool h1 = i + 64 < n, h2 = i + 128 < n, h3 = i + 192 < n;
    const lz4_u8 b0 = s[i], b1 = h1 ? s[i + 64] : (lz4_u8)0, b2 = h2 ? s[i + 128] : (lz4_u8)0, b3 = h3 ? s[i + 192] : (lz4_u8)0;
    d[i] = b0;
    if (h1) d[i + 64] = b1;
    if (h2) d[i + 128] = b2;
    if (h3) d[i + 192] = b3;
  }
}

// One block: src[0 .. n_in) -> dst[0 .. n_out), n_in and n_out below 2^31. The walk over the sequences is wave-uniform — input
// position, output position, lengths and offset are the same in every lane; token, extension and offset bytes come through the
// tile (QH_LZ4_TILE bytes, the kernel's LDS). Literals and match bytes are spread over the lanes; a match of any length is
// copied 64 bytes per step and lane, its sources named by qh_lz4_copy_src, so no step reads what another step of the same match
// stores. Bytes other lanes stored are read back from memory under the same-wavefront rule k_pq_unsnap states; the fence per
// sequence keeps the compiler to program order. So dst is neither const nor restrict. Every check comes before the access it
// guards; a refused block leaves dst half written. Length extensions stop adding as soon as the sum exceeds what the input
// (literals) or the output (matches) has left, so no sum passes 2^31 + 255.
QH_LZ4_DEV lz4_u32 qh_lz4_block(const lz4_u8* src, lz4_u32 n_in, lz4_u8* dst, lz4_u32 n_out, lz4_u8* tile, lz4_u32 lane) {
  if (n_in == 0) {
    if (n_out) return QH_LZ4_E_END;
    QH_LZ4_FORM(QH_LZ4F_EMPTY);
    return QH_LZ4_OK;
  }
  lz4_u32 ip = 0, op = 0, tbase = n_in;   // (ip - tbase wraps to 2^31 or more: no tile yet)
  for (;;) {
    // ---- the token and the literal run (ip < n_in here)
    const lz4_u32 token = qh_lz4_fetch(src, n_in, tile, &tbase, ip++, lane);
    lz4_u32 lit = token >> 4;
    if (lit == 15) {
      QH_LZ4_FORM(QH_LZ4F_LITEXT);
      for (;;) {
        if (ip >= n_in) return QH_LZ4_E_CUT;
        const lz4_u32 b = qh_lz4_fetch(src, n_in, tile, &tbase, ip++, lane);
        lit += b;
        if (b != 255) break;
        if (ip < n_in && lit > n_in - ip) return QH_LZ4_E_LITERAL;   // (stop adding; at the input's end the extension is cut off)
      }
    }
    if (lit > n_in - ip) return QH_LZ4_E_LITERAL;
    if (lit > n_out - op) return QH_LZ4_E_OUTPUT;
    if (ip - tbase + lit <= QH_LZ4_TILE) {
      const lz4_u8* t = tile + (ip - tbase);
      QH_LZ4_LANES(l) for (lz4_u32 i = l; i < lit; i += 64) dst[op + i] = t[i];
    } else {
      qh_lz4_spread(src + ip, dst + op, lit, lane);
    }
    ip += lit; op += lit;
    QH_LZ4_FENCE();
    if (ip == n_in) {   // the last sequence ends after its literals
      if (op != n_out) return QH_LZ4_E_END;
      QH_LZ4_FORM(QH_LZ4F_LAST);
      if (n_out == 0) QH_LZ4_FORM(QH_LZ4F_EMPTY);
      return QH_LZ4_OK;
    }
    if (op == n_out) return QH_LZ4_E_END;   // (input left behind a full output)
    // ---- the match
    if (n_in - ip < 2) return QH_LZ4_E_CUT;
    const lz4_u32 lo = qh_lz4_fetch(src, n_in, tile, &tbase, ip, lane), hi = qh_lz4_fetch(src, n_in, tile, &tbase, ip + 1, lane);
    const lz4_u32 offset = lo | (hi << 8);
    ip += 2;
    lz4_u32 mlen = (token & 15u) + 4;
    if (mlen == 19) {
      QH_LZ4_FORM(QH_LZ4F_MATCHEXT);
      for (;;) {
        if (ip >= n_in) return QH_LZ4_E_CUT;
        const lz4_u32 b = qh_lz4_fetch(src, n_in, tile, &tbase, ip++, lane);
        mlen += b;
        if (b != 255) break;
        if (ip < n_in && mlen > n_out - op) return QH_LZ4_E_OUTPUT;   // (stop adding)
      }
    }
    if (offset == 0 || offset > op) return QH_LZ4_E_OFFSET;
    if (mlen > n_out - op) return QH_LZ4_E_OUTPUT;
    if (offset >= 64) QH_LZ4_FORM(QH_LZ4F_FAR);
    else if (offset < mlen) QH_LZ4_FORM(QH_LZ4F_OVERLAP);
    if (mlen > 64) QH_LZ4_FORM(QH_LZ4F_LONG);
    if (offset >= mlen) {
      qh_lz4_spread(dst + (op - offset), dst + op, mlen, lane);   // (i % offset is i: the source lies whole in front of op)
    } else {
      QH_LZ4_LANES(l) for (lz4_u32 i = l; i < mlen; i += 256) {
        const bool h1 = i + 64 < mlen, h2 = i + 128 < mlen, h3 = i + 192 < mlen;
        const lz4_u8 b0 = dst[qh_lz4_copy_src(op, offset, i)], b1 = h1 ? dst[qh_lz4_copy_src(op, offset, i + 64)] : (lz4_u8)0,
                     b2 = h2 ? dst[qh_lz4_copy_src(op, offset, i + 128)] : (lz4_u8)0, b3 = h3 ? dst[qh_lz4_copy_src(op, offset, i + 192)] : (lz4_u8)0;
        dst[op + i] = b0;
        if (h1) dst[op + i + 64] = b1;
        if (h2) dst[op + i + 128] = b2;
        if (h3) dst[op + i + 192] = b3;
      }
    }
    op += mlen;
    QH_LZ4_FENCE();
    if (ip == n_in) return QH_LZ4_E_END;   // (a block ends behind literals, never behind a match)
  }
}

#endif  // QHIP_LZ4_INC
