// qhip_delta.inc — DELTA_BINARY_PACKED as the device Parquet decoder reads it (encoding set 2: kernels_parquet.hip k_pq_delta,
// DESIGN §3.9): the stream header, a block header, the geometry and width checks and the bit extraction of one delta.
//
// A stream is: ULEB128 block size, miniblocks per block, total count; a zigzag first value; then blocks of a zigzag min delta,
// one bit-width byte per miniblock and the miniblocks, each (values per miniblock) deltas bit-packed little-endian at its width.
// Value k is first + the sum of (min delta + packed delta) over its predecessors, in wrapping arithmetic of the type's width.
// The last miniblock that holds a value is stored whole; the miniblocks behind it are not stored and their width bytes mean nothing.
//
// One text for two compilers, as device/qhip_parquet.inc (which is included first): the kernel calls these functions in every
// lane, tests/cpp/parquet_encodings_tests.cpp calls them from loops that stand for the lanes, under the sanitizers. Every
// count and width is untrusted; each function says which bytes it reads.
#ifndef QHIP_DELTA_INC
#define QHIP_DELTA_INC

#define QH_DL_MAX_BLOCK 65536u

typedef struct qh_dl_head {
  pq_u64 first;      // the first value (zigzag decoded), to be truncated to the type's width
  pq_u64 end;        // bytes of the header: where the first block begins
  pq_u32 block;      // values per block
  pq_u32 mpb;        // miniblocks per block
  pq_u32 vpm;        // values per miniblock: a multiple of 32
  pq_u32 total;      // values of the stream, the first one included
} qh_dl_head;

// ULEB128 of a u64 at s[pos ..), nothing read at or behind s[len]. Returns the bytes consumed; 0 when it does not end.
QH_PQ_HD inline int qh_dl_varint(const pq_u8* s, pq_u64 len, pq_u64 pos, pq_u64* out) {
  pq_u64 v = 0;
  for (int i = 0; i < 10; ++i) {
    if (pos + (pq_u64)i >= len) return 0;
    const pq_u64 b = s[pos + (pq_u64)i];
    if (i == 9 && b > 1u) return 0;
    v |= (b & 0x7Fu) << (7 * i);
    if (!(b & 0x80u)) { *out = v; return i + 1; }
  }
  return 0;
}
// why a varint at pos did not end: the stream ended first, or ten bytes did not do
QH_PQ_HD inline int qh_dl_varint_reason(pq_u64 len, pq_u64 pos) { return pos > len || len - pos < 10 ? QH_PQ_R_DELTA_SHORT : QH_PQ_R_DELTA_VARINT; }

QH_PQ_HD inline pq_u64 qh_dl_zigzag(pq_u64 z) { return (z >> 1) ^ (0ull - (z & 1ull)); }

// The header of the stream s[0 .. len). QH_PQ_OK or a reason; reads nothing behind s[len - 1].
QH_PQ_HD inline int qh_dl_header(const pq_u8* s, pq_u64 len, qh_dl_head* h) {
  pq_u64 pos = 0, block = 0, mpb = 0, total = 0, first = 0;
  int used = qh_dl_varint(s, len, pos, &block);
  if (!used) return qh_dl_varint_reason(len, pos);
  pos += (pq_u64)used;
  used = qh_dl_varint(s, len, pos, &mpb);
  if (!used) return qh_dl_varint_reason(len, pos);
  pos += (pq_u64)used;
  used = qh_dl_varint(s, len, pos, &total);
  if (!used) return qh_dl_varint_reason(len, pos);
  pos += (pq_u64)used;
  used = qh_dl_varint(s, len, pos, &first);
  if (!used) return qh_dl_varint_reason(len, pos);
  pos += (pq_u64)used;
  if (block == 0 || (block & 127u)) return QH_PQ_R_DELTA_GEOMETRY;
  if (block > QH_DL_MAX_BLOCK) return QH_PQ_R_DELTA_LARGE;
  if (mpb == 0 || mpb > block || block % mpb) return QH_PQ_R_DELTA_GEOMETRY;
  if ((block / mpb) & 31u) return QH_PQ_R_DELTA_GEOMETRY;
  if (total > 0xFFFFFFFFull) return QH_PQ_R_DELTA_COUNT;
  h->first = qh_dl_zigzag(first); h->end = pos;
  h->block = (pq_u32)block; h->mpb = (pq_u32)mpb; h->vpm = (pq_u32)(block / mpb); h->total = (pq_u32)total;
  return QH_PQ_OK;
}

// The block header at s[pos ..): the min delta, then mpb width bytes at *widths_at (all inside the stream), the first miniblock
// at *data_at <= len.
QH_PQ_HD inline int qh_dl_block(const pq_u8* s, pq_u64 len, pq_u64 pos, pq_u32 mpb, pq_u64* min_delta, pq_u64* widths_at, pq_u64* data_at) {
  pq_u64 z = 0;
  const int used = qh_dl_varint(s, len, pos, &z);
  if (!used) return qh_dl_varint_reason(len, pos);
  pos += (pq_u64)used;
  if ((pq_u64)mpb > len - pos) return QH_PQ_R_DELTA_SHORT;
  *min_delta = qh_dl_zigzag(z); *widths_at = pos; *data_at = pos + (pq_u64)mpb;
  return QH_PQ_OK;
}

// A miniblock that holds a value: its width w against the type's bits, its vpm / 8 * w bytes against the `avail` bytes left.
QH_PQ_HD inline int qh_dl_miniblock(pq_u32 w, pq_u32 bits, pq_u32 vpm, pq_u64 avail) {
  if (w > bits) return QH_PQ_R_DELTA_WIDTH;
  if ((pq_u64)(vpm >> 3) * w > avail) return QH_PQ_R_DELTA_SHORT;
  return QH_PQ_OK;
}

// delta k (k < vpm) of the miniblock whose bytes begin at d: w (0..64) bits at bit k * w. Reads at most 9 bytes, all of the miniblock.
QH_PQ_HD inline pq_u64 qh_dl_extract(const pq_u8* d, pq_u64 k, pq_u32 w) {
  if (!w) return 0;
  const pq_u64 bit = k * w, b = bit >> 3;
  const pq_u32 sh = (pq_u32)(bit & 7u), nb = (sh + w + 7u) >> 3;
  pq_u64 v = 0;
  for (pq_u32 i = 0; i < nb && i < 8; ++i) v |= (pq_u64)d[b + i] << (8 * i);
  v >>= sh;
  if (nb == 9) v |= (pq_u64)d[b + 8] << (64 - sh);   // (nb == 9 only with sh > 0)
  if (w < 64) v &= (1ull << w) - 1ull;
  return v;
}

#endif  // QHIP_DELTA_INC
