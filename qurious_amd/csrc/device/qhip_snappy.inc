// qhip_snappy.inc — the token code of the device Snappy decoder (kernels_parquet.hip k_pq_unsnap; parquet_meta.hpp, parquet.cpp;
// DESIGN §3.9, format level 2): the preamble reader, the size checks the host makes before anything is allocated, the element
// parser, the checks that come before an element's bytes are touched, and the source index of one lane of a copy.
//
// One text for two compilers, as qhip_parquet.inc is: included by kernels_parquet.hip for hipcc and, as plain host C++, by
// parquet_meta.hpp and tests/cpp/parquet_snappy_tests.cpp, where loops stand for the lanes. Self-contained: builtin integer
// types only, no #include. A raw Snappy stream is a ULEB128 preamble (the uncompressed length) and then elements, each a tag
// byte whose low two bits say what follows:
//   00 literal   length - 1 in the tag's upper six bits when below 60; 60..63: in the 1..4 bytes behind the tag, little-endian
//   01 copy      length 4..11 in bits 2..4, offset = bits 5..7 << 8 | the next byte
//   10 copy      length 1..64 in the upper six bits, a 2-byte little-endian offset
//   11 copy      the same with a 4-byte offset
// A copy repeats `length` bytes that begin `offset` bytes behind the output position; with offset < length it overlaps itself.
// Every length and offset is untrusted.
#ifndef QHIP_SNAPPY_INC
#define QHIP_SNAPPY_INC
#ifndef QH_PQ_HD
#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define QH_PQ_HD __host__ __device__
#else
#define QH_PQ_HD
#endif
#endif

typedef unsigned char sn_u8;
typedef unsigned int sn_u32;
typedef unsigned long long sn_u64;

// why a stream is refused (the Parquet reasons QH_PQ_R_SNAPPY_* are QH_PQ_R_SNAPPY_BASE + these)
#define QH_SNAP_OK 0
#define QH_SNAP_E_PREAMBLE 1   // the preamble does not end in 5 bytes, exceeds 32 bits, or is not the declared uncompressed size
#define QH_SNAP_E_SIZE 2       // the declared size exceeds 64/3 times the compressed size: no stream expands further
#define QH_SNAP_E_INPUT 3      // an element's bytes reach past the input; the input ends with output missing, or goes on behind a full output
#define QH_SNAP_E_OUTPUT 4     // a literal or copy reaches past the declared size
#define QH_SNAP_E_OFFSET 5     // a copy offset of 0, or one beyond the bytes produced so far
#define QH_SNAP_E_COUNT 6

#define QH_SNAP_LITERAL 0u
#define QH_SNAP_COPY 1u

typedef struct qh_snap_elem {
  sn_u64 len;      // bytes the element produces: literal 1 .. 2^32, copy 1 .. 64
  sn_u64 offset;   // copy: how far behind the output position its source begins (unchecked); literal: 0
  sn_u32 kind;     // QH_SNAP_LITERAL / QH_SNAP_COPY
  sn_u32 header;   // bytes of the tag and its length or offset bytes: 1 .. 5
} qh_snap_elem;

// The preamble at s[0 ..): nothing read at or behind s[len]. Returns the bytes consumed (1..5), 0 when it does not end in
// time or does not fit 32 bits.
QH_PQ_HD inline int qh_snap_preamble(const sn_u8* s, sn_u64 len, sn_u32* out) {
  sn_u32 v = 0;
  for (int i = 0; i < 5; ++i) {
    if ((sn_u64)i >= len) return 0;
    const sn_u32 b = s[i];
    if (i == 4 && b > 0x0Fu) return 0;
    v |= (b & 0x7Fu) << (7 * i);
    if (!(b & 0x80u)) { *out = v; return i + 1; }
  }
  return 0;
}

// What the host checks of a stream s[0 .. len) before it reserves `declared` bytes for its output: the preamble ends and says
// `declared`, and `declared` is no more than Snappy can make of len bytes (a 3-byte copy element yields at most 64 bytes).
// *start: where the elements begin.
QH_PQ_HD inline int qh_snap_check_sizes(const sn_u8* s, sn_u64 len, sn_u64 declared, sn_u32* start) {
  sn_u32 n = 0;
  const int used = qh_snap_preamble(s, len, &n);
  if (!used || (sn_u64)n != declared) return QH_SNAP_E_PREAMBLE;
  if (declared * 3 > len * 64) return QH_SNAP_E_SIZE;   // (both below 2^32: no overflow)
  *start = (sn_u32)used;
  return QH_SNAP_OK;
}

// The element whose tag is p[0]; `avail` (>= 1) bytes of input begin at p and nothing at or behind p[avail] is read.
// QH_SNAP_OK, or QH_SNAP_E_INPUT when the tag's length or offset bytes are cut off.
QH_PQ_HD inline int qh_snap_element(const sn_u8* p, sn_u64 avail, qh_snap_elem* e) {
  const sn_u32 tag = p[0], top = tag >> 2;
  sn_u32 extra;   // bytes behind the tag
  switch (tag & 3u) {
    case 0: extra = top < 60 ? 0 : top - 59; break;
    case 1: extra = 1; break;
    case 2: extra = 2; break;
    default: extra = 4; break;
  }
  if ((sn_u64)extra + 1 > avail) return QH_SNAP_E_INPUT;
  sn_u64 v = 0;
  for (sn_u32 i = 0; i < extra; ++i) v |= (sn_u64)p[1 + i] << (8 * i);
  e->header = extra + 1;
  if ((tag & 3u) == 0) { e->kind = QH_SNAP_LITERAL; e->len = (top < 60 ? (sn_u64)top : v) + 1; e->offset = 0; }
  else if ((tag & 3u) == 1) { e->kind = QH_SNAP_COPY; e->len = 4 + (top & 7u); e->offset = ((sn_u64)(tag >> 5) << 8) | v; }
  else { e->kind = QH_SNAP_COPY; e->len = (sn_u64)top + 1; e->offset = v; }
  return QH_SNAP_OK;
}

// Before any byte of the element is read or written: in_left input bytes lie behind its header, `op` bytes of the `out_size`
// are produced (op <= out_size).
QH_PQ_HD inline int qh_snap_check(const qh_snap_elem* e, sn_u64 in_left, sn_u64 op, sn_u64 out_size) {
  if (e->kind == QH_SNAP_LITERAL) { if (e->len > in_left) return QH_SNAP_E_INPUT; }
  else if (e->offset == 0 || e->offset > op) return QH_SNAP_E_OFFSET;
  if (e->len > out_size - op) return QH_SNAP_E_OUTPUT;
  return QH_SNAP_OK;
}

// Where byte `lane` (< length) of a copy at output position op comes from. One rule for plain and overlapping copies: the
// source pattern is the `offset` bytes in front of op, repeated — every index it names is below op, so all lanes of a copy
// read bytes that earlier elements stored and none that this copy stores.
QH_PQ_HD inline sn_u64 qh_snap_copy_src(sn_u64 op, sn_u64 offset, sn_u32 lane) { return op - offset + ((sn_u64)lane % offset); }

#endif  // QHIP_SNAPPY_INC
