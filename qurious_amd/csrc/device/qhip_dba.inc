// qhip_dba.inc — DELTA_BYTE_ARRAY as the device Parquet decoder reads it (the DELTA_BYTE_ARRAY switch: kernels_parquet.hip
// k_pq_delta and k_pq_dba_fill, DESIGN §3.9): the checks of a value's prefix and suffix length and the source rule of the fill.
//
// A page's values region is a DELTA_BINARY_PACKED stream of prefix lengths, a second one of suffix lengths that begins where
// the first ends, and the suffix bytes. Value k is the first prefix[k] bytes of value k - 1 followed by its suffix[k] bytes;
// Arrow's writer and reader reset "the value before" at every page, so a page's first prefix is 0 and a page whose first
// prefix is not (the writers of PARQUET-246) is not decoded here.
//
// One text for two compilers, as device/qhip_delta.inc (device/qhip_parquet.inc is included first): the kernels call these
// functions in every lane, tests/cpp/parquet_dba_tests.cpp calls them from loops that stand for the lanes. Every length is
// untrusted.
#ifndef QHIP_DBA_INC
#define QHIP_DBA_INC

// a prefix length as the first stream holds it: the page's first one is 0, none is negative
QH_PQ_HD inline int qh_dba_check_prefix(pq_u32 prefix, bool first) {
  if (first ? prefix != 0u : (int)prefix < 0) return QH_PQ_R_DBA_PREFIX;
  return QH_PQ_OK;
}

// value k > 0 once its suffix length is known: prefix (checked above) against prev_len, the length of value k - 1; the value's
// length against 2^31 - 1 and, where flba is not 0, against the column's width. The first value is checked with prev_len 0.
QH_PQ_HD inline int qh_dba_check_value(pq_u32 prefix, pq_u32 suffix, pq_u32 prev_len, pq_u32 flba) {
  if ((int)suffix < 0) return QH_PQ_R_DBA_SUFFIX;
  if (prefix > prev_len) return QH_PQ_R_DBA_PREFIX;
  if ((pq_u64)prefix + suffix > 0x7FFFFFFFull) return QH_PQ_R_DBA_SUFFIX;
  if (flba && prefix + suffix != flba) return QH_PQ_R_DBA_WIDTH;
  return QH_PQ_OK;
}

// the suffix bytes of a page, `sum` of them, against the `avail` bytes behind the second stream
QH_PQ_HD inline int qh_dba_check_total(pq_u64 sum, pq_u64 avail) { return sum > avail ? QH_PQ_R_DBA_SUFFIX : QH_PQ_OK; }

// The fill, 64 rows per step, lane = row. Byte j < prefix[r] of row r is byte j of the nearest earlier non-NULL row k of the
// page with prefix[k] <= j, where it is a suffix byte. `mask`: the ballot of "non-NULL and prefix <= j" over the step. Returns
// the highest lane below `lane` in it, or -1: then the byte is byte j of the last non-NULL row of the steps before.
QH_PQ_HD inline int qh_dba_source_lane(pq_u64 mask, int lane) {
  const pq_u64 below = mask & ((1ull << lane) - 1ull);
  return below ? 63 - __builtin_clzll(below) : -1;
}

// a step whose longest prefix is above this walks its rows in order, the wavefront copying each prefix 64 bytes per trip
#define QH_DBA_STEP_PREFIX 64u

#endif  // QHIP_DBA_INC
