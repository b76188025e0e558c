// qhip_widekey.inc — per-row code of the wide-key encoding stage (agg.cpp maybe_encode_wide_key, kernels_rel.hip
// k_widekey_encode): a GROUP BY key of any width -> one 32-bit group code per row, exactly. The reference hashes keys of any
// length and any number of columns (utils/array.rs:171-210); the aggregate kernels pack a key into at most 8 words, so a wider
// key is replaced by its code in front of them.
//
// code[row] = the number of ONE row that carries the same key (the group's representative: whichever row of the group won the
// slot). An open-addressing table of 8-byte slots, (tag << 32) | (row + 1), 0 = empty, maps keys to representatives; a slot
// never changes once it is set, and what it names is input data written before the launch, so the slot word is the only word
// the workgroups exchange. No busy state, no spinning: a row that loses the compare-and-swap goes on with the winner's word.
//
// One text for two compilers: included by kernels_rel.hip for hipcc and, as plain host C++, by tests/cpp/widekey_tests.cpp
// (the insert loop single-threaded against a std::map). Self-contained: builtin integer types only, no #include. The slot
// accesses come in through the policy `A` (load / cas): agent-scope atomics on the device, plain accesses in the host test.
#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define QH_WK_HD __host__ __device__
#else
#define QH_WK_HD
#endif

#define QH_WK_MAX_COLS 32

// One key column (Arrow layout, plain and materialised). width = bytes per value (1, 2, 4, 8, 16), 0 = Utf8: v holds the
// int32 offsets (rows + 1 of them), d the bytes. Utf8 bytes are read 8 at a time: the buffer behind d carries >= 8 bytes of slack.
struct qh_wk_col {
  const void* v;
  const unsigned char* d;
  const unsigned char* n;   // validity bitmap (LSB order) or null
  unsigned width;
  unsigned pad;
};

typedef unsigned long long __attribute__((aligned(1))) qh_wk_u64_unaligned;

QH_WK_HD inline unsigned long long qh_wk_mix(unsigned long long x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33; return x;
}
QH_WK_HD inline bool qh_wk_valid(const qh_wk_col& c, unsigned row) { return !c.n || ((c.n[row >> 3] >> (row & 7)) & 1); }
// a fixed-width value of up to 8 bytes, zero-extended (equal bytes <=> equal words)
QH_WK_HD inline unsigned long long qh_wk_word(const qh_wk_col& c, unsigned row) {
  switch (c.width) {
    case 1: return ((const unsigned char*)c.v)[row];
    case 2: return ((const unsigned short*)c.v)[row];
    case 4: return ((const unsigned*)c.v)[row];
    default: return ((const unsigned long long*)c.v)[row];
  }
}
// bytes [8 w, 8 w + 8) of a Utf8 value of `len` bytes, the ones past its end zeroed
QH_WK_HD inline unsigned long long qh_wk_str_word(const unsigned char* p, unsigned len, unsigned w) {
  const unsigned long long raw = *(const qh_wk_u64_unaligned*)(p + 8 * w);
  const unsigned nb = len - 8 * w;   // (> 0 for every word the callers ask for)
  return nb >= 8 ? raw : raw & (~0ULL >> (64 - 8 * nb));
}

// 64-bit hash of the row's key: per column a null marker, or the value bytes (Utf8: the length, then the bytes)
QH_WK_HD inline unsigned long long qh_wk_hash(const qh_wk_col* cols, int ncols, unsigned row) {
  unsigned long long h = 0x243f6a8885a308d3ULL;
  for (int k = 0; k < ncols; ++k) {
    const qh_wk_col& c = cols[k];
    if (!qh_wk_valid(c, row)) { h = qh_wk_mix(h ^ 0x9e3779b97f4a7c15ULL); continue; }
    if (c.width == 0) {
      const int* off = (const int*)c.v;
      const unsigned o = (unsigned)off[row], len = (unsigned)off[row + 1] - o;
      h = qh_wk_mix(h ^ len);
      const unsigned nw = (len + 7) >> 3;
      for (unsigned w = 0; w < nw; ++w) h = qh_wk_mix(h ^ qh_wk_str_word(c.d + o, len, w));
    } else if (c.width == 16) {
      const unsigned long long* v = (const unsigned long long*)c.v + 2 * (unsigned long long)row;
      h = qh_wk_mix(qh_wk_mix(h ^ v[0]) ^ v[1]);
    } else {
      h = qh_wk_mix(h ^ qh_wk_word(c, row));
    }
  }
  return h;
}

// Column by column: NULL equals NULL, a NULL's value bytes are ignored, otherwise the bytes are compared exactly.
QH_WK_HD inline bool qh_wk_equal(const qh_wk_col* cols, int ncols, unsigned a, unsigned b) {
  for (int k = 0; k < ncols; ++k) {
    const qh_wk_col& c = cols[k];
    const bool va = qh_wk_valid(c, a), vb = qh_wk_valid(c, b);
    if (va != vb) return false;
    if (!va) continue;
    if (c.width == 0) {
      const int* off = (const int*)c.v;
      const unsigned oa = (unsigned)off[a], la = (unsigned)off[a + 1] - oa;
      const unsigned ob = (unsigned)off[b], lb = (unsigned)off[b + 1] - ob;
      if (la != lb) return false;
      const unsigned nw = (la + 7) >> 3;
      for (unsigned w = 0; w < nw; ++w)
        if (qh_wk_str_word(c.d + oa, la, w) != qh_wk_str_word(c.d + ob, la, w)) return false;
    } else if (c.width == 16) {
      const unsigned long long* v = (const unsigned long long*)c.v;
      if (v[2 * (unsigned long long)a] != v[2 * (unsigned long long)b] || v[2 * (unsigned long long)a + 1] != v[2 * (unsigned long long)b + 1]) return false;
    } else if (qh_wk_word(c, a) != qh_wk_word(c, b)) {
      return false;
    }
  }
  return true;
}

// The row's group code. table: slot_mask + 1 slots (a power of two, at least twice the rows: never full), zeroed before the
// first row. hash_mask: all ones; fewer bits only to force collisions (tests). A::load(p) reads a slot, A::cas(p, desired)
// sets an EMPTY slot and returns what the slot held before (0 = this row won it).
template <class A>
QH_WK_HD inline unsigned qh_wk_insert(const qh_wk_col* cols, int ncols, unsigned long long* table, unsigned slot_mask,
                                      unsigned long long hash_mask, unsigned row) {
  const unsigned long long h = qh_wk_hash(cols, ncols, row) & hash_mask;
  const unsigned tag = (unsigned)(h >> 32);
  const unsigned long long mine = ((unsigned long long)tag << 32) | (unsigned long long)(row + 1u);
  unsigned s = (unsigned)h & slot_mask;
  for (;;) {
    unsigned long long cur = A::load(table + s);
    if (cur == 0) {
      cur = A::cas(table + s, mine);
      if (cur == 0) return row;
    }
    if ((unsigned)(cur >> 32) == tag) {
      const unsigned other = (unsigned)cur - 1u;
      if (qh_wk_equal(cols, ncols, row, other)) return other;
    }
    s = (s + 1u) & slot_mask;
  }
}

// ---- join keys (join.cpp maybe_encode_wide_join_key, kernels_rel.hip k_widekey_join_build / k_widekey_join_lookup): the build
// side's rows are inserted as above, the probe side's rows are then looked up in the finished table, so that both sides carry
// codes of ONE numbering: build code == probe code <=> the keys are equal and non-NULL. In a join a NULL key never matches
// (probe_hash_table, hash_join.rs:191-215), unlike GROUP BY where NULL is a value of its own.

// any key column NULL in this row?
QH_WK_HD inline bool qh_wk_any_null(const qh_wk_col* cols, int ncols, unsigned row) {
  for (int k = 0; k < ncols; ++k)
    if (!qh_wk_valid(cols[k], row)) return true;
  return false;
}

// qh_wk_equal with row a read through colsA and row b through colsB (the same types column by column: the host checks that).
// Both rows are known to have no NULL key column. Same masked-tail Utf8 word reads, same slack behind the data buffers.
QH_WK_HD inline bool qh_wk_equal2(const qh_wk_col* colsA, const qh_wk_col* colsB, int ncols, unsigned a, unsigned b) {
  for (int k = 0; k < ncols; ++k) {
    const qh_wk_col& ca = colsA[k];
    const qh_wk_col& cb = colsB[k];
    if (ca.width == 0) {
      const int* offa = (const int*)ca.v;
      const int* offb = (const int*)cb.v;
      const unsigned oa = (unsigned)offa[a], la = (unsigned)offa[a + 1] - oa;
      const unsigned ob = (unsigned)offb[b], lb = (unsigned)offb[b + 1] - ob;
      if (la != lb) return false;
      const unsigned nw = (la + 7) >> 3;
      for (unsigned w = 0; w < nw; ++w)
        if (qh_wk_str_word(ca.d + oa, la, w) != qh_wk_str_word(cb.d + ob, la, w)) return false;
    } else if (ca.width == 16) {
      const unsigned long long* va = (const unsigned long long*)ca.v + 2 * (unsigned long long)a;
      const unsigned long long* vb = (const unsigned long long*)cb.v + 2 * (unsigned long long)b;
      if (va[0] != vb[0] || va[1] != vb[1]) return false;
    } else if (qh_wk_word(ca, a) != qh_wk_word(cb, b)) {
      return false;
    }
  }
  return true;
}

// The code of a BUILD row: a row with a NULL key column is not inserted and is its own code (unique, and no inserted key's:
// a representative is always a row without NULLs); every other row is inserted as above. Codes lie in [0, build rows).
template <class A>
QH_WK_HD inline unsigned qh_wk_join_build_row(const qh_wk_col* cols, int ncols, unsigned long long* table, unsigned slot_mask,
                                              unsigned long long hash_mask, unsigned row) {
  if (qh_wk_any_null(cols, ncols, row)) return row;
  return qh_wk_insert<A>(cols, ncols, table, slot_mask, hash_mask, row);
}

// The code of a PROBE row: the build row that represents its key, -1 when a key column is NULL or no build row has the key.
// The table is complete and read-only here. The hash of equal non-NULL keys is the same through either side's descriptors.
template <class A>
QH_WK_HD inline int qh_wk_join_lookup_row(const qh_wk_col* pcols, const qh_wk_col* bcols, int ncols, const unsigned long long* table,
                                          unsigned slot_mask, unsigned long long hash_mask, unsigned row) {
  if (qh_wk_any_null(pcols, ncols, row)) return -1;
  const unsigned long long h = qh_wk_hash(pcols, ncols, row) & hash_mask;
  const unsigned tag = (unsigned)(h >> 32);
  unsigned s = (unsigned)h & slot_mask;
  for (;;) {
    const unsigned long long cur = A::load(table + s);
    if (cur == 0) return -1;
    if ((unsigned)(cur >> 32) == tag) {
      const unsigned other = (unsigned)cur - 1u;
      if (qh_wk_equal2(pcols, bcols, ncols, row, other)) return (int)other;
    }
    s = (s + 1u) & slot_mask;
  }
}
