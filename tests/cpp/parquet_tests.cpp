// parquet_tests.cpp — the device Parquet decoder without a device (tests/test_parquet_cpu.py builds and runs this, plainly and
// under the address and undefined-behaviour sanitizers; nothing of it is loaded into Python). It contains the host half as it is
// (qurious_amd/csrc/parquet_meta.hpp: Thrift reader, footer, page walk) and the per-run and per-value code of the kernels
// (csrc/device/qhip_parquet.inc), driven page by page by loops that stand for the lanes of kernels_parquet.hip. Every buffer is
// a heap allocation of exactly the size the data has, so that a read outside the file, its pages or the columns is a report.
//
//   decode FILE TYPES PROJ   TYPES: one code per field of the file (i8 .. u64, f32, f64, date, bool, utf8, ts3 / ts6 / ts9,
//                            dec:P:S, x = a type the C ABI does not carry); PROJ: field indices, or -
//                            -> "ROWS n", "NULLS c0 c1 ..", then one line per row, or "NEEDS_HOST reason rowgroup column page"
//   stream W N FILE          the first N values of the hybrid stream in FILE at bit width W, through the run cursor, 64 per step
//   levels FIRST N FILE      the level stream in FILE for rows FIRST .. FIRST + N -> the rows' validity bits, or "REASON r"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "parquet_meta.hpp"

using namespace qhip_pq;

static std::vector<uint8_t> read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> v((size_t)n);
  if (n && fread(v.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
  fclose(f);
  return v;
}

// exactly-sized heap copies (a std::vector may keep capacity behind its size)
struct Heap {
  uint8_t* p; size_t n;
  explicit Heap(size_t bytes, int fill = 0) : p(new uint8_t[bytes ? bytes : 1]), n(bytes) { memset(p, fill, bytes ? bytes : 1); }
  ~Heap() { delete[] p; }
  Heap(const Heap&) = delete;
};

struct FirstError {
  uint64_t word = ~0ULL;
  void report(uint64_t page, uint32_t reason) { const uint64_t m = (page << 8) | reason; if (m < word) word = m; }
};

// ---- k_pq_levels, one page
static void levels_page(const uint8_t* buf, const qh_pq_page& pg, const qh_pq_col& col, qh_pq_state& st, uint64_t page, FirstError& err, uint64_t& nulls) {
  const uint64_t n = pg.num_values;
  if (!col.valid) { st.nonnull = (uint32_t)n; st.values_off = 0; return; }
  const uint8_t* p = buf + pg.pos;
  uint32_t reason = QH_PQ_OK, len = 0;
  if (pg.size < 4) reason = QH_PQ_R_LEVELS_LENGTH;
  else { len = qh_pq_le32(p); if (len > pg.size - 4) reason = QH_PQ_R_LEVELS_LENGTH; }
  const uint8_t* s = p + 4;
  pq_u64 cpos = 0;
  uint64_t row = 0, nonnull = 0;
  qh_pq_run run;
  qh_pq_run_init(&run);
  while (!reason && row < n) {
    reason = (uint32_t)qh_pq_next_run(s, len, &cpos, 1, &run);
    if (reason) break;
    uint64_t take = run.count;
    const uint64_t left = n - row;
    if (run.packed) { if (take >= left + 8) reason = QH_PQ_R_RUN_COUNT; else if (take > left) take = left; }
    else if (take > left) reason = QH_PQ_R_RUN_COUNT;
    else if (run.value > 1) reason = QH_PQ_R_LEVEL_VALUE;
    if (reason) break;
    const uint64_t g0 = pg.first_row + row;
    if (run.packed || run.value)
      for (uint64_t w = g0 >> 6; w <= ((g0 + take - 1) >> 6); ++w) {   // (the lanes take these words 64 at a time)
        const uint64_t bits = qh_pq_level_word(s, &run, g0, take, w);
        if (w * 64 >= g0 && w * 64 + 64 <= g0 + take) col.valid[w] = bits; else col.valid[w] |= bits;
        nonnull += (uint64_t)__builtin_popcountll(bits);
      }
    row += take;
  }
  st.nonnull = (uint32_t)nonnull;
  st.values_off = 4 + len;
  if (reason) err.report(page, reason); else nulls += n - nonnull;
}

// ---- k_pq_strings, one page (the device stages the same bytes through LDS; the checks are the same two calls)
static void strings_page(const uint8_t* buf, const qh_pq_page& pg, const qh_pq_col& col, const qh_pq_state& st, uint64_t page, FirstError& err) {
  if (col.phys != QH_PQ_P_BYTES || pg.enc == QH_PQ_ENC_DICT) return;
  uint64_t base = pg.pos, size = pg.size, count = pg.num_values;
  if (pg.enc == QH_PQ_ENC_PLAIN) { base += st.values_off; size -= st.values_off; count = st.nonnull; }
  qh_pq_ent* ent = col.ent + pg.ent;
  uint64_t q = 0;
  for (uint64_t k = 0; k < count; ++k) {
    if (!qh_pq_chain_has_prefix(q, size)) { err.report(page, QH_PQ_R_BYTE_ARRAY); return; }
    const uint32_t len = qh_pq_le32(buf + base + q);
    if (!qh_pq_chain_fits(q, size, len)) { err.report(page, QH_PQ_R_BYTE_ARRAY); return; }
    ent[k].pos = base + q + 4; ent[k].len = len; ent[k].pad = 0;
    q += 4 + (uint64_t)len;
  }
}

// the run cursor of k_pq_values for one step of 64 lanes: idx[l] for the lanes with valid[l], `end` = one past the step's
// highest index. Returns a reason.
static uint32_t cursor_step(const uint8_t* s, uint64_t slen, pq_u64* cpos, uint32_t w, qh_pq_run* run, const bool* valid, const uint64_t* idx, uint64_t end,
                            uint32_t* index) {
  bool served[64];
  for (int l = 0; l < 64; ++l) served[l] = !valid[l];
  for (;;) {
    for (int l = 0; l < 64; ++l)
      if (!served[l] && idx[l] >= run->start && idx[l] < run->start + run->count) { index[l] = qh_pq_run_value(s, run, idx[l], w); served[l] = true; }
    if (run->start + run->count >= end) return QH_PQ_OK;
    const int reason = qh_pq_next_run(s, slen, cpos, w, run);
    if (reason) return (uint32_t)reason;
  }
}

// ---- k_pq_values, one page
static void values_page(const uint8_t* buf, const qh_pq_page& pg, const qh_pq_col& col, const qh_pq_state& st, uint64_t page, FirstError& err, uint64_t& utf8_bytes) {
  const uint64_t nn = st.nonnull;
  const uint8_t* v = buf + pg.pos + st.values_off;
  const uint64_t vsize = (uint64_t)pg.size - st.values_off;
  const uint32_t pw = qh_pq_phys_bytes(col.phys, col.flba);
  const bool dict = pg.enc == QH_PQ_ENC_DICT;
  uint32_t reason = QH_PQ_OK, w = 0;
  const uint8_t* s = v;
  uint64_t slen = 0;
  if (dict) {
    if (nn) {
      if (vsize < 1) reason = QH_PQ_R_VALUES_SHORT;
      else { w = v[0]; s = v + 1; slen = vsize - 1; if (w > 32) reason = QH_PQ_R_BIT_WIDTH; }
    }
  } else if (col.phys == QH_PQ_P_BOOL) { if ((nn + 7) / 8 > vsize) reason = QH_PQ_R_VALUES_SHORT; }
  else if (col.phys != QH_PQ_P_BYTES) { if (nn * pw > vsize) reason = QH_PQ_R_VALUES_SHORT; }
  qh_pq_run run;
  qh_pq_run_init(&run);
  pq_u64 cpos = 0;
  uint64_t base = 0, bytes = 0;
  const uint64_t r_begin = pg.first_row, r_end = r_begin + pg.num_values;
  for (uint64_t t0 = r_begin & ~(uint64_t)63; !reason && t0 < r_end; t0 += 64) {
    bool in[64], valid[64];
    uint64_t idx[64];
    uint32_t index[64] = {0};
    for (int l = 0; l < 64; ++l) {
      const uint64_t row = t0 + (uint64_t)l;
      in[l] = row >= r_begin && row < r_end;
      valid[l] = in[l] && (!col.valid || ((col.valid[t0 >> 6] >> l) & 1ULL));
      idx[l] = base;
      if (valid[l]) ++base;
    }
    if (base > nn) { reason = QH_PQ_R_VALUES_SHORT; break; }
    if (dict) {
      reason = cursor_step(s, slen, &cpos, w, &run, valid, idx, base, index);
      if (reason) break;
      for (int l = 0; l < 64; ++l) if (valid[l] && index[l] >= pg.dict_n) reason = QH_PQ_R_DICT_INDEX;
      if (reason) break;
    }
    uint64_t word = 0;
    for (int l = 0; l < 64 && !reason; ++l) {
      const uint64_t row = t0 + (uint64_t)l;
      pq_u64 lo = 0, hi = 0;
      if (col.phys == QH_PQ_P_BYTES) {
        if (!in[l]) continue;
        qh_pq_ent e; e.pos = 0; e.len = 0; e.pad = 0;
        if (valid[l]) e = col.ent[pg.ent + (dict ? (uint64_t)index[l] : idx[l])];
        ((uint32_t*)col.values)[row] = e.len; col.strpos[row] = e.pos; bytes += e.len;
      } else if (col.phys == QH_PQ_P_BOOL) {
        if (valid[l] && ((v[idx[l] >> 3] >> (idx[l] & 7)) & 1)) word |= 1ULL << l;
      } else {
        if (valid[l]) {
          const uint8_t* src = dict ? buf + pg.dict_pos + (uint64_t)index[l] * pw : v + idx[l] * pw;
          qh_pq_read_value(src, col.phys, col.flba, &lo, &hi);
          if (col.narrow && !qh_pq_in_range(lo, col.width, col.narrow)) { reason = QH_PQ_R_RANGE; break; }
        }
        if (in[l]) qh_pq_store(col.values, row, col.width, lo, hi);
      }
    }
    if (col.phys == QH_PQ_P_BOOL && word) ((uint64_t*)col.values)[t0 >> 6] |= word;
  }
  if (reason) err.report(page, reason); else utf8_bytes += bytes;
}

// ---------------------------------------------------------------- decode a whole file
static ArrowType parse_type(const std::string& c) {
  ArrowType t;
  static const struct { const char* code; int id; } kTable[] = {
      {"i8", QHIP_INT8}, {"i16", QHIP_INT16}, {"i32", QHIP_INT32}, {"i64", QHIP_INT64}, {"u8", QHIP_UINT8}, {"u16", QHIP_UINT16}, {"u32", QHIP_UINT32},
      {"u64", QHIP_UINT64}, {"f32", QHIP_FLOAT32}, {"f64", QHIP_FLOAT64}, {"date", QHIP_DATE32}, {"bool", QHIP_BOOL}, {"utf8", QHIP_UTF8},
      {"ts3", QHIP_TIMESTAMP_MS}, {"ts6", QHIP_TIMESTAMP_US}, {"ts9", QHIP_TIMESTAMP_NS}};
  for (const auto& e : kTable) if (c == e.code) t.id = e.id;
  if (c.rfind("dec:", 0) == 0) { t.id = QHIP_DECIMAL128; sscanf(c.c_str(), "dec:%d:%d", &t.precision, &t.scale); }
  return t;
}

static void print_i128(uint64_t lo, uint64_t hi) {
  unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
  const bool neg = (hi >> 63) != 0;
  if (neg) v = ~v + 1;
  char buf[48];
  int n = 0;
  do { buf[n++] = (char)('0' + (int)(v % 10)); v /= 10; } while (v);
  if (neg) putchar('-');
  while (n) putchar(buf[--n]);
}

static int decode(const char* path, const char* type_codes, const char* proj_text) {
  const std::vector<uint8_t> raw = read_file(path);
  Heap file(raw.size());
  if (!raw.empty()) memcpy(file.p, raw.data(), raw.size());
  std::vector<ArrowType> types;
  for (const char* p = type_codes; *p;) {
    const char* e = strchr(p, ',');
    types.push_back(parse_type(e ? std::string(p, e) : std::string(p)));
    if (!e) break;
    p = e + 1;
  }
  std::vector<int32_t> proj;
  if (strcmp(proj_text, "-") != 0) for (const char* p = proj_text; *p;) { proj.push_back(atoi(p)); const char* e = strchr(p, ','); if (!e) break; p = e + 1; }
  else for (size_t k = 0; k < types.size(); ++k) proj.push_back((int32_t)k);
  Plan plan;
  try {
    plan = plan_file(file.p, file.n, nullptr, types, proj);
  } catch (const PqNeedsHost& e) {
    printf("NEEDS_HOST %d %lld %lld %lld\n", e.reason, (long long)e.row_group, (long long)e.column, (long long)e.page);
    return 0;
  }
  const uint64_t R = plan.num_rows, words = (R + 63) / 64;
  Heap buf((size_t)plan.upload_bytes);   // (no slack: the device's vector loads read it, these loops must not)
  for (const Range& r : plan.ranges) memcpy(buf.p + r.buf_off, file.p + r.file_off, (size_t)r.bytes);
  const size_t ncols = proj.size();
  std::vector<std::unique_ptr<Heap>> keep;
  auto heap = [&](size_t n, int fill) { keep.emplace_back(new Heap(n, fill)); return keep.back()->p; };
  std::vector<qh_pq_col> cols(ncols);
  for (size_t k = 0; k < ncols; ++k) {
    const ColPlan& cp = plan.cols[k];
    qh_pq_col& d = cols[k];
    memset(&d, 0, sizeof d);
    if (cp.optional) d.valid = (pq_u64*)heap(words * 8, 0);
    if (cp.utf8) {
      d.values = heap((size_t)(R + 1) * 4, 0xAB);
      d.strpos = (pq_u64*)heap((size_t)R * 8, 0xAB);
      d.ent = (qh_pq_ent*)heap((size_t)(R + cp.dict_entries) * sizeof(qh_pq_ent), 0xAB);
    } else if (cp.boolean) d.values = heap(words * 8, 0);
    else d.values = heap((size_t)R * cp.width, 0xAB);
    d.phys = cp.phys; d.flba = cp.flba; d.width = cp.width; d.narrow = cp.narrow;
  }
  std::vector<qh_pq_state> state(plan.pages.size());
  std::vector<uint64_t> nulls(ncols, 0), utf8(ncols, 0);
  FirstError err;
  for (size_t p = 0; p < plan.pages.size(); ++p)
    if (plan.pages[p].enc != QH_PQ_ENC_DICTPAGE) levels_page(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err, nulls[plan.pages[p].col]);
  if (err.word == ~0ULL)
    for (size_t p = 0; p < plan.pages.size(); ++p) strings_page(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err);
  if (err.word == ~0ULL)
    for (size_t p = 0; p < plan.pages.size(); ++p)
      if (plan.pages[p].enc != QH_PQ_ENC_DICTPAGE) values_page(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err, utf8[plan.pages[p].col]);
  if (err.word != ~0ULL) {
    const PageWhere& w = plan.where[(size_t)(err.word >> 8)];
    printf("NEEDS_HOST %d %lld %lld %lld\n", (int)(err.word & 0xFF), (long long)w.row_group, (long long)w.column, (long long)w.page);
    return 0;
  }
  printf("ROWS %llu\nNULLS", (unsigned long long)R);
  for (size_t k = 0; k < ncols; ++k) printf(" %llu", (unsigned long long)nulls[k]);
  printf("\n");
  for (uint64_t r = 0; r < R; ++r) {
    for (size_t k = 0; k < ncols; ++k) {
      const qh_pq_col& d = cols[k];
      const ArrowType& ty = types[(size_t)proj[k]];
      if (k) putchar('\t');
      if (d.valid && !((d.valid[r >> 6] >> (r & 63)) & 1)) { putchar('N'); continue; }
      switch (ty.id) {
        case QHIP_BOOL: putchar((((uint64_t*)d.values)[r >> 6] >> (r & 63)) & 1 ? '1' : '0'); break;
        case QHIP_INT8: printf("%d", (int)((int8_t*)d.values)[r]); break;
        case QHIP_INT16: printf("%d", (int)((int16_t*)d.values)[r]); break;
        case QHIP_INT32: case QHIP_DATE32: printf("%d", ((int32_t*)d.values)[r]); break;
        case QHIP_UINT8: printf("%u", (unsigned)((uint8_t*)d.values)[r]); break;
        case QHIP_UINT16: printf("%u", (unsigned)((uint16_t*)d.values)[r]); break;
        case QHIP_UINT32: printf("%u", ((uint32_t*)d.values)[r]); break;
        case QHIP_FLOAT32: printf("%08x", ((uint32_t*)d.values)[r]); break;
        case QHIP_UINT64: printf("%llu", (unsigned long long)((uint64_t*)d.values)[r]); break;
        case QHIP_FLOAT64: printf("%016llx", (unsigned long long)((uint64_t*)d.values)[r]); break;
        case QHIP_DECIMAL128: print_i128(((uint64_t*)d.values)[2 * r], ((uint64_t*)d.values)[2 * r + 1]); break;
        case QHIP_UTF8: {
          putchar('s');
          const uint32_t len = ((uint32_t*)d.values)[r];
          const uint64_t pos = d.strpos[r];
          if (pos > plan.upload_bytes || len > plan.upload_bytes - pos) { fprintf(stderr, "a string outside the buffer\n"); return 3; }
          for (uint32_t b = 0; b < len; ++b) printf("%02x", buf.p[pos + b]);
          break;
        }
        default: printf("%lld", (long long)((int64_t*)d.values)[r]); break;   // Int64, Timestamp
      }
    }
    putchar('\n');
  }
  return 0;
}

// ---------------------------------------------------------------- one hybrid stream through the run cursor
static int stream(uint32_t w, uint64_t n, const char* path) {
  const std::vector<uint8_t> raw = read_file(path);
  Heap s(raw.size());
  if (!raw.empty()) memcpy(s.p, raw.data(), raw.size());
  qh_pq_run run;
  qh_pq_run_init(&run);
  pq_u64 cpos = 0;
  std::vector<uint32_t> out;
  for (uint64_t t0 = 0; t0 < n; t0 += 64) {
    bool valid[64];
    uint64_t idx[64];
    uint32_t index[64] = {0};
    for (int l = 0; l < 64; ++l) { idx[l] = t0 + (uint64_t)l; valid[l] = idx[l] < n; }
    const uint64_t end = t0 + 64 < n ? t0 + 64 : n;
    const uint32_t reason = cursor_step(s.p, s.n, &cpos, w, &run, valid, idx, end, index);
    if (reason) { printf("REASON %u\n", reason); return 0; }
    for (int l = 0; l < 64; ++l) if (valid[l]) out.push_back(index[l]);
  }
  for (uint32_t v : out) printf("%u\n", v);
  return 0;
}

static int levels(uint64_t first, uint64_t n, const char* path) {
  const std::vector<uint8_t> raw = read_file(path);
  Heap page(raw.size() + 4);
  const uint32_t len = (uint32_t)raw.size();
  memcpy(page.p, &len, 4);
  if (!raw.empty()) memcpy(page.p + 4, raw.data(), raw.size());
  const uint64_t words = (first + n + 63) / 64;
  Heap bitmap((size_t)words * 8);
  qh_pq_page pg;
  memset(&pg, 0, sizeof pg);
  pg.first_row = first; pg.size = (uint32_t)page.n; pg.num_values = (uint32_t)n;
  qh_pq_col col;
  memset(&col, 0, sizeof col);
  col.valid = (pq_u64*)bitmap.p;
  qh_pq_state st;
  FirstError err;
  uint64_t nulls = 0;
  levels_page(page.p, pg, col, st, 0, err, nulls);
  if (err.word != ~0ULL) { printf("REASON %u\n", (unsigned)(err.word & 0xFF)); return 0; }
  for (uint64_t r = 0; r < first; ++r) if ((col.valid[r >> 6] >> (r & 63)) & 1) { fprintf(stderr, "a bit in front of the page\n"); return 3; }
  std::string out;
  for (uint64_t r = first; r < first + n; ++r) out += ((col.valid[r >> 6] >> (r & 63)) & 1) ? '1' : '0';
  printf("%s\nNONNULL %u NULLS %llu\n", out.c_str(), st.nonnull, (unsigned long long)nulls);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "decode")) return decode(argv[2], argv[3], argv[4]);
  if (argc == 5 && !strcmp(argv[1], "stream")) return stream((uint32_t)atoi(argv[2]), strtoull(argv[3], nullptr, 10), argv[4]);
  if (argc == 5 && !strcmp(argv[1], "levels")) return levels(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), argv[4]);
  fprintf(stderr, "usage: decode FILE TYPES PROJ | stream W N FILE | levels FIRST N FILE\n");
  return 2;
}
