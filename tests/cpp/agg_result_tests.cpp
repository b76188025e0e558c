// The hash aggregate's host-side result logic (qurious_amd/csrc/agg_result.cpp) without a GPU: AggPlan descriptors and slot
// words are built by hand here, and every expected value is written out or computed with plain arithmetic in this file.
// Slot layout: [occupancy word | W key words (word 0 = the null mask when the plan has one) | cells].
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "agg_result.hpp"

using namespace qhip;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    ++g_checked;                                                                    \
    if (!(cond)) { ++g_failed; fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static const DType I8(QHIP_INT8), I16(QHIP_INT16), I32(QHIP_INT32), I64(QHIP_INT64), U32(QHIP_UINT32), F32(QHIP_FLOAT32), F64(QHIP_FLOAT64),
    D32(QHIP_DATE32), UTF8(QHIP_UTF8), DEC15_2(QHIP_DECIMAL128, 15, 2), DEC19_6(QHIP_DECIMAL128, 19, 6);

// ---- order-preserving images, as the kernels store them in MAXORD cells (MIN cells hold the complement)
static uint64_t ord_i64(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ULL; }
static uint64_t ord_f64(double d) {
  uint64_t b; memcpy(&b, &d, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
static u128 ord_i128(i128 v) { return (u128)v ^ ((u128)1 << 127); }

// ---- plans by hand
struct PlanBuilder {
  AggPlan p;
  int cell_words = 0;
  PlanBuilder() { add_cell(CELL_ROWS, -1, false, 1); }
  int add_cell(int kind, int arg, bool is_min, int words) {
    CellDesc c; c.kind = kind; c.arg = arg; c.is_min = is_min; c.off = cell_words; c.words = words;
    cell_words += words;
    p.cells.push_back(c);
    return (int)p.cells.size() - 1;
  }
  void key(const DType& t, bool nullable, int words) {
    if (p.keys.empty() && p.null_mask_word) p.W = 1;
    KeyDesc k; k.root = 0; k.type = t; k.nullable = nullable; k.word_off = p.W; k.words = words;
    p.W += words;
    p.keys.push_back(k);
  }
  // an aggregate over an argument of its own: a CELL_CNT cell for its non-null count + the value cell (none for COUNT)
  void agg(int kind, const DType& ret, const DType& arg_type, int value_cell_kind = -1, int value_words = 0) {
    ArgDesc a; a.root = 0; a.type = arg_type; a.nullable = true;
    p.args.push_back(a);
    const int arg = (int)p.args.size() - 1;
    AggDesc d; d.kind = kind; d.ret = ret; d.arg = arg;
    d.count_cell = add_cell(CELL_CNT, arg, false, 1);
    d.value_cell = value_cell_kind < 0 ? -1 : add_cell(value_cell_kind, arg, kind == QHIP_AGG_MIN, value_words);
    p.aggs.push_back(d);
  }
  void count_rows() {   // COUNT(*) / COUNT over an argument that is never NULL: the CELL_ROWS cell
    AggDesc d; d.kind = QHIP_AGG_COUNT; d.ret = I64; d.arg = -1; d.count_cell = 0; d.value_cell = -1;
    p.aggs.push_back(d);
  }
  const AggPlan& done() { p.slot_words = 1 + p.W + cell_words; return p; }
  // word offsets inside a slot
  int key_word(int k, int w = 0) const { return 1 + p.keys[(size_t)k].word_off + w; }
  int cnt_word(int a) const { return 1 + p.W + p.cells[(size_t)p.aggs[(size_t)a].count_cell].off; }
  int val_word(int a, int w = 0) const { return 1 + p.W + p.cells[(size_t)p.aggs[(size_t)a].value_cell].off + w; }
};

template <class T> static T value_at(HostColumn& c, size_t g) { T v; memcpy(&v, c.values.data() + g * sizeof(T), sizeof(T)); return v; }
static i128 dec_at(HostColumn& c, size_t g) {
  uint64_t lo = value_at<uint64_t>(c, 2 * g), hi = value_at<uint64_t>(c, 2 * g + 1);
  return (i128)(((u128)hi << 64) | lo);
}
static bool is_null(const HostColumn& c, size_t g) { return !c.validity.empty() && !((c.validity[g >> 3] >> (g & 7)) & 1); }

// ---------------------------------------------------------------- replica merge + every cell kind through the columns
// One Int64 key; D distinct keys spread over 3 table replicas: key 0 sits in all three, key 1 (when there is one) only in replica 1,
// key j >= 2 in replicas {j % 3, (j + 1) % 3}. Slot order: replica 0's keys ascending, then replica 1's, then replica 2's.
static bool in_replica(int j, int r) { return j == 0 || (j == 1 ? r == 1 : (r == j % 3 || r == (j + 1) % 3)); }
static int64_t contrib(int j, int r) { return (int64_t)(j * 37 + r * 11) - 400; }   // distinct per (key, replica), both signs

static void test_merge(int D) {
  PlanBuilder b;
  b.key(I64, false, 1);
  b.count_rows();                                            // 0
  b.agg(QHIP_AGG_SUM, I64, I64, CELL_SUM_U64, 1);            // 1
  b.agg(QHIP_AGG_SUM, DEC15_2, DEC15_2, CELL_SUM_I128, 2);   // 2
  b.agg(QHIP_AGG_SUM, F64, F64, CELL_SUM_F64, 1);            // 3
  b.agg(QHIP_AGG_MAX, I64, I64, CELL_MAXORD64, 1);           // 4
  b.agg(QHIP_AGG_MIN, I64, I64, CELL_MAXORD64, 1);           // 5
  b.agg(QHIP_AGG_MAX, DEC15_2, DEC15_2, CELL_MAXORD128, 2);  // 6
  b.agg(QHIP_AGG_MIN, DEC15_2, DEC15_2, CELL_MAXORD128, 2);  // 7
  b.agg(QHIP_AGG_MAX, F64, F64, CELL_MAXORD64, 1);           // 8
  b.agg(QHIP_AGG_MIN, F64, F64, CELL_MAXORD64, 1);           // 9
  b.agg(QHIP_AGG_AVG, F64, F64, CELL_SUM_F64, 1);            // 10
  const AggPlan& p = b.done();
  const int sw = p.slot_words;
  const i128 big = (i128)1 << 70;   // Decimal contributions beyond 64 bits: v * 2^70
  std::vector<uint64_t> slots;
  std::vector<int> first_seen;      // keys in the order of their first slot
  uint32_t G = 0;
  for (int r = 0; r < 3; ++r)
    for (int j = 0; j < D; ++j) {
      if (!in_replica(j, r)) continue;
      bool seen = false;
      for (int k : first_seen) seen = seen || k == j;
      if (!seen) first_seen.push_back(j);
      std::vector<uint64_t> s((size_t)sw, 0);
      const int64_t v = contrib(j, r);
      const uint64_t rows = (uint64_t)(r + 1);   // the replica saw r + 1 rows of the key, all with the same value
      s[0] = 1;
      s[(size_t)b.key_word(0)] = (uint64_t)(int64_t)(1000 - j);
      s[(size_t)(1 + p.W)] = rows;
      for (int a = 1; a <= 10; ++a) s[(size_t)b.cnt_word(a)] = rows;
      s[(size_t)b.val_word(1)] = (uint64_t)(v * (int64_t)rows);
      const u128 ds = (u128)((i128)v * big * (i128)rows);
      s[(size_t)b.val_word(2)] = (uint64_t)ds; s[(size_t)b.val_word(2, 1)] = (uint64_t)(ds >> 64);
      const double fs = (double)v * 0.25 * (double)rows;
      memcpy(&s[(size_t)b.val_word(3)], &fs, 8);
      memcpy(&s[(size_t)b.val_word(10)], &fs, 8);
      s[(size_t)b.val_word(4)] = ord_i64(v);
      s[(size_t)b.val_word(5)] = ~ord_i64(v);
      const u128 od = ord_i128((i128)v * big);
      s[(size_t)b.val_word(6)] = (uint64_t)od; s[(size_t)b.val_word(6, 1)] = (uint64_t)(od >> 64);
      s[(size_t)b.val_word(7)] = (uint64_t)~od; s[(size_t)b.val_word(7, 1)] = (uint64_t)(~od >> 64);
      s[(size_t)b.val_word(8)] = ord_f64((double)v * 0.25);
      s[(size_t)b.val_word(9)] = ~ord_f64((double)v * 0.25);
      slots.insert(slots.end(), s.begin(), s.end());
      ++G;
    }
  const uint32_t merged = merge_replica_slots(p, slots, G);
  CHECK(merged == (uint32_t)D);
  CHECK(slots.size() == (size_t)D * (size_t)sw);
  std::vector<HostColumn> cols = assemble_host_columns(p, slots, merged, 1, 11, false);
  CHECK(cols.size() == 12);
  for (size_t g = 0; g < (size_t)merged && g < first_seen.size(); ++g) {
    const int j = first_seen[g];
    int64_t rows = 0, sum = 0, mx = INT64_MIN, mn = INT64_MAX;
    for (int r = 0; r < 3; ++r)
      if (in_replica(j, r)) {
        const int64_t v = contrib(j, r);
        rows += r + 1; sum += v * (r + 1);
        if (v > mx) mx = v;
        if (v < mn) mn = v;
      }
    CHECK(value_at<int64_t>(cols[0], g) == 1000 - j);
    CHECK(value_at<int64_t>(cols[1], g) == rows);
    CHECK(value_at<int64_t>(cols[2], g) == sum);
    CHECK(dec_at(cols[3], g) == (i128)sum * big);
    CHECK(value_at<double>(cols[4], g) == (double)sum * 0.25);   // (multiples of 0.25 far below 2^53: every partial sum is exact)
    CHECK(value_at<int64_t>(cols[5], g) == mx);
    CHECK(value_at<int64_t>(cols[6], g) == mn);
    CHECK(dec_at(cols[7], g) == (i128)mx * big);
    CHECK(dec_at(cols[8], g) == (i128)mn * big);
    CHECK(value_at<double>(cols[9], g) == (double)mx * 0.25);
    CHECK(value_at<double>(cols[10], g) == (double)mn * 0.25);
    CHECK(value_at<double>(cols[11], g) == (double)sum * 0.25 / (double)rows);
    for (auto& c : cols) CHECK(c.null_count == 0);
  }
}

static void test_merge_i128_carry_and_wrap() {
  PlanBuilder b;
  b.key(I64, false, 1);
  b.agg(QHIP_AGG_SUM, DEC15_2, DEC15_2, CELL_SUM_I128, 2);
  const AggPlan& p = b.done();
  const int sw = p.slot_words;
  const uint64_t ones = ~0ULL;
  // key 7: (hi 5, lo 2^64 - 1) + (hi 1, lo 2) = (hi 7, lo 1): a carry out of the low word
  // key 9: (hi 2^64 - 1, lo 2^64 - 1) + (hi 0, lo 1) = 0: wraps mod 2^128
  const uint64_t in[4][3] = {{7, ones, 5}, {9, ones, ones}, {7, 2, 1}, {9, 1, 0}};
  std::vector<uint64_t> slots((size_t)(4 * sw), 0);
  for (int g = 0; g < 4; ++g) {
    uint64_t* s = &slots[(size_t)(g * sw)];
    s[0] = 1; s[b.key_word(0)] = in[g][0]; s[1 + p.W] = 1; s[b.cnt_word(0)] = 1;
    s[b.val_word(0)] = in[g][1]; s[b.val_word(0, 1)] = in[g][2];
  }
  CHECK(merge_replica_slots(p, slots, 4) == 2);
  CHECK(slots[(size_t)b.key_word(0)] == 7 && slots[(size_t)b.val_word(0)] == 1 && slots[(size_t)b.val_word(0, 1)] == 7);
  CHECK(slots[(size_t)(sw + b.key_word(0))] == 9 && slots[(size_t)(sw + b.val_word(0))] == 0 && slots[(size_t)(sw + b.val_word(0, 1))] == 0);
  CHECK(slots[(size_t)b.cnt_word(0)] == 2 && slots[(size_t)(sw + b.cnt_word(0))] == 2);
}

// ---------------------------------------------------------------- MIN / MAX of a cell no value ever reached
static void test_min_max_seeds() {
  PlanBuilder b;
  b.key(I64, false, 1);
  const DType types[] = {I8, I16, I32, I64, D32, U32, F32, F64};
  for (const DType& t : types) {
    b.agg(QHIP_AGG_MIN, t, t, CELL_MAXORD64, 1);
    b.agg(QHIP_AGG_MAX, t, t, CELL_MAXORD64, 1);
  }
  b.agg(QHIP_AGG_MIN, DEC15_2, DEC15_2, CELL_MAXORD128, 2);
  b.agg(QHIP_AGG_MAX, DEC15_2, DEC15_2, CELL_MAXORD128, 2);
  const AggPlan& p = b.done();
  std::vector<uint64_t> slots((size_t)p.slot_words, 0);
  slots[0] = 1; slots[(size_t)b.key_word(0)] = 3; slots[(size_t)(1 + p.W)] = 5;   // a group of 5 rows whose arguments were all NULL
  std::vector<HostColumn> c = assemble_host_columns(p, slots, 1, 1, 18, false);
  for (auto& col : c) CHECK(col.null_count == 0);   // Some(seed), not NULL: the group exists
  CHECK(value_at<int8_t>(c[1], 0) == 127 && value_at<int8_t>(c[2], 0) == -128);
  CHECK(value_at<int16_t>(c[3], 0) == 32767 && value_at<int16_t>(c[4], 0) == -32768);
  CHECK(value_at<int32_t>(c[5], 0) == 2147483647 && value_at<int32_t>(c[6], 0) == -2147483647 - 1);
  CHECK(value_at<int64_t>(c[7], 0) == INT64_MAX && value_at<int64_t>(c[8], 0) == INT64_MIN);
  CHECK(value_at<int32_t>(c[9], 0) == 2147483647 && value_at<int32_t>(c[10], 0) == -2147483647 - 1);
  CHECK(value_at<uint32_t>(c[11], 0) == 4294967295u && value_at<uint32_t>(c[12], 0) == 0u);
  CHECK(value_at<float>(c[13], 0) == FLT_MAX && value_at<float>(c[14], 0) == -FLT_MAX);
  CHECK(value_at<double>(c[15], 0) == DBL_MAX && value_at<double>(c[16], 0) == -DBL_MAX);
  const i128 i128_max = (i128)(~(u128)0 >> 1), i128_min = -i128_max - 1;
  CHECK(dec_at(c[17], 0) == i128_max && dec_at(c[18], 0) == i128_min);
  CHECK(c[1].values.size() == 1 && c[3].values.size() == 2 && c[5].values.size() == 4 && c[17].values.size() == 16);
}

static void test_ord_to_f64() {
  const double v[] = {0.0, -0.0, 1.5, -1.5, DBL_MAX, -DBL_MAX, 4.9406564584124654e-324, -2.2250738585072014e-308};
  for (double d : v) {
    const double back = ord_to_f64(ord_f64(d));
    CHECK(memcmp(&back, &d, 8) == 0);
  }
  CHECK(ord_to_f64(0xBFF8000000000000ULL) == 1.5);    // bits of 1.5 = 0x3FF8..., sign bit flipped
  CHECK(ord_to_f64(0x4007FFFFFFFFFFFFULL) == -1.5);   // bits of -1.5 = 0xBFF8..., complemented
}

// ---------------------------------------------------------------- NoGrouping, zero non-null counts
static void test_no_grouping_and_null_results() {
  PlanBuilder b;   // W = 0: the one slot is [occupancy | cells]
  b.count_rows();                                            // 0
  b.agg(QHIP_AGG_COUNT, I64, I64);                           // 1
  b.agg(QHIP_AGG_SUM, I64, I64, CELL_SUM_U64, 1);            // 2
  b.agg(QHIP_AGG_SUM, DEC15_2, DEC15_2, CELL_SUM_I128, 2);   // 3
  b.agg(QHIP_AGG_AVG, F64, F64, CELL_SUM_F64, 1);            // 4
  b.agg(QHIP_AGG_AVG, DEC19_6, DEC15_2, CELL_SUM_I128, 2);   // 5
  b.agg(QHIP_AGG_MIN, I32, I32, CELL_MAXORD64, 1);           // 6
  b.agg(QHIP_AGG_MAX, F64, F64, CELL_MAXORD64, 1);           // 7
  b.agg(QHIP_AGG_MAX, DEC15_2, DEC15_2, CELL_MAXORD128, 2);  // 8
  const AggPlan& p = b.done();
  CHECK(p.W == 0 && p.slot_words == 20);   // occupancy + ROWS + 8 count cells + 10 value words
  std::vector<uint64_t> slots((size_t)p.slot_words, 0);
  {   // no input batch at all: COUNT 0, everything else NULL
    std::vector<HostColumn> c = assemble_host_columns(p, slots, 1, 0, 9, true);
    CHECK(c.size() == 9);
    CHECK(value_at<int64_t>(c[0], 0) == 0 && c[0].null_count == 0 && value_at<int64_t>(c[1], 0) == 0 && c[1].null_count == 0);
    for (size_t k = 2; k < 9; ++k) CHECK(c[k].null_count == 1 && is_null(c[k], 0) && c[k].length == 1);
  }
  {   // batches arrived, every argument NULL: SUM / AVG NULL, MIN / MAX the seeds
    slots[1] = 4;
    std::vector<HostColumn> c = assemble_host_columns(p, slots, 1, 0, 9, false);
    CHECK(value_at<int64_t>(c[0], 0) == 4 && value_at<int64_t>(c[1], 0) == 0);
    for (size_t k = 2; k < 6; ++k) CHECK(c[k].null_count == 1 && is_null(c[k], 0));
    CHECK(c[6].null_count == 0 && value_at<int32_t>(c[6], 0) == 2147483647);
    CHECK(c[7].null_count == 0 && value_at<double>(c[7], 0) == -DBL_MAX);
    CHECK(c[8].null_count == 0 && dec_at(c[8], 0) == -(i128)(~(u128)0 >> 1) - 1);
  }
}

// ---------------------------------------------------------------- Decimal AVG (avg.rs:91-116)
static std::string avg_error(const AggPlan& p, std::vector<uint64_t>& slots, uint32_t G) {
  try {
    assemble_host_columns(p, slots, G, 1, 1, false);
  } catch (const Error& e) {
    CHECK(e.code == QHIP_EXEC_ERROR);
    return e.what();
  }
  return "";
}
static void test_decimal_avg() {
  PlanBuilder b;
  b.key(I64, false, 1);
  b.agg(QHIP_AGG_AVG, DEC19_6, DEC15_2, CELL_SUM_I128, 2);   // scaled by 10^4
  const AggPlan& p = b.done();
  const int sw = p.slot_words;
  struct Case { i128 sum; uint64_t cnt; i128 want; };
  const Case cases[] = {{-1, 3, -3333}, {1, 3, 3333}, {-7, 2, -35000}, {-20, 3, -66666}, {123456789, 7, (i128)1234567890000 / 7}, {5, 0, 0}};
  std::vector<uint64_t> slots((size_t)(6 * sw), 0);
  for (int g = 0; g < 6; ++g) {
    uint64_t* s = &slots[(size_t)(g * sw)];
    s[0] = 1; s[b.key_word(0)] = (uint64_t)g; s[1 + p.W] = 3; s[b.cnt_word(0)] = cases[g].cnt;
    s[b.val_word(0)] = (uint64_t)(u128)cases[g].sum; s[b.val_word(0, 1)] = (uint64_t)((u128)cases[g].sum >> 64);
  }
  std::vector<HostColumn> c = assemble_host_columns(p, slots, 6, 1, 1, false);
  for (size_t g = 0; g < 5; ++g) CHECK(!is_null(c[1], g) && dec_at(c[1], g) == cases[g].want);
  CHECK(-10000 / 3 == -3333);   // (what "truncating toward zero" means for the first case: floor would give -3334)
  CHECK(is_null(c[1], 5) && c[1].null_count == 1);
  CHECK(c[1].type.id == QHIP_DECIMAL128 && c[1].type.precision == 19 && c[1].type.scale == 6);

  std::vector<uint64_t> one((size_t)sw, 0);
  one[0] = 1; one[(size_t)(1 + p.W)] = 1; one[(size_t)b.cnt_word(0)] = 1;
  const u128 huge = (u128)1 << 126;   // 2^126 * 10^4 does not fit i128
  one[(size_t)b.val_word(0)] = (uint64_t)huge; one[(size_t)b.val_word(0, 1)] = (uint64_t)(huge >> 64);
  CHECK(avg_error(p, one, 1) == "AVG(Decimal128): sum * 10^k overflows i128 (reference yields a mistyped NULL, avg.rs:105-116)");
  one[(size_t)b.val_word(0)] = 1000000000000000ULL; one[(size_t)b.val_word(0, 1)] = 0;   // 10^15 * 10^4 = 10^19: not below 10^19
  CHECK(avg_error(p, one, 1) == "AVG(Decimal128): scaled sum exceeds Decimal128(19, 6) (reference yields a mistyped NULL, avg.rs:105-116)");
  const u128 neg = (u128)(-(i128)1000000000000000LL);
  one[(size_t)b.val_word(0)] = (uint64_t)neg; one[(size_t)b.val_word(0, 1)] = (uint64_t)(neg >> 64);
  CHECK(avg_error(p, one, 1) == "AVG(Decimal128): scaled sum exceeds Decimal128(19, 6) (reference yields a mistyped NULL, avg.rs:105-116)");
  one[(size_t)b.val_word(0)] = 999999999999999ULL; one[(size_t)b.val_word(0, 1)] = 0;    // 10^15 - 1: the largest sum that fits
  CHECK(avg_error(p, one, 1) == "");

  PlanBuilder nb;   // a result scale below the argument's
  nb.key(I64, false, 1);
  nb.agg(QHIP_AGG_AVG, DType(QHIP_DECIMAL128, 19, 1), DEC15_2, CELL_SUM_I128, 2);
  const AggPlan& np = nb.done();
  CHECK(avg_error(np, one, 1) == "Internal error: Arithmetic Overflow in DecimalAvgAccumulator");
  try { describe_fin_cols(np, 1, 1); CHECK(false); } catch (const Error& e) { CHECK(std::string(e.what()) == "Internal error: Arithmetic Overflow in DecimalAvgAccumulator"); }
}

// ---------------------------------------------------------------- key decode
static void pack_utf8(const std::string& s, int words, uint64_t* kw) {   // bytes little-endian across the words, the length in the top byte of the last
  for (int w = 0; w < words; ++w) kw[w] = 0;
  for (size_t k = 0; k < s.size(); ++k) kw[k >> 3] |= (uint64_t)(uint8_t)s[k] << (8 * (k & 7));
  kw[words - 1] |= (uint64_t)s.size() << 56;
}
static void test_keys() {
  PlanBuilder b;
  b.p.null_mask_word = true;
  b.key(UTF8, true, 2);        // word_off 1 (behind the null mask)
  b.key(DEC15_2, false, 2);    // word_off 3
  b.key(I32, true, 1);         // word_off 5
  b.count_rows();
  const AggPlan& p = b.done();
  CHECK(p.W == 6 && p.slot_words == 8);
  CHECK(p.keys[0].word_off == 1 && p.keys[1].word_off == 3 && p.keys[2].word_off == 5);
  const std::string strs[] = {"", "sevenby", "eight by", "nine byte", "fifteen bytes.."};
  CHECK(strs[1].size() == 7 && strs[2].size() == 8 && strs[3].size() == 9 && strs[4].size() == 15);
  const i128 decs[] = {0, -12345, ((i128)1 << 100) + 77, -((i128)1 << 100), 99999, 1, 2};
  const int32_t ints[] = {-5, 2147483647, -2147483647 - 1, 0, 42, 0, 6};
  const int G = 7;   // group 5: NULL Utf8 key, group 6: NULL Int32 key (both: mask bit set, key words zero)
  std::vector<uint64_t> slots((size_t)(G * p.slot_words), 0);
  for (int g = 0; g < G; ++g) {
    uint64_t* s = &slots[(size_t)(g * p.slot_words)];
    s[0] = 1;
    s[1] = g == 5 ? 1u : g == 6 ? 4u : 0u;
    if (g != 5) pack_utf8(strs[g == 6 ? 1 : g], 2, s + b.key_word(0));
    s[b.key_word(1)] = (uint64_t)(u128)decs[g]; s[b.key_word(1, 1)] = (uint64_t)((u128)decs[g] >> 64);
    if (g != 6) s[b.key_word(2)] = (uint64_t)(int64_t)ints[g];   // the sign-extended word
    s[1 + p.W] = (uint64_t)(g + 1);
  }
  CHECK(slots[(size_t)b.key_word(2)] == 0xFFFFFFFFFFFFFFFBULL);
  std::vector<HostColumn> c = assemble_host_columns(p, slots, G, 3, 1, false);
  const std::string want_data = strs[0] + strs[1] + strs[2] + strs[3] + strs[4] + "" + strs[1];
  const int32_t want_off[] = {0, 0, 7, 15, 24, 39, 39, 46};
  CHECK(c[0].offsets.size() == 8 && memcmp(c[0].offsets.data(), want_off, sizeof want_off) == 0);
  CHECK(std::string(c[0].data.begin(), c[0].data.end()) == want_data);
  CHECK(c[0].null_count == 1 && is_null(c[0], 5));
  for (size_t g = 0; g < (size_t)G; ++g) {
    if (g != 5) CHECK(!is_null(c[0], g));
    CHECK(dec_at(c[1], g) == decs[g]);
    CHECK(is_null(c[2], g) == (g == 6));
    if (g != 6) CHECK(value_at<int32_t>(c[2], g) == ints[g]);
    CHECK(value_at<int64_t>(c[3], g) == (int64_t)g + 1);
  }
  CHECK(c[1].null_count == 0 && c[1].validity.empty() && c[2].null_count == 1 && c[2].values.size() == 4 * (size_t)G);
}

// ---------------------------------------------------------------- k_agg_finalize's descriptors
static void test_describe_fin_cols() {
  PlanBuilder b;
  b.p.null_mask_word = true;
  b.key(UTF8, true, 3);        // key words 1..3 of the key area (word 0 = null mask)
  b.key(DEC15_2, true, 2);     // 4..5
  b.key(I32, false, 1);        // 6
  b.key(D32, true, 1);         // 7        -> W = 8, the cells start at slot word 9
  b.count_rows();                                            //  0: the ROWS cell, slot word 9
  b.agg(QHIP_AGG_COUNT, I64, I64);                           //  1: cnt 10
  b.agg(QHIP_AGG_SUM, I64, I64, CELL_SUM_U64, 1);            //  2: cnt 11, value 12
  b.agg(QHIP_AGG_SUM, DEC15_2, DEC15_2, CELL_SUM_I128, 2);   //  3: cnt 13, value 14..15
  b.agg(QHIP_AGG_SUM, F64, F64, CELL_SUM_F64, 1);            //  4: cnt 16, value 17
  b.agg(QHIP_AGG_AVG, F64, F64, CELL_SUM_F64, 1);            //  5: cnt 18, value 19
  b.agg(QHIP_AGG_AVG, DEC19_6, DEC15_2, CELL_SUM_I128, 2);   //  6: cnt 20, value 21..22
  b.agg(QHIP_AGG_MIN, I16, I16, CELL_MAXORD64, 1);           //  7: cnt 23, value 24
  b.agg(QHIP_AGG_MAX, U32, U32, CELL_MAXORD64, 1);           //  8: cnt 25, value 26
  b.agg(QHIP_AGG_MIN, F64, F64, CELL_MAXORD64, 1);           //  9: cnt 27, value 28
  b.agg(QHIP_AGG_MAX, F32, F32, CELL_MAXORD64, 1);           // 10: cnt 29, value 30
  b.agg(QHIP_AGG_MIN, DEC15_2, DEC15_2, CELL_MAXORD128, 2);  // 11: cnt 31, value 32..33
  b.agg(QHIP_AGG_MAX, D32, D32, CELL_MAXORD64, 1);           // 12: cnt 34, value 35
  const AggPlan& p = b.done();
  CHECK(p.W == 8 && p.slot_words == 36);
  const std::vector<FinCol> fc = describe_fin_cols(p, 4, 13);
  CHECK(fc.size() == 17);
  struct Want { int kind, src_word, cnt_word, width, key_index, is_min, is_signed, pad; };
  const Want want[17] = {
      {F_KEY_UTF8_LEN, 2, -1, 4, 0, 0, 0, 3}, {F_KEY_DEC, 5, -1, 16, 1, 0, 0, 0}, {F_KEY_FIXED, 7, -1, 4, -1, 0, 0, 0}, {F_KEY_FIXED, 8, -1, 4, 3, 0, 0, 0},
      {F_COUNT, 0, 9, 8, -1, 0, 0, 0},    {F_COUNT, 0, 10, 8, -1, 0, 0, 0},   {F_SUM64, 12, 11, 8, -1, 0, 0, 0},   {F_SUM128, 14, 13, 16, -1, 0, 0, 0},
      {F_SUM64, 17, 16, 8, -1, 0, 0, 0},  {F_AVG_F64, 19, 18, 8, -1, 0, 0, 0}, {F_AVG_DEC, 21, 20, 16, -1, 0, 0, 0}, {F_MM_INT, 24, -1, 2, -1, 1, 1, 0},
      {F_MM_INT, 26, -1, 4, -1, 0, 0, 0}, {F_MM_F64, 28, -1, 8, -1, 1, 0, 0}, {F_MM_F32, 30, -1, 4, -1, 0, 0, 0},  {F_MM_DEC, 32, -1, 16, -1, 1, 0, 0},
      {F_MM_INT, 35, -1, 4, -1, 0, 1, 0}};
  for (size_t k = 0; k < 17; ++k) {
    const FinCol& f = fc[k];
    const Want& w = want[k];
    const bool same = f.kind == w.kind && f.src_word == w.src_word && f.cnt_word == w.cnt_word && f.width == w.width && f.key_index == w.key_index &&
                      f.is_min == w.is_min && f.is_signed == w.is_signed && f.pad == w.pad;
    if (!same) fprintf(stderr, "  column %zu: kind %d src %d cnt %d width %d key %d min %d signed %d pad %d\n", k, f.kind, f.src_word, f.cnt_word, f.width,
                       f.key_index, f.is_min, f.is_signed, f.pad);
    CHECK(same);
    CHECK(f.out_values == nullptr && f.out_valid == nullptr);
    if (f.kind != F_AVG_DEC) CHECK(f.mul_lo == 0 && f.mul_hi == 0 && f.lim_lo == 0 && f.lim_hi == 0);
  }
  // AVG(Decimal(15, 2)) -> Decimal(19, 6): x 10^4, |scaled sum| < 10^19 (= 0x8AC7230489E80000)
  CHECK(fc[10].mul_lo == 10000 && fc[10].mul_hi == 0 && fc[10].lim_lo == 10000000000000000000ULL && fc[10].lim_hi == 0);
  // a limit beyond 64 bits: Decimal(38, 10) from Decimal(20, 2): 10^38 = 0x4B3B4CA85A86C47A * 2^64 + 0x098A224000000000
  PlanBuilder wb;
  wb.key(I64, false, 1);
  wb.agg(QHIP_AGG_AVG, DType(QHIP_DECIMAL128, 38, 10), DType(QHIP_DECIMAL128, 20, 2), CELL_SUM_I128, 2);
  const std::vector<FinCol> wf = describe_fin_cols(wb.done(), 1, 1);
  CHECK(wf[1].mul_lo == 100000000 && wf[1].mul_hi == 0 && wf[1].lim_hi == 0x4B3B4CA85A86C47AULL && wf[1].lim_lo == 0x098A224000000000ULL);
  CHECK(wf[0].kind == F_KEY_FIXED && wf[0].src_word == 1 && wf[0].key_index == -1 && wf[0].width == 8);
}

int main() {
  for (int D : {1, 16, 17, 40}) test_merge(D);   // up to 16 distinct keys: linear search; the 17th builds the map
  test_merge_i128_carry_and_wrap();
  test_min_max_seeds();
  test_ord_to_f64();
  test_no_grouping_and_null_results();
  test_decimal_avg();
  test_keys();
  test_describe_fin_cols();
  printf("agg_result_tests: %d checks, %d failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
