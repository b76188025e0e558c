// The hash join's layout / size / launch-shape arithmetic and its hint and plan keys (qurious_amd/csrc/join_shape.cpp) without a
// GPU. The fixed expectations are the rules' values at Q3's shapes and at their thresholds; the sweeps assert what keeps the
// kernels inside LDS, inside their entry buffers and inside their per-chunk counters.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "join_shape.hpp"

using namespace qhip;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    ++g_checked;                                                                    \
    if (!(cond)) { ++g_failed; fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static const EnvInt kNoOverride;

// ---------------------------------------------------------------- fixed expectations
static void test_region_geometry_table() {
  struct Row { uint64_t B; int W; bool filter; uint32_t n_regions, slot_bits, bword_bits, nslots, filter_words; };
  const Row rows[] = {
      {1460000, 1, false, 2163, 11, 8, 4429824, 553728},
      {1500000, 1, true, 1465, 11, 8, 3000320, 375040},
      {15000000, 1, false, 0, 0, 0, 0, 0},               // load raised to 50 %, still more than 8192 regions: legacy
      {6000000, 2, false, 5860, 11, 8, 12001280, 1500160},   // load raised to 50 %, region grown to 2^11 slots
      {2048, 1, false, 4, 11, 8, 8192, 1024},
      {100000, 7, false, 596, 9, 6, 305152, 38144},
  };
  for (const Row& w : rows) {
    const RegionGeometry g = region_geometry(w.B, w.W, w.filter, kNoOverride, 0);
    CHECK(g.n_regions == w.n_regions);
    if (w.n_regions == 0) continue;
    CHECK(g.slot_bits == w.slot_bits);
    CHECK(g.bword_bits == w.bword_bits);
    const TableSizes z = table_sizes(JOIN_LAYOUT_REGIONS, w.B, w.W, 0, g);
    CHECK(z.nslots == w.nslots);
    CHECK(z.filter_words == w.filter_words);
    CHECK(z.table_bytes == (size_t)w.nslots * (1 + (size_t)w.W) * 8 && z.count_bytes == 0 && z.bloom_bytes == (size_t)w.filter_words * 8);
  }
  // the overrides: a load in percent (clamped to 25..80), slots per region from 2^4
  CHECK(region_geometry(2048, 1, false, EnvInt{true, true, 50}, 0).n_regions == 2);
  CHECK(region_geometry(2048, 1, false, EnvInt{true, true, 5}, 0).load_pct == 25);
  CHECK(region_geometry(2048, 1, false, EnvInt{true, true, 95}, 0).load_pct == 80);
  CHECK(region_geometry(2048, 1, false, EnvInt{true, false, 0}, 0).load_pct == 33);   // set to nothing: the default
  const RegionGeometry g6 = region_geometry(2048, 1, false, kNoOverride, 6);
  CHECK(g6.slot_bits == 6 && g6.bword_bits == 3 && g6.n_regions == (2048 + 20) / 21);
  CHECK(region_geometry(2048, 1, false, kNoOverride, 3).slot_bits == 11);   // below 4: no override
}

static void test_probe_shape_table() {
  struct Row {
    JoinLayout layout; uint64_t P; int probe_r; uint32_t dense_words; int lds_mode; int wgs_per_cu;
    const char* kernel; uint32_t lds_words; unsigned waves; size_t dyn_lds; uint64_t tpw; unsigned grid; uint64_t nchunks;   // 0: not stated
  };
  const Row rows[] = {
      {JOIN_LAYOUT_REGIONS, 1000000, 1, 0, 1, 8, "qk_join_probe", 0, 4, 0, 2, 1954, 7816},
      {JOIN_LAYOUT_DENSE, 60000000, 2, 234375, 1, 4, "qk_join_probe_dense_wide", 0, 4, 12288, 29, 4041, 16164},
      {JOIN_LAYOUT_DENSE, 15000000, 2, 47000, 1, 1, "qk_join_probe_dense_hybrid", 32766, 16, 163832, 29, 253, 4048},
      {JOIN_LAYOUT_DENSE, 15000000, 2, 30000, 1, 1, "qk_join_probe_dense_lds", 30000, 16, 152768, 29, 253, 4048},
      {JOIN_LAYOUT_DENSE, 127, 2, 10, 2, 1, "qk_join_probe_dense", 0, 4, 12288, 0, 1, 0},   // less than one tile: no variant applies
      {JOIN_LAYOUT_DENSE, 128, 2, 10, 2, 1, "qk_join_probe_dense_lds", 10, 16, 32808, 0, 0, 16},
  };
  for (const Row& w : rows) {
    const ProbeKernel k = choose_probe_kernel(w.layout, w.P, w.probe_r, w.dense_words, w.lds_mode, true, 256);
    CHECK(std::string(k.name) == w.kernel);
    CHECK(k.lds_words == w.lds_words);
    CHECK(k.waves_per_wg == w.waves);
    CHECK(k.dyn_lds == w.dyn_lds);
    CHECK(k.tile_rows == 64u * (unsigned)w.probe_r);
    const ProbeGrid g = probe_grid(w.P, k, 256, w.wgs_per_cu, 32);
    if (w.tpw) CHECK(g.tiles_per_wave == w.tpw);
    if (w.grid) CHECK(g.grid == w.grid);
    if (w.nchunks) CHECK(g.nchunks == w.nchunks);
  }
  CHECK(std::string(choose_probe_kernel(JOIN_LAYOUT_LEGACY, 1000, 4, 0, 1, true, 256).name) == "qk_join_probe_onetable");
  CHECK(std::string(choose_probe_kernel(JOIN_LAYOUT_DENSE, 1000, 2, 10, 0, false, 256).name) == "qk_join_probe_dense");   // not wide, no LDS
  CHECK(std::string(choose_probe_kernel(JOIN_LAYOUT_DENSE_RANK, 1000, 2, 10, 0, true, 256).name) == "qk_join_probe_dense_wide");
}

static void test_dense_rules() {
  // automatic mode: the span within 256x the build rows + 65536 and below 2^max_span_bits; mode 2: any span below 2^30
  CHECK(!dense_range_rule(0, 100, 0, 10, 28).candidate);
  CHECK(!dense_range_rule(1, 0, 0, 10, 28).candidate);
  DenseRange d = dense_range_rule(1, 100, -5, 5, 28);
  CHECK(d.candidate && d.dense_n == 11);
  CHECK(dense_range_rule(1, 100, 0, 256 * 100 + 65535, 28).candidate);
  CHECK(!dense_range_rule(1, 100, 0, 256 * 100 + 65536, 28).candidate);
  CHECK(dense_range_rule(2, 100, 0, 256 * 100 + 65536, 28).candidate);
  CHECK(dense_range_rule(1, 1u << 20, 0, (1 << 16) - 1, 16).candidate);
  CHECK(!dense_range_rule(1, 1u << 20, 0, 1 << 16, 16).candidate);
  CHECK(dense_range_rule(2, 1, 0, (1ll << 30) - 1, 28).dense_n == (1ull << 30));
  CHECK(!dense_range_rule(2, 1, 0, 1ll << 30, 28).candidate);
  d = dense_range_rule(2, 1, INT64_MIN, INT64_MAX, 28);   // (the difference fits 64 unsigned bits)
  CHECK(!d.candidate);
  d = dense_range_rule(2, 1, INT64_MIN, INT64_MIN + 7, 28);
  CHECK(d.candidate && d.dense_n == 8);
  // sorted form: one workgroup per 1024 build rows, 16384 bitmap words each at most on average
  CHECK(sorted_build_fits(16384 * 32, 1) && !sorted_build_fits(16384 * 32 + 1, 1));
  CHECK(sorted_build_fits(2 * 16384 * 32, 1025) && !sorted_build_fits(2 * 16384 * 32 + 1, 2048));
  CHECK(sorted_build_fits(1, 0));
  struct F { bool dense, bytemap; int mode; bool asc; uint64_t n, B; bool unsorted, all; bool sorted, rank; };
  const F forms[] = {
      {true, false, 1, true, 1000, 1000, false, true, true, true},
      {true, false, 1, true, 1000, 1000, false, false, true, false},    // a scan filter or NULL keys: row_of stays
      {true, false, 1, false, 1000, 1000, false, true, false, false},   // order not known
      {true, false, 2, false, 1000, 1000, false, true, true, true},     // forced
      {true, false, 2, false, 1000, 1000, true, true, false, false},    // found out of order before
      {true, false, 0, true, 1000, 1000, false, true, false, false},
      {true, true, 2, true, 1000, 1000, false, true, false, false},     // the byte-map form was asked for
      {false, false, 2, true, 1000, 1000, false, true, false, false},
      {true, false, 1, true, 16384 * 32 + 1, 1, false, true, false, false},   // too wide for the workgroups
      {true, false, 2, true, 16384 * 32 + 1, 1, false, true, true, true},     // (forced: the kernel's own cap decides)
  };
  for (const F& f : forms) {
    const DenseBuildForm got = dense_build_form(f.dense, f.bytemap, f.mode, f.asc, f.n, f.B, f.unsorted, f.all);
    CHECK(got.sorted == f.sorted && got.rank == f.rank);
  }
  CHECK(regions_wanted(false, true, 2048, 1) && !regions_wanted(false, true, 2047, 1) && regions_wanted(false, true, 1, 2));
  CHECK(!regions_wanted(true, true, 5000, 2) && !regions_wanted(false, false, 5000, 2) && !regions_wanted(false, true, 0, 2) && !regions_wanted(false, true, 5000, 0));
}

// ---------------------------------------------------------------- invariants
static std::vector<uint64_t> sweep_values() {   // 0, 1, powers of two +- 1 up to 2^32, minus 3
  std::vector<uint64_t> v = {0, 1};
  for (int b = 1; b <= 32; ++b)
    for (int64_t d = -1; d <= 1; ++d) v.push_back((uint64_t)((int64_t)(1ull << b) + d));
  v.push_back((1ull << 32) - 3);
  return v;
}

static void check_sizes(JoinLayout layout, const TableSizes& z) {
  // [table | count | filter]: the three parts follow each other without overlap, the filter 8-byte aligned
  CHECK(z.count_offset() == z.table_bytes);
  CHECK(z.bloom_offset() == z.count_offset() + z.count_bytes);
  CHECK(z.arena_bytes() == z.bloom_offset() + z.bloom_bytes);
  CHECK(z.arena_bytes() == z.table_bytes + z.count_bytes + z.bloom_bytes);
  CHECK(z.bloom_offset() % 8 == 0);
  CHECK(z.count_offset() % 4 == 0);
  (void)layout;
}

static void test_layout_invariants() {
  const std::vector<uint64_t> vals = sweep_values();
  const EnvInt loads[] = {kNoOverride, EnvInt{true, true, 25}, EnvInt{true, true, 50}, EnvInt{true, true, 80}};
  for (uint64_t B : vals) {
    if (B >= 0xFFFFFFFEull) continue;   // (validate_join_args: inputs of 2^32 - 2 rows or more are refused)
    for (int W = 1; W <= 8; ++W) {
      for (int filter = 0; filter < 2; ++filter)
        for (const EnvInt& load : loads)
          for (int sb_override : {0, 4, 8, 12}) {
            const RegionGeometry g = region_geometry(B, W, filter != 0, load, sb_override);
            if (g.n_regions == 0) continue;
            CHECK(g.n_regions <= 8192);
            CHECK(g.lds_bytes(W) <= 64 * 1024);
            CHECK(g.load_pct >= 25 && g.load_pct <= 80);
            const uint64_t per_region = std::max<uint64_t>(1, ((1ull << g.slot_bits) * g.load_pct) / 100);
            CHECK((uint64_t)g.n_regions * per_region >= B);   // capacity at the chosen load
            CHECK(per_region <= (1ull << g.slot_bits));
            const TableSizes z = table_sizes(JOIN_LAYOUT_REGIONS, B, W, 0, g);
            CHECK(z.nslots == g.n_regions << g.slot_bits && (uint64_t)z.nslots >= B);
            CHECK((uint64_t)z.filter_words * 8 == (uint64_t)z.nslots);   // 8 filter bits per slot
            check_sizes(JOIN_LAYOUT_REGIONS, z);
            for (uint64_t max_wgs : {1ull, 7ull, 512ull}) {
              const ScatterShape sc = scatter_shape(B, max_wgs);
              CHECK(sc.wgs >= 1 && sc.wgs <= max_wgs && sc.rows_per_wg % 64 == 0);
              CHECK(sc.wgs * sc.rows_per_wg >= B && (sc.wgs - 1) * sc.rows_per_wg < B);   // every row owned, no empty workgroup
            }
          }
      const TableSizes z = table_sizes(JOIN_LAYOUT_LEGACY, B, W, 0, RegionGeometry());
      CHECK(z.nslots >= 16 && (z.nslots & (z.nslots - 1)) == 0);
      CHECK((uint64_t)z.nslots >= std::min<uint64_t>(2 * B, 1ull << 31));
      CHECK(z.filter_words >= 16 && (z.filter_words & (z.filter_words - 1)) == 0);   // (the probe masks with filter_words - 1)
      CHECK(z.count_bytes >= ((size_t)z.nslots + 2) * 4);
      check_sizes(JOIN_LAYOUT_LEGACY, z);
    }
    for (uint64_t dense_n : vals) {
      if (dense_n == 0 || dense_n > (1ull << 30)) continue;   // (dense_range_rule: a span below 2^30)
      for (JoinLayout layout : {JOIN_LAYOUT_DENSE, JOIN_LAYOUT_DENSE_RANK}) {
        const TableSizes z = table_sizes(layout, B, 1, dense_n, RegionGeometry());
        CHECK((uint64_t)z.dense_words * 32 >= dense_n && ((uint64_t)z.dense_words - 1) * 32 < dense_n);
        CHECK(z.nslots == 0 && z.filter_words == 0 && z.count_bytes == 0);
        CHECK(z.bloom_bytes >= (size_t)z.dense_words * 4 && z.bloom_bytes % 128 == 0);
        CHECK(z.table_bytes >= (layout == JOIN_LAYOUT_DENSE_RANK ? (size_t)z.dense_words : (size_t)dense_n) * 4 && z.table_bytes % 128 == 0);
        check_sizes(layout, z);
      }
    }
  }
}

static void test_probe_invariants() {
  const std::vector<uint64_t> vals = sweep_values();
  const int cus = 256;
  for (uint64_t P : vals) {
    if (P >= 0xFFFFFFFEull) continue;
    for (int probe_r : {1, 2})
      for (JoinLayout layout : {JOIN_LAYOUT_LEGACY, JOIN_LAYOUT_REGIONS, JOIN_LAYOUT_DENSE, JOIN_LAYOUT_DENSE_RANK})
        for (uint64_t dense_n : vals) {
          const bool dense = layout == JOIN_LAYOUT_DENSE || layout == JOIN_LAYOUT_DENSE_RANK;
          if (dense ? (dense_n == 0 || dense_n > (1ull << 30)) : dense_n != 1) continue;
          const uint32_t dense_words = dense ? (uint32_t)((dense_n + 31) / 32) : 0;
          for (int lds_mode = 0; lds_mode <= 2; ++lds_mode)
            for (int wide = 0; wide < 2; ++wide) {
              const ProbeKernel k = choose_probe_kernel(layout, P, probe_r, dense_words, lds_mode, wide != 0, 256);
              CHECK(k.dyn_lds <= 160 * 1024);
              CHECK(k.lds_words <= dense_words);
              CHECK(k.waves_per_wg == 4 || k.waves_per_wg == 16);
              if (dense) {
                CHECK(k.stage_cap >= k.tile_rows);   // at least one tile's worth of entries staged per wavefront
                CHECK(k.dyn_lds >= (size_t)k.lds_words * 4 + (size_t)k.waves_per_wg * 8 * k.stage_cap);
              } else {
                CHECK(k.dyn_lds == 0 && k.lds_words == 0);
              }
              for (int wgs_per_cu = 1; wgs_per_cu <= 8; ++wgs_per_cu) {
                const ProbeGrid g = probe_grid(P, k, cus, wgs_per_cu, 32);
                CHECK(g.grid >= 1 && g.tiles_per_wave >= 1);
                CHECK(g.nchunks == (uint64_t)g.grid * k.waves_per_wg);
                CHECK(g.nchunks * g.tiles_per_wave * k.tile_rows >= P);   // every probe row in some wavefront's chunk
                CHECK(g.tiles_per_wave <= 0xFFFFFFFFull);
              }
            }
        }
  }
  // the cap on a wavefront's tiles holds while the rounds are whole
  const ProbeKernel k = choose_probe_kernel(JOIN_LAYOUT_REGIONS, 1ull << 30, 1, 0, 1, true, 256);
  for (uint64_t tpw_max : {1ull, 12ull, 32ull}) CHECK(probe_grid(1ull << 30, k, cus, 8, tpw_max).tiles_per_wave <= tpw_max);
}

// ---------------------------------------------------------------- keys
static qhip_expr column_expr(int column) {
  qhip_expr e;
  memset(&e, 0, sizeof e);   // (the keys read the PODs as bytes, padding included)
  e.kind = QHIP_EXPR_COLUMN; e.column = column; e.left = e.right = e.third = -1;
  return e;
}
static qhip_expr utf8_literal(const char* bytes, int64_t len) {
  qhip_expr e;
  memset(&e, 0, sizeof e);
  e.kind = QHIP_EXPR_LITERAL; e.column = -1; e.left = e.right = e.third = -1;
  e.dtype.id = QHIP_UTF8;
  e.lit_str = bytes; e.lit_len = len;
  return e;
}

struct Keys { uint64_t dup, size; std::string plan; };
static Keys keys_of(const std::vector<qhip_expr>& lex, const std::vector<qhip_expr>& rex, int32_t on_l, int32_t on_r, int join_type, int lpred) {
  std::vector<InputCol> lcols(2), rcols(2);
  for (auto* cols : {&lcols, &rcols})
    for (auto& ic : *cols) ic.type = DType(QHIP_UTF8);
  Keys k;
  k.dup = join_dup_hint(5000, lpred, lex.data(), (int)lex.size(), &on_l, 1);
  k.size = join_size_key(5000, 70000, join_type, lpred, -1, lex.data(), (int)lex.size(), rex.data(), (int)rex.size(), &on_l, &on_r, 1);
  k.plan = join_plan_key(lcols, rcols, lex.data(), (int)lex.size(), rex.data(), (int)rex.size(), &on_l, &on_r, 1, lpred, -1, true, false, false);
  return k;
}

static void test_keys() {
  const std::string s1 = "BUILDING", s2 = "BUILDING", s3 = "BUILDINH";   // s1 / s2: equal bytes at two addresses
  CHECK(s1.data() != s2.data());
  const std::vector<qhip_expr> rex = {column_expr(0), column_expr(1)};
  auto lex_with = [&](const std::string& s) { return std::vector<qhip_expr>{column_expr(0), column_expr(1), utf8_literal(s.data(), (int64_t)s.size())}; };
  const Keys base = keys_of(lex_with(s1), rex, 0, 0, QHIP_JOIN_INNER, 2);
  const Keys same = keys_of(lex_with(s2), rex, 0, 0, QHIP_JOIN_INNER, 2);
  CHECK(base.dup == same.dup && base.size == same.size && base.plan == same.plan);
  const Keys other_byte = keys_of(lex_with(s3), rex, 0, 0, QHIP_JOIN_INNER, 2);
  CHECK(base.dup != other_byte.dup && base.size != other_byte.size && base.plan != other_byte.plan);
  const Keys other_on = keys_of(lex_with(s1), rex, 1, 0, QHIP_JOIN_INNER, 2);
  CHECK(base.dup != other_on.dup && base.size != other_on.size && base.plan != other_on.plan);
  const Keys other_pred = keys_of(lex_with(s1), rex, 0, 0, QHIP_JOIN_INNER, -1);
  CHECK(base.dup != other_pred.dup && base.size != other_pred.size && base.plan != other_pred.plan);
  // the join type is part of the join's size key only: the build side's hint and the lowered key plans do not depend on it
  const Keys other_type = keys_of(lex_with(s1), rex, 0, 0, QHIP_JOIN_LEFT, 2);
  CHECK(base.size != other_type.size && base.dup == other_type.dup && base.plan == other_type.plan);
  // the hash arithmetic itself: FNV-1a over the POD with the pointer left out, the literal bytes behind it
  const qhip_expr lit = utf8_literal(s1.data(), (int64_t)s1.size());
  qhip_expr bare = lit;
  bare.lit_str = nullptr;
  uint64_t h = 7 * 0x9E3779B97F4A7C15ULL + 1;
  for (size_t i = 0; i < sizeof bare; ++i) { h ^= ((const unsigned char*)&bare)[i]; h *= 1099511628211ULL; }
  for (unsigned char ch : s1) { h ^= ch; h *= 1099511628211ULL; }
  const int32_t on0 = 3;
  CHECK(join_dup_hint(7, 0, &lit, 1, &on0, 1) == h * 1099511628211ULL + 3);
  // the plan key's byte stream: "join|" + 8 ints per column + "|" per side, then the expressions
  const Keys k = keys_of({column_expr(0)}, {column_expr(0)}, 0, 0, QHIP_JOIN_INNER, -1);
  CHECK(k.plan.size() == 5 + 2 * (2 * 8 * sizeof(int) + 1) + 2 * (sizeof(qhip_expr) + 1) + 2 * sizeof(int32_t) + 5 * sizeof(int));
  CHECK(k.plan.compare(0, 5, "join|") == 0);
}

int main() {
  test_region_geometry_table();
  test_probe_shape_table();
  test_dense_rules();
  test_layout_invariants();
  test_probe_invariants();
  test_keys();
  printf("join_shape_tests: %d checks, %d failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
