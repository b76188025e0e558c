// join_shape.cpp — see join_shape.hpp: the hash join's layout, size and launch-shape arithmetic and its hint / plan keys.
#include "join_shape.hpp"

#include <algorithm>

#include "kargs_host.hpp"

namespace qhip {

// ---------------------------------------------------------------- dense layout
DenseRange dense_range_rule(int mode, uint64_t B, int64_t kmin, int64_t kmax, int max_span_bits) {
  DenseRange d;
  if (mode == 0 || B == 0) return d;
  const uint64_t span = (uint64_t)kmax - (uint64_t)kmin;   // (kmax >= kmin; the difference fits 64 unsigned bits)
  // automatic mode: the bitmap at most 32 bytes per build row AND the table bounded in absolute terms — row_of is 4 bytes per
  // VALUE of the range (span < 2^28: at most 1 GB beside a 32 MB bitmap; Q3's join 2 at SF100: 600 M values would be 2.4 GB
  // for 15 M build rows — the hashed layouts take over there). Whatever the mode, an allocation that fails falls back to
  // the hashed layouts instead of failing the query.
  const uint64_t max_span = (uint64_t)1 << max_span_bits;
  if (span < (1ULL << 30) && (mode == 2 || (span < 256 * B + 65536 && span < max_span))) { d.candidate = true; d.dense_n = span + 1; }
  return d;
}

// (automatic mode: not when the bitmap words outnumber what the workgroups may own even on average — a subset of a much
// wider column; the kernel's own cap catches the uneven cases)
bool sorted_build_fits(uint64_t dense_n, uint64_t B) {
  return (dense_n + 31) / 32 <= std::max<uint64_t>(1, (B + kSortedBuildRows - 1) / kSortedBuildRows) * kSortedMaxWords;
}

// The sorted form of the dense build (no atomics, no memset; the build keys' order is verified by the kernel and a build
// side found out of order is remembered by dup_hint and runs the atomic build from then on). QHIP_JOIN_DENSE_SORTED: 0
// never, 1 when the build key is known strictly ascending (default), 2 whenever the dense layout applies (tests).
// Rank form when every build row is inserted (no fused scan filter, no NULL keys): no row_of[] at all.
DenseBuildForm dense_build_form(bool dense, bool bytemap_wanted, int sorted_mode, bool key_asc, uint64_t dense_n, uint64_t B, bool known_unsorted,
                                bool every_row_inserted) {
  DenseBuildForm f;
  f.sorted = dense && !bytemap_wanted && sorted_mode != 0 && (sorted_mode == 2 || (key_asc && sorted_build_fits(dense_n, B))) && !known_unsorted;
  f.rank = f.sorted && every_row_inserted;
  return f;
}

// ---------------------------------------------------------------- region layout
bool regions_wanted(bool dense, bool speculate, uint64_t B, int region_mode) {
  return !dense && speculate && B > 0 && (region_mode == 2 || (region_mode == 1 && B >= 2048));
}

RegionGeometry region_geometry(uint64_t B, int W, bool scan_filter, const EnvInt& load, int slot_bits_override) {
  RegionGeometry g;
  // region = the biggest power of two of slots within 32 KB of LDS (W = 1: 2048 slots); 64 KB when that keeps the
  // number of regions (two LDS counters each in qk_join_scatter) within 8192
  uint32_t slot_bits = 4;
  while (((size_t)16 * (1 + W) << slot_bits) <= 32 * 1024) ++slot_bits;
  // table load: 1/3 when every build row enters the table, 1/2 of the rows when a fused scan filter keeps only part of them
  // (measured on Q3's second join, 1.46 M rows: load 1/2 -> 1/3 build 88 -> 79 us, probe 221 -> 209 us — fewer collisions
  // in the LDS inserts, fewer filter bits set; 0.6 / 0.7 cost 101 / 141 and 248 / 325 us)
  uint64_t load_pct = (uint64_t)std::max(25, std::min(80, load.or_default(scan_filter ? 50 : 33)));
  auto regions_for = [&](uint32_t sb) { const uint64_t per = std::max<uint64_t>(1, ((1ull << sb) * load_pct) / 100); return (uint32_t)((B + per - 1) / per); };   // load <= load_pct %
  if (load_pct < 50 && regions_for(slot_bits) > 8192) load_pct = 50;   // (a big build side: rather load 1/2 than more than 8192 regions)
  if (slot_bits_override >= 4) slot_bits = (uint32_t)slot_bits_override;
  else if (regions_for(slot_bits) > 8192 && ((size_t)16 * (1 + W) << slot_bits) <= 60 * 1024) ++slot_bits;
  g.n_regions = regions_for(slot_bits);
  g.slot_bits = slot_bits;
  g.bword_bits = slot_bits - 3;   // 64-bit filter words per region: 8 filter bits per slot = >= 16 per key
  g.load_pct = load_pct;
  if (g.n_regions > 8192 || g.lds_bytes(W) > 64 * 1024) g.n_regions = 0;
  return g;
}

// ---------------------------------------------------------------- table sizes
// one arena: [table | count | filter] (legacy: zero-filled; region layout: every byte of table and filter is stored by
// k_join_region_build, the counts are not used)
// (dense layout: table = u32 row_of[dense_n], never initialised — read only where the bitmap says a key is there; "filter"
// = the exact bitmap, the only part that is cleared)
// (rank form of the sorted dense build: table = u32 rank[dense_words] instead of row_of)
TableSizes table_sizes(JoinLayout layout, uint64_t B, int W, uint64_t dense_n, const RegionGeometry& g) {
  TableSizes z;
  const bool dense = layout == JOIN_LAYOUT_DENSE || layout == JOIN_LAYOUT_DENSE_RANK, regions = layout == JOIN_LAYOUT_REGIONS;
  z.dense_words = dense ? (uint32_t)((dense_n + 31) / 32) : 0;
  z.nslots = dense ? 0 : regions ? g.n_regions << g.slot_bits : std::max<uint32_t>(16, pow2_ceil32(B * 2));
  // hash filter: 64-bit words, 8 bits per slot (region layout: 2^bword_bits words per region)
  z.filter_words = dense ? 0 : regions ? g.n_regions << g.bword_bits : std::max<uint32_t>(16, z.nslots / 8);
  z.table_bytes = layout == JOIN_LAYOUT_DENSE_RANK ? ((size_t)z.dense_words * 4 + 127) / 128 * 128
                  : dense                          ? ((size_t)dense_n * 4 + 127) / 128 * 128
                                                   : (size_t)z.nslots * (1 + (size_t)W) * 8;
  z.count_bytes = (regions || dense) ? 0 : (((size_t)z.nslots + 2) * 4 + 7) / 8 * 8;
  z.bloom_bytes = dense ? ((size_t)z.dense_words * 4 + 127) / 128 * 128 : (size_t)z.filter_words * 8;
  return z;
}

// a step-1 workgroup (1024 threads) owns a row range of two or three rows per thread when the rows allow (2
// workgroups per CU); its entries stay inside the range, so nothing is shared between workgroups
ScatterShape scatter_shape(uint64_t B, uint64_t max_wgs) {
  ScatterShape sc;
  sc.wgs = std::max<uint64_t>(1, std::min<uint64_t>((B + 2047) / 2048, max_wgs));
  sc.rows_per_wg = (((B + sc.wgs - 1) / sc.wgs) + 63) / 64 * 64;
  sc.wgs = (B + sc.rows_per_wg - 1) / sc.rows_per_wg;
  return sc;
}

// ---------------------------------------------------------------- probe shape
// which probe kernel (the table layout is a template parameter of the generated kernel). Dense layout: probe sides of
// less than one tile run the general kernel; else a lane owns consecutive rows (16-byte column loads,
// QHIP_JOIN_DENSE_WIDE=0: not), and QHIP_JOIN_DENSE_LDS stages the bitmap in LDS: 1 = when all of it fits the CU's
// 160 KB, the hybrid kernel (first 160 KB in LDS, the rest through L2) up to four times that; 2 = hybrid always
ProbeKernel choose_probe_kernel(JoinLayout layout, uint64_t P, int probe_r, uint32_t dense_words, int lds_mode, bool wide, uint32_t stage_extra) {
  ProbeKernel k;
  const bool dense = layout == JOIN_LAYOUT_DENSE || layout == JOIN_LAYOUT_DENSE_RANK;
  k.tile_rows = (uint64_t)64 * (uint64_t)probe_r;   // one wavefront's tile: 64 * P::PROBE_R consecutive probe rows
  // LDS staging of the dense probe's entries: per wavefront, at least one tile's worth behind the flush threshold
  const uint32_t stage_cap_small = (uint32_t)k.tile_rows + stage_extra, stage_cap_lds = (uint32_t)k.tile_rows + 128;
  const uint32_t kLdsWords = (160 * 1024 - 16 * 2 * 4 * stage_cap_lds) / 4 - 2;   // what the 16 wavefronts' staging areas leave of the CU's 160 KB
  // QHIP_JOIN_DENSE_LDS: 0 never, 1 (default) when at least half of the bitmap fits the CU's LDS and the probe side is
  // big enough to pay for every workgroup's copy of it, 2 always (tests). Measured on Q3 SF10's first join (15 M orders
  // probing 1.5 M customer keys at random, 188 KB of bitmap, 60 % of it staged): 55-59 us against 72-80 us through L1 / L2
  // — a random 4-byte lookup drags a 128-byte line from L2 into L1; the second join's bitmap (7.5 MB, read in key order
  // by lineitem) gains nothing from LDS.
  k.name = layout == JOIN_LAYOUT_REGIONS ? "qk_join_probe" : "qk_join_probe_onetable";
  if (dense) {
    k.name = "qk_join_probe_dense";
    if (P >= k.tile_rows) {
      if (wide) k.name = "qk_join_probe_dense_wide";
      const bool pays = lds_mode == 2 || (lds_mode == 1 && P >= (1u << 20) && P >= 32ull * std::min(dense_words, kLdsWords) && dense_words <= 2 * kLdsWords);
      if (pays && dense_words <= kLdsWords) { k.name = "qk_join_probe_dense_lds"; k.lds_words = dense_words; }
      else if (pays) { k.name = "qk_join_probe_dense_hybrid"; k.lds_words = kLdsWords; }
    }
  }
  const bool dense_lds = k.lds_words > 0;
  k.waves_per_wg = dense_lds ? 16 : 4;
  k.stage_cap = !dense ? 0 : dense_lds ? stage_cap_lds : stage_cap_small;
  // dynamic LDS: [bitmap words of the LDS variants | per wavefront: stage_cap x (idx, row)] (dense layout only)
  k.dyn_lds = !dense ? 0 : (((size_t)k.lds_words + 1) & ~(size_t)1) * 4 + (size_t)k.waves_per_wg * 2 * 4 * k.stage_cap;
  return k;
}

// A wavefront owns a CHUNK of consecutive tiles; a chunk's matches are one run of entries with one count (the scan and
// pass 2 work per chunk). The grid is sized in whole ROUNDS of the wavefronts the chip holds at once (occupancy of the
// loaded kernel x CUs), each wavefront with at most QHIP_PROBE_TILES_PER_WAVE (32) tiles: a wavefront pays ~two extra
// trips to fill its pipeline whatever its chunk, and a last round that fills a third of the chip costs a whole round
// (round 2 gave every wavefront 12 tiles: Q3's lineitem probe ran 2.4 rounds at 12 / 14 pipeline efficiency — 63 % of the
// 6.5 TB/s a bare kernel with the same access pattern reaches, tools/micro/stream_widths.hip).
ProbeGrid probe_grid(uint64_t P, const ProbeKernel& k, int num_cus, int wgs_per_cu, uint64_t tpw_max) {
  ProbeGrid g;
  const uint64_t ntiles = std::max<uint64_t>(1, (P + k.tile_rows - 1) / k.tile_rows);   // (the join probes only P > 0: at least one tile)
  const uint64_t resident = (uint64_t)num_cus * (uint64_t)wgs_per_cu * k.waves_per_wg;   // wavefronts the chip runs at once
  const uint64_t rounds = std::max<uint64_t>(1, (ntiles + resident * tpw_max - 1) / (resident * tpw_max));
  const uint64_t waves_wanted = std::min<uint64_t>(ntiles, rounds * resident);
  g.tiles_per_wave = (ntiles + waves_wanted - 1) / waves_wanted;
  g.grid = (unsigned)std::max<uint64_t>(1, ((ntiles + g.tiles_per_wave - 1) / g.tiles_per_wave + k.waves_per_wg - 1) / k.waves_per_wg);
  g.nchunks = (uint64_t)g.grid * k.waves_per_wg;
  return g;
}

// ---------------------------------------------------------------- keys
namespace {
// every expression POD without its lit_str pointer, a literal's bytes behind it: sink(bytes, n)
template <class Sink> void walk_exprs(const qhip_expr* ex, int n, Sink&& sink) {
  for (int k = 0; k < n; ++k) {
    qhip_expr e = ex[k];
    const char* str = e.lit_str;
    e.lit_str = nullptr;
    sink((const char*)&e, sizeof e);
    if (str && e.lit_len > 0 && e.kind == QHIP_EXPR_LITERAL) sink(str, (size_t)e.lit_len);
  }
}
uint64_t fold_exprs(uint64_t h, const qhip_expr* ex, int n) {   // FNV-1a over the walk
  walk_exprs(ex, n, [&](const char* p, size_t len) { for (size_t i = 0; i < len; ++i) { h ^= (unsigned char)p[i]; h *= 1099511628211ULL; } });
  return h;
}
}  // namespace

uint64_t join_dup_hint(uint64_t B, int lpred, const qhip_expr* lex, int nlex, const int32_t* on_l, int n_on) {
  uint64_t h = fold_exprs(B * 0x9E3779B97F4A7C15ULL + (uint64_t)(lpred + 1), lex, nlex);
  for (int k = 0; k < n_on; ++k) h = h * 1099511628211ULL + (uint64_t)on_l[k];
  return h;
}

uint64_t join_size_key(uint64_t build_rows, uint64_t P, int join_type, int lpred, int rpred, const qhip_expr* lex, int nlex, const qhip_expr* rex,
                       int nrex, const int32_t* on_l, const int32_t* on_r, int n_on) {
  uint64_t h = build_rows * 0x9E3779B97F4A7C15ULL + P * 0xD6E8FEB86659FD93ULL + ((uint64_t)(join_type + 1) << 56) + ((uint64_t)(lpred + 1) << 20) +
               (uint64_t)(rpred + 1);
  h = fold_exprs(fold_exprs(h, lex, nlex), rex, nrex);
  for (int k = 0; k < n_on; ++k) h = (h * 1099511628211ULL + (uint64_t)on_l[k]) * 1099511628211ULL + (uint64_t)on_r[k];
  return h;
}

std::string join_plan_key(const std::vector<InputCol>& lcols, const std::vector<InputCol>& rcols, const qhip_expr* lex, int nlex, const qhip_expr* rex,
                          int nrex, const int32_t* on_l, const int32_t* on_r, int n_on, int lpred, int rpred, bool want_regions, bool build_rows_on_device,
                          bool dense) {
  std::string pkey = "join|";
  auto put = [&](const void* p, size_t n) { pkey.append((const char*)p, n); };
  for (const std::vector<InputCol>* cols : {&lcols, &rcols}) {
    for (auto& ic : *cols) {
      const int v[8] = {ic.type.id, ic.type.precision, ic.type.scale, ic.has_nulls ? 1 : 0, ic.utf8_max_len, ic.utf8_fixed1 ? 1 : 0, ic.indirect ? 1 : 0, ic.narrow_bytes};
      put(v, sizeof v);
    }
    put("|", 1);
  }
  walk_exprs(lex, nlex, put); put("|", 1);
  walk_exprs(rex, nrex, put); put("|", 1);
  put(on_l, sizeof(int32_t) * (size_t)n_on);
  put(on_r, sizeof(int32_t) * (size_t)n_on);
  const int v[5] = {lpred, rpred, want_regions ? 1 : 0, build_rows_on_device ? 1 : 0, dense ? 1 : 0};
  put(v, sizeof v);
  return pkey;
}

}  // namespace qhip
