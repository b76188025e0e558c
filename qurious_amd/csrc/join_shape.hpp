// join_shape.hpp — the hash join's arithmetic: which table layout applies, how big its parts are and where they lie in the
// arena, the probe kernel and its launch shape, and the keys under which a join's hints and lowered plan are remembered.
// These numbers decide whether a kernel stays within LDS, within its entry buffers and within its per-chunk counters. Plain
// host code: no HIP runtime call, no Ctx, no DevBuf and no environment (tuning values come in as arguments), so all of it
// runs (and is tested, tests/cpp/join_shape_tests.cpp) without a GPU. join.cpp is the only caller.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "common.hpp"
#include "expr.hpp"

namespace qhip {

// ---- the dense (direct-address) layout: an exact bitmap over the build key's range [kmin, kmax] + row_of[key - kmin]
struct DenseRange { bool candidate = false; uint64_t dense_n = 0; };   // dense_n = values in the range (candidate only)
// mode = QHIP_JOIN_DENSE (0 never, 1 when the range is within 256x the build rows, 2 whenever the key qualifies);
// kmax >= kmin; max_span_bits as clamped by the tuning (16..30)
DenseRange dense_range_rule(int mode, uint64_t B, int64_t kmin, int64_t kmax, int max_span_bits);
// automatic mode of the sorted dense build: the bitmap words must not outnumber what the workgroups may own on average
bool sorted_build_fits(uint64_t dense_n, uint64_t B);
struct DenseBuildForm { bool sorted = false, rank = false; };
// sorted_mode = QHIP_JOIN_DENSE_SORTED (0 never, 1 when the build key is known strictly ascending and the words fit, 2 whenever
// the dense layout applies); known_unsorted: this build side was found out of order before; every_row_inserted: no fused
// scan filter and no NULL keys (then the rank form: no row_of[] at all)
DenseBuildForm dense_build_form(bool dense, bool bytemap_wanted, int sorted_mode, bool key_asc, uint64_t dense_n, uint64_t B, bool known_unsorted,
                                bool every_row_inserted);

// ---- the region layout: the table cut into regions of 2^slot_bits slots that k_join_region_build assembles in LDS
struct RegionGeometry {
  uint32_t n_regions = 0, slot_bits = 0, bword_bits = 0;   // n_regions == 0: the legacy layout (one table, atomics)
  uint64_t load_pct = 0;                                   // a region holds at most this share of its slots
  size_t lds_bytes(int W) const { return (((size_t)8 * (1 + (size_t)W)) << slot_bits) + ((size_t)8 << bword_bits); }   // a region's image + its filter slice
};
// region_mode = QHIP_JOIN_REGION (0 never, 1 when it pays, 2 always); regions only while unique build keys are assumed
bool regions_wanted(bool dense, bool speculate, uint64_t B, int region_mode);
// W key words; scan_filter: a fused scan filter keeps only part of the build rows; load = QHIP_JOIN_REGION_LOAD (percent, clamped
// to 25..80); slot_bits_override = QHIP_JOIN_REGION_SLOT_BITS (>= 4 to count)
RegionGeometry region_geometry(uint64_t B, int W, bool scan_filter, const EnvInt& load, int slot_bits_override);

// ---- one arena: [table | count | filter]
enum JoinLayout { JOIN_LAYOUT_LEGACY = 0, JOIN_LAYOUT_REGIONS, JOIN_LAYOUT_DENSE, JOIN_LAYOUT_DENSE_RANK };
struct TableSizes {
  uint32_t dense_words = 0;    // 32-bit words of the dense layout's bitmap
  uint32_t nslots = 0;         // slots of the hashed table (dense: 0)
  uint32_t filter_words = 0;   // 64-bit words of the hash filter (dense: 0)
  size_t table_bytes = 0, count_bytes = 0, bloom_bytes = 0;
  size_t count_offset() const { return table_bytes; }
  size_t bloom_offset() const { return table_bytes + count_bytes; }
  size_t arena_bytes() const { return table_bytes + count_bytes + bloom_bytes; }
};
TableSizes table_sizes(JoinLayout layout, uint64_t B, int W, uint64_t dense_n, const RegionGeometry& g);
// step 1 of the region build (qk_join_scatter): workgroups and the rows each owns; B > 0, max_wgs >= 1
struct ScatterShape { uint64_t wgs = 0, rows_per_wg = 0; };
ScatterShape scatter_shape(uint64_t B, uint64_t max_wgs);

// ---- the probe: which kernel, and its launch shape
struct ProbeKernel {
  const char* name = nullptr;
  uint64_t tile_rows = 0;      // one wavefront's tile: 64 * PROBE_R consecutive probe rows
  uint32_t lds_words = 0;      // bitmap words staged in LDS (the LDS / hybrid variants)
  unsigned waves_per_wg = 4;
  uint32_t stage_cap = 0;      // dense layout: entries a wavefront stages in LDS
  size_t dyn_lds = 0;
};
// lds_mode = QHIP_JOIN_DENSE_LDS, wide = QHIP_JOIN_DENSE_WIDE, stage_extra = QHIP_DENSE_STAGE_EXTRA
ProbeKernel choose_probe_kernel(JoinLayout layout, uint64_t P, int probe_r, uint32_t dense_words, int lds_mode, bool wide, uint32_t stage_extra);
struct ProbeGrid { uint64_t tiles_per_wave = 0; unsigned grid = 0; uint64_t nchunks = 0; };
// wgs_per_cu: the occupancy of the loaded kernel at k.dyn_lds; tpw_max = QHIP_PROBE_TILES_PER_WAVE (>= 1)
ProbeGrid probe_grid(uint64_t P, const ProbeKernel& k, int num_cus, int wgs_per_cu, uint64_t tpw_max);

// ---- keys. Expression PODs are walked with their literal bytes appended and the lit_str pointer left out
// the build side by its key / filter expressions and row count (duplicate keys? out of order?)
uint64_t join_dup_hint(uint64_t B, int lpred, const qhip_expr* lex, int nlex, const int32_t* on_l, int n_on);
// the join as a whole (deferred sizing); build_rows = 0 when they are themselves a capacity
uint64_t join_size_key(uint64_t build_rows, uint64_t P, int join_type, int lpred, int rpred, const qhip_expr* lex, int nlex, const qhip_expr* rex,
                       int nrex, const int32_t* on_l, const int32_t* on_r, int n_on);
// the lowered key plans of both sides in the context's plan cache
std::string join_plan_key(const std::vector<InputCol>& lcols, const std::vector<InputCol>& rcols, const qhip_expr* lex, int nlex, const qhip_expr* rex,
                          int nrex, const int32_t* on_l, const int32_t* on_r, int n_on, int lpred, int rpred, bool want_regions, bool build_rows_on_device,
                          bool dense);

}  // namespace qhip
