// join.cpp — qhip_hash_join_execute: HashJoinExec::execute (physical/plan/join/hash_join.rs:354-384).
//
//   build (left, hash_join.rs:148-175)    key words (JIT) -> open-addressing table of distinct keys + a one-bit-per-hash
//                                          filter (stays in L2) -> unique keys: slot -> row; duplicated keys: rows grouped by
//                                          slot with a stable radix sort (ascending build row inside a key, the order the
//                                          reference's reverse-built chains yield) -> CSR start/count per slot
//   probe (right, hash_join.rs:218-275)   pass 1 (JIT): fused scan filter + key words + lookup straight from the probe
//                                          table's columns -> slot per probe row, pair count per 256-row tile -> scan
//                                          -> pass 2: (build, probe) pairs in probe-row order
//                                          [-> residual JoinFilter on an intermediate batch, join/mod.rs:125-154]
//                                          -> visited bitmap -> Right/Full NULL padding (join/mod.rs:176-207)
//   output (utils/batch.rs:18-61)         every column gathered by the index vectors; one batch per non-empty probe batch,
//                                          then the unmatched-build / semi tail batch (hash_join.rs:277-343, 374-381)
// All probe batches are probed in one launch; batch boundaries are recovered from the pairs' (ascending) probe rows.
//
// hash_join (the driver, at the end of the file) is the operator's outline: a loop over ATTEMPTS, every stage a function of
// this file. A stage that finds that the attempt cannot go on returns why (Repeat) and the driver starts the next one from the top:
//    0  maybe_encode_wide_join_key   (once, in front of the driver) a key that does not fit the packed key words: one shared
//                                  key code per row of either side, then the driver below on the codes
//    1  validate_join_args
//    2  choose_dense_candidate     the build key's range: direct-address table?
//    3  resolve_join_inputs        deferred columns, Utf8 key lengths of both sides, narrow copies; check_scan_filters
//    4  decide_speculation         dup_hint / size_key, unique keys assumed?, sorted dense build?, regions?, deferred size?
//    5  lookup_or_lower_plan       plan cache (JoinPlan)
//    6  choose_table_layout        region geometry (join_shape.cpp);  settle_build_side -> Repeat::SettleBuild
//    7  allocate_table             sizes and arena carving (join_shape.cpp) -> Repeat::DenseDoesNotFit
//    8  build_dense_sorted | build_dense | build_regions | build_legacy_insert
//    9  read_build_status          (only without speculation);  build_csr for duplicated keys
//   10  launch_probe               kernel and launch shape (join_shape.cpp), pass 1, scan of the chunk totals
//   11  emit_deferred | read_probe_status -> Repeat::BuildOutOfOrder / DuplicateBuildKeys, emit_waited    (emit_pairs: pass 2)
//   12  apply_residual_filter, mark_visited_and_count, pad_right_rows, select_tail
//   13  concat_index_vectors, make_output_columns, set_batch_offsets, set_join_stats
// JoinArgs holds the call's parameters, JoinTuning every environment switch (read once per attempt), JoinCall what is fixed
// once the layout is chosen, JoinRun what the build and the probe produce for the stages behind them. The arithmetic that keeps
// the kernels within LDS, their entry buffers and their per-chunk counters is join_shape.cpp (tests/test_join_shape_cpu.py).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <map>

#include "common.hpp"
#include "device/qhip_status.h"
#include "jit.hpp"
#include "join_shape.hpp"
#include "kargs_host.hpp"
#include "kernels.hpp"
#include "relops.hpp"

using namespace qhip;

namespace {

uint32_t read_u32(hipStream_t s, const void* dev) {
  uint32_t v = 0;
  copy_sync(s, &v, dev, 4, hipMemcpyDeviceToHost);
  return v;
}

// ---------------------------------------------------------------- the operator's state
struct JoinArgs {
  const qhip_table *L, *R;
  int join_type;
  const qhip_expr* lex; int nlex;   // build side: key / scan-filter expressions
  const qhip_expr* rex; int nrex;   // probe side
  const int32_t *on_l, *on_r; int n_on;
  const qhip_expr* fex; int nfex, froot;   // residual JoinFilter (froot < 0: none) over the intermediate batch of
  const int32_t *fsides, *fcols; int nfcols;   // columns fcols[k] of side fsides[k] (0 = build)
  int lpred, rpred;                 // fused scan filters (roots in lex / rex, < 0: none)
};

// Every environment switch of the join, read ONCE at the top of an attempt (per attempt: tests flip them between executions of
// one process). Nothing below read_join_tuning looks at the environment.
struct JoinTuning {
  int dense_mode;             // QHIP_JOIN_DENSE 0 never / 1 when the key range is within 256x the build rows / 2 whenever the key qualifies (policy; 2 = tests)
  int dense_max_span_bits;    // QHIP_JOIN_DENSE_MAX_SPAN_BITS (16..30): automatic mode's absolute bound of the key range (policy)
  EnvInt late_gather_build;   // QHIP_LATE_GATHER_BUILD: the build key read through a deferred gather's index vector; default: dense candidates only (measurement)
  int64_t stats_min_rows;     // QHIP_STATS_MIN_ROWS: inputs from this size collect column statistics (policy; tests / the fuzzer lower it)
  bool force_csr;             // QHIP_JOIN_FORCE_CSR=1: the CSR layout even for unique build keys, no speculation (test forcing)
  bool speculation;           // QHIP_JOIN_NO_SPECULATION=1 switches the assumption of unique build keys off (test forcing)
  int region_mode;            // QHIP_JOIN_REGION 0 never / 1 when it pays / 2 always: the LDS-staged region build (policy; 2 = tests)
  int sorted_mode;            // QHIP_JOIN_DENSE_SORTED 0 never / 1 build key known ascending / 2 whenever dense: the sorted dense build (policy; 2 = tests)
  bool bytemap;               // QHIP_JOIN_DENSE_BYTEMAP=1: the byte-map form of the dense build (measured slower; kept as a tested switch)
  int bytemap_max_bits;       // QHIP_JOIN_DENSE_BYTEMAP_MAX_BITS (10..30): largest key range of that form (test forcing)
  bool defer;                 // QHIP_JOIN_NO_DEFER=1 switches deferred sizes off: every join waits for its pair total (test forcing)
  EnvInt region_load;         // QHIP_JOIN_REGION_LOAD (25..80 percent): load of the region tables; default 50 behind a build-side scan filter, else 33 (measurement)
  int region_slot_bits;       // QHIP_JOIN_REGION_SLOT_BITS (>= 4 to count): slots per region (test forcing)
  EnvInt scatter_wgs;         // QHIP_JOIN_SCATTER_WGS (>= 1): workgroups of the region build's step 1; default two per CU (measurement)
  bool key_materialize;       // QHIP_JOIN_KEY_MATERIALIZE=0: the join key of an Inner dense join is gathered like every other column (measurement)
  uint32_t stage_extra;       // QHIP_DENSE_STAGE_EXTRA (>= 0): LDS staging entries per wavefront beyond one tile, dense probe (measurement)
  int dense_lds;              // QHIP_JOIN_DENSE_LDS 0 never / 1 when it pays / 2 always: the dense probe's bitmap staged in LDS (policy; 2 = tests)
  bool dense_wide;            // QHIP_JOIN_DENSE_WIDE=0: never the consecutive-rows dense probe (test forcing)
  uint64_t probe_tiles_per_wave;   // QHIP_PROBE_TILES_PER_WAVE (>= 1): most tiles a probe wavefront owns (measurement)
  bool eager_gather;          // QHIP_EAGER_GATHER=1: output columns gathered at once, not when first read (test forcing)
  bool eager_offsets;         // QHIP_EAGER_OFFSETS=1: the output's batch offsets fetched at once (test forcing)
  int wide_keys;              // QHIP_JOIN_WIDE_KEYS 0 never / 1 when the packed key does not fit / 2 every hash join over plain key columns:
                              // keys of both sides encoded to shared key codes first (policy, off; 2 = tests) — the context's own mode goes first
  int wide_key_hash_bits;     // QHIP_JOIN_WIDE_KEY_HASH_BITS (1..63): only so many bits of the encoding's hash (test forcing: long probe chains)
  bool lazy_index;            // QHIP_JOIN_LAZY_INDEX=0: pass 2 always looks the build rows up and writes the key column (measurement; relops.cpp reads it for the compositions)
  bool fold_scan;             // QHIP_JOIN_FOLD_SCAN=0: a deferred-size join scans its chunk counters in a launch of its own, as every other join does (measurement)
  uint64_t fold_max_chunks;   // QHIP_JOIN_FOLD_SCAN_MAX_CHUNKS (0..8192): most chunks pass 2 sums by itself (test forcing: the separate scan above it)
};
JoinTuning read_join_tuning() {
  JoinTuning t;
  t.dense_mode = env_int("QHIP_JOIN_DENSE", 1);
  t.dense_max_span_bits = std::max(16, std::min(30, env_int("QHIP_JOIN_DENSE_MAX_SPAN_BITS", 28)));
  t.late_gather_build = env_opt("QHIP_LATE_GATHER_BUILD");
  t.stats_min_rows = (int64_t)env_int("QHIP_STATS_MIN_ROWS", 1 << 22);
  t.force_csr = env_int("QHIP_JOIN_FORCE_CSR", 0) != 0;
  t.speculation = env_int("QHIP_JOIN_NO_SPECULATION", 0) == 0;
  t.region_mode = env_int("QHIP_JOIN_REGION", 1);
  t.sorted_mode = env_int("QHIP_JOIN_DENSE_SORTED", 1);
  t.bytemap = env_int("QHIP_JOIN_DENSE_BYTEMAP", 0) != 0;
  t.bytemap_max_bits = std::max(10, std::min(30, env_int("QHIP_JOIN_DENSE_BYTEMAP_MAX_BITS", 27)));
  t.defer = env_int("QHIP_JOIN_NO_DEFER", 0) == 0;
  t.region_load = env_opt("QHIP_JOIN_REGION_LOAD");
  t.region_slot_bits = env_int("QHIP_JOIN_REGION_SLOT_BITS", 0);
  t.scatter_wgs = env_opt("QHIP_JOIN_SCATTER_WGS");
  t.key_materialize = env_int("QHIP_JOIN_KEY_MATERIALIZE", 1) != 0;
  t.stage_extra = (uint32_t)std::max(0, env_int("QHIP_DENSE_STAGE_EXTRA", 256));
  t.dense_lds = env_int("QHIP_JOIN_DENSE_LDS", 1);
  t.dense_wide = env_int("QHIP_JOIN_DENSE_WIDE", 1) != 0;
  t.probe_tiles_per_wave = (uint64_t)std::max(1, env_int("QHIP_PROBE_TILES_PER_WAVE", 32));
  t.eager_gather = env_int("QHIP_EAGER_GATHER", 0) != 0;
  t.eager_offsets = env_int("QHIP_EAGER_OFFSETS", 0) != 0;
  t.wide_keys = env_int("QHIP_JOIN_WIDE_KEYS", 0);
  t.wide_key_hash_bits = env_int("QHIP_JOIN_WIDE_KEY_HASH_BITS", 0);
  t.lazy_index = env_int("QHIP_JOIN_LAZY_INDEX", 1) != 0;
  t.fold_scan = env_int("QHIP_JOIN_FOLD_SCAN", 1) != 0;
  t.fold_max_chunks = (uint64_t)std::max(0, std::min(QH_JOIN_FOLD_MAX_CHUNKS, env_int("QHIP_JOIN_FOLD_SCAN_MAX_CHUNKS", QH_JOIN_FOLD_MAX_CHUNKS)));
  return t;
}

// the lowered key plans of both sides (typing + generated source + loaded kernels), cached per context (lookup_or_lower_plan)
struct JoinPlan {
  KeysPlan lkp, rkp; std::shared_ptr<Module> lmod; std::map<std::string, std::shared_ptr<Module>> rmods; DevBuf lstr, rstr;   // (+ the string literals, uploaded once)
  // the dense build's byte map, kept between executions: bytes[key - min] = the execution's stamp (1..255), so that it is
  // cleared once in 255 executions instead of every time (8x the bitmap's bytes: 60 MB for Q3's join 2)
  std::shared_ptr<DevBuf> bytemap; uint64_t bytemap_n = 0; uint32_t bytemap_gen = 0;
  std::shared_ptr<Module> lmod_sorted;   // qk_join_dense_build_sorted of the build module
};

// why an attempt ends without a result; each reason is gone when the next attempt gets there (see hash_join)
enum class Repeat { No, SettleBuild, DenseDoesNotFit, BuildOutOfOrder, DuplicateBuildKeys };

// what is fixed once the table layout is chosen
struct JoinCall {
  uint64_t B = 0, P = 0;   // build / probe rows (a build side of deferred size: its capacity)
  bool semi_anti = false, pad_right = false, has_tail = false;
  bool want_pairs = false;      // not LeftSemi / LeftAnti without a residual filter: those only need the visited bits
  bool mark_in_probe = false;   // the probe marks the visited bits (with a residual filter only surviving pairs mark)
  bool dense_candidate = false, key_asc = false;
  int64_t kmin = 0, kmax = 0;
  uint64_t dense_n = 0;
  bool late_build = false;
  std::vector<InputCol> lcols, rcols;
  uint64_t dup_hint = 0, size_key = 0;
  bool speculate = false, dense = false, dense_sorted = false, dense_rank = false, want_regions = false, defer = false;
  uint64_t defer_cap = 0;
  std::shared_ptr<JoinPlan> jp;
  int W = 0;
  RegionGeometry geo;
  bool region_build = false;
  JoinLayout layout = JOIN_LAYOUT_LEGACY;
  TableSizes sz;
  // device status block of the call: [build status words | probe status words | pair total], read back once
  uint32_t* dstat = nullptr;
  // read-backs land in the context's page-locked scratch: a D2H copy into pageable memory is a stream round trip of its
  // own, so two of them plus the synchronize cost three waits where one does
  uint32_t* st_build = nullptr;   // pinned mirror of the device status block: [build | probe | pair total]
  uint32_t* st = nullptr;
};

// what the build and the probe produce
struct JoinRun {
  DevBuf arena;   // [table | count | filter]
  uint64_t* table = nullptr; uint32_t* count = nullptr; uint64_t* bloom = nullptr;
  DevBuf lkeys, lvalid, row_slot;   // legacy build: key words, their validity, the slot of every build row
  uint32_t max_count = 0;
  bool unique_keys = true;
  DevBuf start, sorted_rows;        // CSR of the build rows of every slot (duplicated keys)
  const uint32_t* start_ptr = nullptr; const uint32_t* rows_ptr = nullptr;
  DevBuf visited; bool visited_done = false;
  DevBuf ent_slot, ent_row, tile_tot, tile_nent;   // pass 1: (slot, probe row) per matching row; pair total / entries per chunk
  uint64_t nchunks = 0, tiles_per_wave = 0, chunk_rows = 0;
  bool fold_scan = false;   // tile_tot holds the chunks' pair counts, unscanned: pass 2 (of a deferred-size join) sums them itself
  std::string probe_name;   // (the entry point launched, for the statistics)
  bool probe_timed = false;
  DevBuf cnt, pair_off, b_idx, p_idx;   // pass 2: pairs per probe row and their first position (Right / Full); the pairs
  uint64_t M = 0;
  bool mat_key = false;
  // the build-side index vector is left as pass 1's dense key indices (key - min) and owed (LazyIndex, pending translation): pass 2
  // looked nothing up and wrote no key column. Decided before pass 2 (wants_lazy_build), true only if pass 2 took its pairs-only branch
  bool lazy_build = false;
  std::shared_ptr<DevBuf> key_vals;   // the join key of every output row (mat_key)
  std::shared_ptr<DevBuf> rows_blk; std::shared_ptr<uint64_t> rows_final; const uint32_t* deferred_slot = nullptr;   // deferred size
  DevBuf cnt2, off2, out_off;   // surviving pairs per probe row behind the residual filter, their scan; Right / Full: output positions
  const uint32_t* final_cnt = nullptr; const uint32_t* final_off = nullptr;
  uint64_t T = 0; DevBuf tail_sel;   // tail rows
  uint64_t total_rows = 0;
  std::shared_ptr<DevBuf> b_all, p_all;   // index vectors of the whole output: [pairs | tail]
};

// ---------------------------------------------------------------- stages
void validate_join_args(const JoinArgs& a) {
  if (a.n_on <= 0) fail(QHIP_INVALID_ARGUMENT, "Internal error: On constraints in HashJoinExec should be non-empty");
  if (a.join_type < QHIP_JOIN_LEFT || a.join_type > QHIP_JOIN_LEFT_ANTI) fail(QHIP_INVALID_ARGUMENT, "unknown join type");
  if (a.L->num_rows >= (int64_t)kNullIdx - 1 || a.R->num_rows >= (int64_t)kNullIdx - 1)
    fail(QHIP_UNSUPPORTED, "join inputs of 2^32 - 2 rows or more are not supported");
}

// the rows of both sides as the attempt finds them, and what the join type asks for
void set_join_type_flags(const JoinArgs& a, JoinCall& c) {
  c.B = (uint64_t)a.L->num_rows; c.P = (uint64_t)a.R->num_rows;
  c.semi_anti = a.join_type == QHIP_JOIN_LEFT_SEMI || a.join_type == QHIP_JOIN_LEFT_ANTI;
  c.pad_right = a.join_type == QHIP_JOIN_RIGHT || a.join_type == QHIP_JOIN_FULL;
  c.has_tail = a.join_type == QHIP_JOIN_LEFT || a.join_type == QHIP_JOIN_FULL || c.semi_anti;
  c.want_pairs = !(c.semi_anti && a.froot < 0);
  c.mark_in_probe = c.has_tail && a.froot < 0;
}

void check_scan_filters(const JoinArgs& a) {
  if ((a.lpred >= 0 || a.rpred >= 0) && a.join_type != QHIP_JOIN_INNER)
    fail(QHIP_INVALID_ARGUMENT, "fused scan filters are only defined for Inner joins (rows rejected by a filter must not surface as unmatched rows)");
  if (a.lpred >= a.nlex || a.rpred >= a.nrex) fail(QHIP_INVALID_ARGUMENT, "scan filter index out of range");
}

// ---- dense (direct-address) layout? ONE integer key column whose build-side values span a small range [kmin, kmax]
// (DevColumn::range, found once per base table: looked at BEFORE the key column is gathered, while a deferred gather
// still names its source): the table is then an exact bitmap over the range + row_of[key - kmin]
// (qh_join_dense_build_body / qh_join_probe_dense_body). QHIP_JOIN_DENSE: 0 never, 1 when the range is within 256x the
// build rows (default), 2 whenever the key qualifies (tests).
// (dense_off: this join is being run again after its dense table did not fit the device memory, see allocate_table)
void choose_dense_candidate(Ctx* ctx, const JoinArgs& a, const JoinTuning& t, bool dense_off, JoinCall& c) {
  const int dense_mode = dense_off ? 0 : t.dense_mode;
  const qhip_table* L = a.L;
  if (dense_mode != 0 && a.n_on == 1 && c.B > 0 && a.on_l[0] >= 0 && a.on_l[0] < a.nlex && a.lex[a.on_l[0]].kind == QHIP_EXPR_COLUMN &&
      a.lex[a.on_l[0]].column >= 0 && a.lex[a.on_l[0]].column < (int)L->cols.size()) {
    const DevColumn& kc = L->cols[(size_t)a.lex[a.on_l[0]].column];
    const int id = kc.type.id;
    if ((id == QHIP_INT64 || id == QHIP_INT32 || id == QHIP_UINT8 || id == QHIP_DATE32 || id == QHIP_DATE64 || (id >= QHIP_TIME32_S && id <= QHIP_TIME64_NS)) &&
        key_range_of(ctx, kc, c.kmin, c.kmax)) {
      const DenseRange d = dense_range_rule(dense_mode, c.B, c.kmin, c.kmax, t.dense_max_span_bits);
      c.dense_candidate = d.candidate;
      c.dense_n = d.dense_n;
      // strictly ascending build keys (found by the same reduction as the range, read through index vectors that keep the
      // order): the dense build can then store every bitmap word once, without atomics (qh_join_dense_build_sorted_body)
      c.key_asc = c.dense_candidate && key_ascending(ctx, kc);
    }
  }
}

// ---- key words of both sides (only the columns the key / scan-filter expressions read are gathered if deferred)
// (measured on Q3's second join: reading the build key through join 1's index vector inside qk_join_scatter costs 17 us
// more than the separate gather it saves — 92 vs 75 us — so the build side gathers; QHIP_LATE_GATHER_BUILD=1 switches it on)
void resolve_join_inputs(Ctx* ctx, const JoinArgs& a, const JoinTuning& t, JoinCall& c) {
  // the build key of a join over a join's output is a deferred gather: the dense build kernel reads it THROUGH the index
  // vector (one dependent load more per row, no gather launch + write + re-read of the key: Q3's join 2 24 + 38 -> 54 us);
  // the region build's scatter kernel lost by that (92 vs 75 us), so the hashed layouts gather first
  c.late_build = t.late_gather_build.or_default(c.dense_candidate ? 1 : 0) != 0;
  resolve_referenced(ctx, a.L, a.lex, a.nlex, c.late_build);
  resolve_referenced(ctx, a.R, a.rex, a.nrex);
  c.lcols = input_cols_of(a.L, c.late_build);
  c.rcols = input_cols_of(a.R);
  std::vector<InputCol>&lcols = c.lcols, &rcols = c.rcols;
  ensure_utf8_key_lengths(ctx, a.L, a.lex, a.nlex, a.on_l, a.n_on, lcols);
  ensure_utf8_key_lengths(ctx, a.R, a.rex, a.nrex, a.on_r, a.n_on, rcols);
  ensure_narrow_int_columns(ctx, a.R, a.rex, a.nrex, rcols, t.stats_min_rows);   // (the probe side streams its key column: 4 bytes where they do)
  // both sides must pack a Utf8 key into the same number of words
  for (int k = 0; k < a.n_on; ++k) {
    if (a.on_l[k] < 0 || a.on_l[k] >= a.nlex || a.on_r[k] < 0 || a.on_r[k] >= a.nrex) fail(QHIP_INVALID_ARGUMENT, "join key index out of range");
    const qhip_expr &le = a.lex[a.on_l[k]], &re = a.rex[a.on_r[k]];
    if (le.kind == QHIP_EXPR_COLUMN && re.kind == QHIP_EXPR_COLUMN && le.column >= 0 && le.column < (int)lcols.size() && re.column >= 0 &&
        re.column < (int)rcols.size() && lcols[(size_t)le.column].type.id == QHIP_UTF8 && rcols[(size_t)re.column].type.id == QHIP_UTF8) {
      const int m = std::max(lcols[(size_t)le.column].utf8_max_len, rcols[(size_t)re.column].utf8_max_len);
      lcols[(size_t)le.column].utf8_max_len = m;
      rcols[(size_t)re.column].utf8_max_len = m;
    }
  }
}

// The build's status (key-evaluation errors, duplicate keys?) is needed before the probe only to choose between the
// unique-key and the CSR layout. Unique keys are the rule (every FK -> PK join), so unless this build side is known to
// have had duplicates the probe is launched on that assumption and the build status is read together with the probe's:
// one host round trip less per join. A wrong guess is memory-safe (a slot's state word always names a valid build row),
// is detected below, remembered, and the join runs again the careful way.
// (the hint identifies the build side by its key / filter expressions and row count)
void decide_speculation(Ctx* ctx, const JoinArgs& a, const JoinTuning& t, JoinCall& c) {
  c.dup_hint = join_dup_hint(c.B, a.lpred, a.lex, a.nlex, a.on_l, a.n_on);
  c.speculate = !t.force_csr && t.speculation && !ctx->join_dup_builds.count(c.dup_hint);
  c.dense = c.dense_candidate && c.speculate;   // (unique build keys assumed and checked, like the region build)
  // (the sorted and the rank form of the dense build: dense_build_form, join_shape.cpp)
  const bool every_row_inserted = c.dense && a.lpred < 0 && !c.lcols[(size_t)a.lex[a.on_l[0]].column].has_nulls;
  const DenseBuildForm f = dense_build_form(c.dense, t.bytemap, t.sorted_mode, c.key_asc, c.dense_n, c.B, ctx->join_unsorted_builds.count(c.dup_hint) != 0,
                                            every_row_inserted);
  c.dense_sorted = f.sorted;
  c.dense_rank = f.rank;
  c.want_regions = regions_wanted(c.dense, c.speculate, c.B, t.region_mode);   // LDS-staged region build: 0 never, 1 when it pays, 2 always (tests)
  // Deferred sizing (qhip.h: qhip_ctx_allow_deferred_sizes): this join as a whole is identified by both sides' expressions,
  // its type and the probe rows (the build rows too unless they are themselves a capacity)
  c.size_key = join_size_key(a.L->rows_dev ? 0 : c.B, c.P, a.join_type, a.lpred, a.rpred, a.lex, a.nlex, a.rex, a.nrex, a.on_l, a.on_r, a.n_on);
  const auto hint = ctx->join_size_hints.find(c.size_key);
  c.defer = ctx->allow_deferred_sizes > 0 && c.speculate && a.join_type == QHIP_JOIN_INNER && a.froot < 0 && c.B > 0 && c.P > 0 &&
            hint != ctx->join_size_hints.end() && t.defer;
  // room for what the join produced last time + 1/8 + 1024 (an FK -> PK join cannot exceed its probe rows)
  c.defer_cap = c.defer ? std::min<uint64_t>(c.P, hint->second + hint->second / 8 + 1024) : 0;
}

// the lowered key plans of both sides (typing + generated source + loaded kernels) are cached per context, keyed by the
// column signatures and the expression PODs: a repeated join costs no typing, code generation or module lookup
void lookup_or_lower_plan(Ctx* ctx, const JoinArgs& a, JoinCall& c) {
  const std::string pkey = join_plan_key(c.lcols, c.rcols, a.lex, a.nlex, a.rex, a.nrex, a.on_l, a.on_r, a.n_on, a.lpred, a.rpred, c.want_regions,
                                         a.L->rows_dev != nullptr, c.dense);
  std::shared_ptr<JoinPlan>& jp = c.jp;
  auto cached = ctx->plan_cache.find(pkey);
  if (cached != ctx->plan_cache.end()) jp = std::static_pointer_cast<JoinPlan>(cached->second);
  else {
    jp = std::make_shared<JoinPlan>();
    ExprSet les, res;
    les.build(a.lex, a.nlex, c.lcols);
    res.build(a.rex, a.nrex, c.rcols);
    plan_keys(les, c.lcols, a.on_l, a.n_on, jp->lkp, a.lpred, c.dense ? KEYS_KERNEL_DENSE_BUILD : c.want_regions ? KEYS_KERNEL_SCATTER : KEYS_KERNEL_EVAL,
              (c.dense || c.want_regions) && a.L->rows_dev);
    plan_keys(res, c.rcols, a.on_r, a.n_on, jp->rkp, a.rpred, c.dense ? KEYS_KERNEL_DENSE_PROBE : KEYS_KERNEL_PROBE);   // the probe side's keys are evaluated inside the probe kernel
    for (int k = 0; k < a.n_on; ++k)
      if (jp->lkp.keys[(size_t)k].type != jp->rkp.keys[(size_t)k].type)   // arrow's eq (hash_join.rs:203) needs identical types
        fail(QHIP_INVALID_ARGUMENT, "Invalid argument error: Invalid comparison operation: " + dtype_name(jp->lkp.keys[(size_t)k].type) +
                                        " == " + dtype_name(jp->rkp.keys[(size_t)k].type));
    if (jp->rkp.W != jp->lkp.W) fail(QHIP_HIP_ERROR, "join key layouts of the two sides differ (internal error)");
    if (ctx->plan_cache.size() > 4096) ctx->plan_cache.clear();
    ctx->plan_cache[pkey] = jp;
  }
  c.W = jp->lkp.W;
}

// ---- build. Two layouts of the distinct-key table (slot = [state | key words], state - 2 = the build row):
//  * region layout, LDS-staged (the default while unique build keys are assumed): the table is cut into regions of 2^sb
//    slots at load <= 1/2; qk_join_scatter (JIT: fused scan filter + key words) drops every build row as an entry into its
//    region, k_join_region_build assembles each region and its slice of the hash filter in LDS and stores them as whole
//    lines. No memset, no per-row HBM atomic. Duplicate keys / an overfull region are detected there -> legacy layout.
//  * legacy layout: ONE open-addressing table filled with agent-scope atomics (k_join_build_insert), per-slot counts and,
//    for duplicated keys, the CSR of the build rows of every key.
void choose_table_layout(const JoinArgs& a, const JoinTuning& t, JoinCall& c) {
  if (c.want_regions) c.geo = region_geometry(c.B, c.W, a.lpred >= 0, t.region_load, t.region_slot_bits);
  c.region_build = c.geo.n_regions > 0;
  c.layout = c.dense_rank ? JOIN_LAYOUT_DENSE_RANK : c.dense ? JOIN_LAYOUT_DENSE : c.region_build ? JOIN_LAYOUT_REGIONS : JOIN_LAYOUT_LEGACY;
}

// only qk_join_scatter reads a device-side row count: otherwise wait, shrink, start over. A join type with a build-side
// tail (Left / Full / LeftSemi / LeftAnti) needs the EXACT build row count as well: the visited bitmap is scanned over
// B rows, and the pad rows [count, capacity) of a deferred table are never inserted, hence never visited — they would
// surface as unmatched build rows.
Repeat settle_build_side(const JoinArgs& a, const JoinCall& c) {
  if (a.L->rows_dev && ((!c.region_build && !c.dense) || (a.join_type != QHIP_JOIN_INNER && a.join_type != QHIP_JOIN_RIGHT))) {
    settle_rows(a.L);
    return Repeat::SettleBuild;
  }
  return Repeat::No;
}

// one arena: [table | count | filter] (table_sizes, join_shape.cpp)
Repeat allocate_table(JoinCall& c, JoinRun& r) {
  c.sz = table_sizes(c.layout, c.B, c.W, c.dense_n, c.geo);
  try {
    r.arena.alloc(c.sz.arena_bytes());
  } catch (const Error& e) {
    if (e.code != QHIP_OUT_OF_MEMORY || !c.dense) throw;
    // the direct-address table does not fit: the hashed layouts need 16-24 bytes per build ROW, not 4 per key VALUE
    return Repeat::DenseDoesNotFit;
  }
  r.table = r.arena.as<uint64_t>();
  r.count = (uint32_t*)(r.arena.as<uint8_t>() + c.sz.count_offset());
  r.bloom = (uint64_t*)(r.arena.as<uint8_t>() + c.sz.bloom_offset());
  return Repeat::No;
}

void build_dense_sorted(Ctx* ctx, const JoinArgs& a, const JoinCall& c, JoinRun& r) {
  JoinPlan* jp = c.jp.get();
  if (!jp->lmod_sorted) jp->lmod_sorted = get_module(ctx, jp->lkp.source, "qk_join_dense_build_sorted");
  HKArgs ka;
  fill_kargs(ctx, a.L, jp->lkp.bind, ka, jp->lstr);
  HDenseSortedLaunch sl;
  sl.bits = (uint32_t*)r.bloom; sl.status = c.dstat;
  if (c.dense_rank) sl.rank = (uint32_t*)r.table; else sl.row_of = (uint32_t*)r.table;
  sl.kmin = (uint64_t)c.kmin; sl.n = (uint32_t)c.dense_n; sl.words = c.sz.dense_words;
  void* args[] = {&ka, &sl};
  // a workgroup per kSortedBuildRows build rows of the capacity (a deferred-size build side: the kernel reads the count)
  const unsigned grid = (unsigned)std::max<uint64_t>(1, (c.B + kSortedBuildRows - 1) / kSortedBuildRows);
  trace_point("join: first launch");
  QHIP_HIP_CHECK(hipModuleLaunchKernel(jp->lmod_sorted->fn, grid, 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr));
  ++ctx->sorted_builds;
  trace_point("join: first launch done");
}

void build_dense(Ctx* ctx, const JoinArgs& a, const JoinTuning& t, const JoinCall& c, JoinRun& r) {
  JoinPlan* jp = c.jp.get();
  hipStream_t s = ctx->stream;
  const uint64_t dense_n = c.dense_n;
  if (!jp->lmod) jp->lmod = get_module(ctx, jp->lkp.source, jp->lkp.kernel_name);
  HKArgs ka;
  fill_kargs(ctx, a.L, jp->lkp.bind, ka, jp->lstr);
  // Byte-map form (round 4, QHIP_JOIN_DENSE_BYTEMAP=1; OFF by default): the build stamps one byte per key with a plain store,
  // a second kernel packs the bytes into the bitmap the probe reads and detects duplicate keys by counting — built to get
  // rid of the bitmap's scattered atomics (~32 G/s at the memory side) and measured SIX TIMES SLOWER on Q3 at SF10 (A/B on one
  // box, profiles/r04_dense_build_bytemap.txt): join 2's build 61 -> 352 us, join 1's 39 -> 86 us. A scattered ONE-BYTE store is
  // the worst thing one can ask of this memory system: every one becomes a read-modify-write of its ECC word at the memory
  // side (~5 G per second), where a scattered 4-byte atomic OR is served at ~32 G/s. Kept as a tested switch, not as a path.
  bool bytemap = t.bytemap && dense_n <= (1ull << t.bytemap_max_bits);
  HDenseBuildLaunch dl;
  dl.bits = (uint32_t*)r.bloom; dl.row_of = (uint32_t*)r.table; dl.status = c.dstat;
  dl.kmin = (uint64_t)c.kmin; dl.n = (uint32_t)dense_n;
  if (bytemap) {
    const size_t map_bytes = (size_t)c.sz.dense_words * 32;   // (whole bitmap words: the packing kernel reads 32 bytes per word)
    if (!jp->bytemap || jp->bytemap_n != dense_n || jp->bytemap_gen >= 255) {
      if (!jp->bytemap || jp->bytemap_n != dense_n) {
        jp->bytemap.reset();
        jp->bytemap_n = 0;
        try {
          jp->bytemap = std::make_shared<DevBuf>(map_bytes);
        } catch (const Error& e) {
          if (e.code != QHIP_OUT_OF_MEMORY) throw;
          bytemap = false;   // (the map stays with the plan between executions: when HBM is short, the atomic form needs no such buffer)
        }
      }
      if (bytemap) {
        QHIP_HIP_CHECK(hipMemsetAsync(jp->bytemap->ptr, 0, map_bytes, s));
        jp->bytemap_n = dense_n;
        jp->bytemap_gen = 0;
      }
    }
  }
  if (bytemap) {
    dl.gen = ++jp->bytemap_gen;
    dl.bytes = jp->bytemap->as<uint8_t>();
    dl.counters = zeroed_block(ctx);
  } else {
    QHIP_HIP_CHECK(hipMemsetAsync(r.bloom, 0, c.sz.bloom_bytes, s));
  }
  void* args[] = {&ka, &dl};
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((c.B + 1023) / 1024, (uint64_t)ctx->num_cus * 8));
  trace_point("join: first launch");
  QHIP_HIP_CHECK(hipModuleLaunchKernel(jp->lmod->fn, grid, 1, 1, 256, 1, 1, 0, s, args, nullptr));
  if (bytemap) launch_bytes_to_bits(dl.bytes, dl.gen, dl.bits, c.sz.dense_words, dl.counters, c.dstat, s);
  trace_point("join: first launch done");
}

void build_regions(Ctx* ctx, const JoinArgs& a, const JoinTuning& t, const JoinCall& c, JoinRun& r) {
  JoinPlan* jp = c.jp.get();
  hipStream_t s = ctx->stream;
  if (!jp->lmod) jp->lmod = get_module(ctx, jp->lkp.source, jp->lkp.kernel_name);
  HKArgs ka;
  fill_kargs(ctx, a.L, jp->lkp.bind, ka, jp->lstr);
  const ScatterShape sc = scatter_shape(c.B, (uint64_t)std::max(1, t.scatter_wgs.or_default(ctx->num_cus * 2)));
  const uint32_t n_regions = c.geo.n_regions;
  DevBuf entries(c.B * (1 + (size_t)c.W) * 8), first(sc.wgs * ((size_t)n_regions + 1) * 4);
  HScatterLaunch sl;
  sl.entries = entries.as<uint64_t>(); sl.first = first.as<uint32_t>(); sl.status = c.dstat;
  sl.n_regions = n_regions; sl.rows_per_wg = (uint32_t)sc.rows_per_wg;
  void* args[] = {&ka, &sl};
  trace_point("join: first launch");
  QHIP_HIP_CHECK(hipModuleLaunchKernel(jp->lmod->fn, (unsigned)sc.wgs, 1, 1, 1024, 1, 1, (n_regions + 1) * 4, s, args, nullptr));
  trace_point("join: first launch done");
  launch_join_region_build(c.W, entries.as<uint64_t>(), first.as<uint32_t>(), (uint32_t)sc.wgs, (uint32_t)sc.rows_per_wg, r.table, r.bloom, n_regions,
                           c.geo.slot_bits, c.geo.bword_bits, c.dstat, s);
  // (entries / first go back to the pool here; whoever gets them next runs on the same stream, i.e. afterwards)
}

void build_legacy_insert(Ctx* ctx, const JoinArgs& a, const JoinCall& c, JoinRun& r) {
  hipStream_t s = ctx->stream;
  QHIP_HIP_CHECK(hipMemsetAsync(r.arena.ptr, 0, r.arena.bytes, s));
  r.row_slot.alloc((c.B + 1) * 4);
  ExprSet les;
  les.build(a.lex, a.nlex, c.lcols);
  KeysPlan lkp_eval;   // (eval_key_words plans by itself: the same layout as the cached plan's lkp)
  eval_key_words(ctx, a.L, les, c.lcols, a.on_l, a.n_on, lkp_eval, r.lkeys, r.lvalid, a.lpred, true, c.dstat);
  launch_join_build_insert(c.W, r.lkeys.as<uint64_t>(), r.lvalid.as<uint64_t>(), c.B, r.table, c.sz.nslots, r.row_slot.as<uint32_t>(), r.count, r.bloom,
                           c.sz.filter_words - 1, c.dstat, s);
}

// the build status words have arrived in the pinned mirror
void check_build_status(const JoinCall& c, JoinRun& r) {
  check_status_words(c.st_build);
  if (c.st_build[QS_OVERFLOW]) fail(QHIP_HIP_ERROR, "join build table overflow (internal error)");
  r.max_count = c.st_build[QS_MAXCOUNT] & ~(uint32_t)QS_ORDER_BROKEN;
}

// one host wait for the build status alone (without speculation; under speculation with no probe rows to read it with)
void read_build_status(Ctx* ctx, const JoinCall& c, JoinRun& r) {
  QHIP_HIP_CHECK(hipMemcpyAsync(c.st_build, c.dstat, QS_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));   // key evaluation + build
  QHIP_HIP_CHECK(sync_stream(ctx->stream));
  verify_pending_sizes(ctx);
  check_build_status(c, r);
}

// Unique build keys (every FK -> PK join): each slot's state word names its one build row and nothing else is needed.
// Otherwise group the build rows by slot with a stable radix sort (ascending build row inside a key: the order the
// reference's reverse-built chains yield) into a CSR.
void build_csr(Ctx* ctx, const JoinCall& c, JoinRun& r) {
  hipStream_t s = ctx->stream;
  const uint64_t B = c.B;
  const uint32_t nslots = c.sz.nslots;
  launch_join_full_counts(c.W, r.table, nslots, r.count, s);
  DevBuf sorted_slot((B + 1) * 4), iota((B + 1) * 4);
  r.sorted_rows.alloc((B + 1) * 4);
  r.start.alloc(((size_t)nslots + 1) * 4);
  launch_iota_u32(iota.as<uint32_t>(), B, s);
  stable_sort_pairs_u32(r.row_slot.as<uint32_t>(), sorted_slot.as<uint32_t>(), iota.as<uint32_t>(), r.sorted_rows.as<uint32_t>(), B, log2u(nslots) + 1, s);
  exclusive_scan_u32(r.count, r.start.as<uint32_t>(), nslots, nullptr, s);
  // (the sort temporaries go back to the pool here; whoever gets them next runs on the same stream, i.e. afterwards)
  r.start_ptr = r.start.as<uint32_t>();
  r.rows_ptr = r.sorted_rows.as<uint32_t>();
}

// The join key of every output row, written by pass 2 for nothing (dense layout: a matching entry holds key - min): an Inner
// join on ONE Int64 column with unique build keys hands its key columns on as PLAIN columns instead of deferred gathers, so
// that a GROUP BY over them (Q3 groups by l_orderkey) streams 8 bytes per row instead of gathering through the index vector —
// one of the aggregate's five random reads per row gone (QHIP_JOIN_KEY_MATERIALIZE=0: gathers like every other column)
bool materializes_key(const JoinArgs& a, const JoinTuning& t, const JoinCall& c, const JoinRun& r) {
  return c.dense && r.unique_keys && a.join_type == QHIP_JOIN_INNER && a.froot < 0 && a.n_on == 1 && a.rex[a.on_r[0]].kind == QHIP_EXPR_COLUMN &&
         a.rex[a.on_r[0]].column >= 0 && a.rex[a.on_r[0]].column < (int)a.R->cols.size() &&
         a.R->cols[(size_t)a.rex[a.on_r[0]].column].type.id == QHIP_INT64 && t.key_materialize;
}

// The build-side index vector may stay owed: the dense layout with unique build keys, an Inner join without residual filter —
// pass 2's pairs-only branch, whose entries ARE the key indices — and a build side without a pending gather among its columns
// (a parent's composition would read the vector at once: Q3's join 2 translates in pass 2 as before; its join 1, whose customer
// columns nobody reads, never translates).
bool wants_lazy_build(const JoinArgs& a, const JoinTuning& t, const JoinCall& c, const JoinRun& r) {
  if (!t.lazy_index || t.eager_gather || !c.dense || !r.unique_keys || a.join_type != QHIP_JOIN_INNER || a.froot >= 0 || c.pad_right || c.has_tail ||
      c.mark_in_probe || r.start_ptr)
    return false;
  for (const DevColumn& col : a.L->cols)
    if (col.deferred && !col.deferred->done) return false;
  return true;
}

// ---- probe. Pass 1 (JIT: fused scan filter + key words + lookup straight from the probe table's columns) leaves one
// (slot, probe row) entry per MATCHING probe row and one pair count per 256-row tile; the tile counts are scanned; pass 2 writes the pairs in
// probe-row order. LeftSemi / LeftAnti without a residual filter only need the visited bits: pass 1 sets them.
void launch_probe(Ctx* ctx, const JoinArgs& a, const JoinTuning& t, const JoinCall& c, JoinRun& r) {
  JoinPlan* jp = c.jp.get();
  hipStream_t s = ctx->stream;
  const KeysPlan& rkp = jp->rkp;
  // (which kernel, its LDS and the grid: choose_probe_kernel / probe_grid, join_shape.cpp)
  const ProbeKernel pk = choose_probe_kernel(c.layout, c.P, rkp.probe_r, c.sz.dense_words, t.dense_lds, t.dense_wide, t.stage_extra);
  r.probe_name = pk.name;
  std::shared_ptr<Module>& rmod = jp->rmods[pk.name];
  if (!rmod) rmod = get_module(ctx, rkp.source, pk.name);
  const std::shared_ptr<Module>& mod = rmod;
  HKArgs ka;
  fill_kargs(ctx, a.R, rkp.bind, ka, jp->rstr);
  // (asked once per module AND dynamic-LDS size: the LDS / hybrid variants' bitmap part changes with the data under one cached
  // plan, and with it the workgroups a CU holds — ADVICE r03)
  if (mod->wgs_per_cu == 0 || mod->wgs_dyn_lds != pk.dyn_lds) {
    int nb = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, mod->fn, (int)pk.waves_per_wg * 64, pk.dyn_lds) != hipSuccess || nb < 1) nb = 1;
    mod->wgs_per_cu = nb;
    mod->wgs_dyn_lds = pk.dyn_lds;
  }
  const ProbeGrid pg = probe_grid(c.P, pk, ctx->num_cus, mod->wgs_per_cu, t.probe_tiles_per_wave);
  r.nchunks = pg.nchunks;
  r.tiles_per_wave = pg.tiles_per_wave;
  r.chunk_rows = pg.tiles_per_wave * pk.tile_rows;
  r.tile_tot.alloc((r.nchunks + 1) * 4);
  r.tile_nent.alloc((r.nchunks + 1) * 4);
  HProbeLaunch pl;
  pl.table = r.table; pl.bloom = r.bloom; pl.count = r.count; pl.start = r.start_ptr; pl.rows = r.rows_ptr;
  pl.ent_slot = r.ent_slot.as<uint32_t>();
  pl.ent_row = r.ent_row.as<uint32_t>();
  pl.tile_nent = r.tile_nent.as<uint32_t>();
  pl.tile_total = r.tile_tot.as<uint32_t>();
  pl.visited = (c.mark_in_probe && !c.want_pairs) ? r.visited.as<uint32_t>() : nullptr;
  pl.status = c.dstat + QS_WORDS;
  pl.nslots = c.sz.nslots; pl.bloom_mask = c.sz.filter_words - 1;
  pl.n_regions = c.geo.n_regions; pl.slot_bits = c.geo.slot_bits; pl.bword_bits = c.geo.bword_bits;
  pl.tiles_per_wave = (uint32_t)pg.tiles_per_wave;
  if (c.dense) {
    pl.count = nullptr;
    pl.stage_cap = pk.stage_cap;
    pl.dense_min = (uint64_t)c.kmin; pl.dense_n = (uint32_t)c.dense_n; pl.dense_words = c.sz.dense_words; pl.lds_words = pk.lds_words;
    pl.dense_rank = c.dense_rank ? (const uint32_t*)r.table : nullptr; pl.dense_last = (uint32_t)(c.B - 1);
  }
  void* args[] = {&ka, &pl};
  time_mark(ctx, 2);
  QHIP_HIP_CHECK(hipModuleLaunchKernel(mod->fn, pg.grid, 1, 1, pk.waves_per_wg * 64, 1, 1, (unsigned)pk.dyn_lds, s, args, nullptr));
  time_mark(ctx, 3);
  r.probe_timed = true;
  // (a join of deferred size needs neither the offsets nor the total before pass 2, and pass 2 can sum a few thousand counters
  // in every workgroup: the scan's launch — one workgroup, ~5 us of stream time — is dropped there)
  r.fold_scan = c.defer && c.want_pairs && t.fold_scan && r.nchunks <= t.fold_max_chunks && join_emit_can_fold(r.nchunks, r.tile_tot.as<uint32_t>());
  if (c.want_pairs && !r.fold_scan) exclusive_scan_u32(r.tile_tot.as<uint32_t>(), r.tile_tot.as<uint32_t>(), r.nchunks, c.dstat + 2 * QS_WORDS, s);
  if (c.want_pairs) ++(r.fold_scan ? ctx->join_scans_folded : ctx->join_scans_launched);
}

// pass 2: the pairs of every chunk's entries into b_idx / p_idx (room for r.M pairs). publish != null, the deferred form: it also
// pads the index vectors up to the capacity, publishes the status block to `publish` and the total to rows_blk
void emit_pairs(Ctx* ctx, const JoinCall& c, JoinRun& r, uint32_t* publish) {
  const bool deferred = publish != nullptr;
  r.b_idx.alloc((r.M + 1) * 4);
  r.p_idx.alloc((r.M + 1) * 4);
  if (c.pad_right && !deferred) {
    r.cnt.alloc((c.P + 1) * 4);
    r.pair_off.alloc((c.P + 1) * 4);
    QHIP_HIP_CHECK(hipMemsetAsync(r.cnt.ptr, 0, r.cnt.bytes, ctx->stream));   // pass 2 only visits matching probe rows
  }
  if (deferred) r.rows_blk = std::make_shared<DevBuf>(64);   // the output table's device-side row count
  if (r.mat_key && !r.lazy_build) r.key_vals = std::make_shared<DevBuf>((r.M + 1) * 8);
  // (owed build rows: without row_of / rank pass 2 stores the entries — the key indices — as they are)
  const uint32_t* const dense_table = r.lazy_build ? nullptr : (const uint32_t*)r.table;
  launch_join_emit(r.ent_slot.as<uint32_t>(), r.ent_row.as<uint32_t>(), r.tile_nent.as<uint32_t>(), r.tile_tot.as<uint32_t>(), r.count, r.start_ptr,
                   r.rows_ptr, c.dense && !c.dense_rank ? dense_table : nullptr, r.nchunks, r.chunk_rows, r.b_idx.as<uint32_t>(), r.p_idx.as<uint32_t>(),
                   c.pad_right && !deferred ? r.pair_off.as<uint32_t>() : nullptr, c.pad_right && !deferred ? r.cnt.as<uint32_t>() : nullptr,
                   c.mark_in_probe && !deferred ? r.visited.as<uint32_t>() : nullptr, deferred ? (uint32_t)r.M : 0xFFFFFFFFu, deferred ? c.dstat : nullptr,
                   publish, deferred ? r.rows_blk->as<uint32_t>() : nullptr, ctx->stream, r.key_vals ? r.key_vals->as<int64_t>() : nullptr, (uint64_t)c.kmin,
                   c.dense_rank ? dense_table : nullptr, (const uint32_t*)r.bloom, c.dense ? (uint32_t)(c.B - 1) : 0xFFFFFFFFu, deferred && r.fold_scan);
  if (r.lazy_build) ++ctx->lazy_index_joins;
}

// deferred size: no read-back — the status block + total go to a page-locked slot that the consumer's synchronisation checks
void emit_deferred(Ctx* ctx, const JoinCall& c, JoinRun& r) {
  if (!ctx->size_slots) QHIP_HIP_CHECK(hipHostMalloc((void**)&ctx->size_slots, (size_t)kSizeSlots * 32 * 4, hipHostMallocDefault));
  if (ctx->pending_sizes.size() >= (size_t)kSizeSlots) fail(QHIP_HIP_ERROR, "too many joins of deferred size in flight (internal error)");
  uint32_t* slot = ctx->size_slots + (size_t)(ctx->size_slot_next++ % kSizeSlots) * 32;
  auto total_out = std::make_shared<uint64_t>(~0ull);
  ctx->pending_sizes.push_back({slot, c.size_key, c.defer_cap, c.dup_hint, total_out});
  r.rows_final = total_out;
  r.M = c.defer_cap;
  emit_pairs(ctx, c, r, slot);
  r.deferred_slot = slot;
}

// ONE read-back: build status (needed only now under speculation), probe status and the pair total. Under speculation
// this is where a build side out of order or with duplicate keys shows: remembered on the context, and the attempt ends
Repeat read_probe_status(Ctx* ctx, const JoinArgs& a, const JoinCall& c, JoinRun& r) {
  QHIP_HIP_CHECK(hipMemcpyAsync(c.st_build, c.dstat, (2 * QS_WORDS + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  QHIP_HIP_CHECK(sync_stream(ctx->stream));
  verify_pending_sizes(ctx);   // (a build side of deferred size: did ITS join have room?)
  if (c.speculate) {
    // the sorted dense build found its keys out of order: remember the build side, run the join again with the atomic build
    if (c.dense_sorted && (c.st_build[QS_MAXCOUNT] & QS_ORDER_BROKEN)) {
      if (ctx->join_unsorted_builds.size() > 4096) ctx->join_unsorted_builds.clear();   // a hint, not a record
      ctx->join_unsorted_builds.insert(c.dup_hint);
      ++ctx->sorted_build_fallbacks;
      return Repeat::BuildOutOfOrder;
    }
    check_build_status(c, r);
    if (r.max_count > 1) {   // duplicate build keys after all: remember, and run again with the CSR layout
      if (ctx->join_dup_builds.size() > 4096) ctx->join_dup_builds.clear();   // a hint, not a record
      ctx->join_dup_builds.insert(c.dup_hint);
      return Repeat::DuplicateBuildKeys;
    }
  }
  check_status_words(c.st);
  r.M = c.st[QS_WORDS];
  if (a.join_type == QHIP_JOIN_INNER && a.froot < 0) {
    if (ctx->join_size_hints.size() > 4096) ctx->join_size_hints.clear();   // hints, not records
    ctx->join_size_hints[c.size_key] = r.M;
  }
  return Repeat::No;
}

// ---- residual JoinFilter (join/mod.rs:125-154): evaluate over an intermediate batch of the filter's columns, keep true rows
bool apply_residual_filter(Ctx* ctx, const JoinArgs& a, JoinRun& r) {
  if (a.froot < 0 || r.M == 0) return false;
  hipStream_t s = ctx->stream;
  const uint64_t M = r.M;
  qhip_table inter;
  inter.ctx = ctx;
  for (int k = 0; k < a.nfcols; ++k) {
    const qhip_table* src = a.fsides[k] == 0 ? a.L : a.R;
    if (a.fcols[k] < 0 || a.fcols[k] >= (int)src->cols.size()) fail(QHIP_INVALID_ARGUMENT, "join filter column index out of range");
    inter.cols.push_back(gather_column(ctx, src->cols[(size_t)a.fcols[k]], a.fsides[k] == 0 ? r.b_idx.as<uint32_t>() : r.p_idx.as<uint32_t>(), M, false));
    inter.names.push_back(src->names[(size_t)a.fcols[k]]);
    inter.nullable.push_back(true);
  }
  inter.num_rows = (int64_t)M;
  inter.batch_offsets = {0, (int64_t)M};
  std::vector<InputCol> fic = input_cols_of(&inter);
  ExprSet fes;
  fes.build(a.fex, a.nfex, fic);
  DevBuf mask, wave, sel;
  run_pred_mask(ctx, &inter, fes, fic, a.froot, mask, wave);
  const uint32_t m2 = select_from_mask(ctx, mask, wave, (int64_t)M, sel);
  DevBuf b2(((uint64_t)m2 + 1) * 4), p2(((uint64_t)m2 + 1) * 4);
  launch_gather_fixed(r.b_idx.ptr, sel.as<uint32_t>(), b2.ptr, m2, 4, s);
  launch_gather_fixed(r.p_idx.ptr, sel.as<uint32_t>(), p2.ptr, m2, 4, s);
  QHIP_HIP_CHECK(sync_stream(s));
  r.b_idx = std::move(b2);
  r.p_idx = std::move(p2);
  r.M = m2;
  return true;
}

// ---- visited bitmap (when the probe kernel has not marked it already); per-probe-row surviving counts for the
// Right / Full padding when the residual filter changed them
void mark_visited_and_count(Ctx* ctx, const JoinCall& c, bool filtered, JoinRun& r) {
  hipStream_t s = ctx->stream;
  DevBuf& cnt2 = r.cnt2;
  if (filtered && c.pad_right) {
    cnt2.alloc((c.P + 1) * 4);
    QHIP_HIP_CHECK(hipMemsetAsync(cnt2.ptr, 0, cnt2.bytes, s));
  }
  if ((c.has_tail && !r.visited_done) || cnt2.ptr)
    launch_join_mark(r.b_idx.as<uint32_t>(), r.p_idx.as<uint32_t>(), r.M, r.visited.as<uint32_t>(), cnt2.ptr ? cnt2.as<uint32_t>() : nullptr, s);
  r.final_cnt = cnt2.ptr ? cnt2.as<uint32_t>() : r.cnt.as<uint32_t>();
  r.final_off = r.pair_off.as<uint32_t>();   // exclusive scan of final_cnt (position of a probe row's first pair)
  if (cnt2.ptr) {
    r.off2.alloc((c.P + 1) * 4);
    exclusive_scan_u32(r.final_cnt, r.off2.as<uint32_t>(), c.P, nullptr, s);
    r.final_off = r.off2.as<uint32_t>();
  }
}

// ---- Right / Full: probe rows without a surviving pair appear once with a NULL build index, in probe order
void pad_right_rows(Ctx* ctx, const JoinCall& c, JoinRun& r) {
  hipStream_t s = ctx->stream;
  const uint64_t P = c.P;
  DevBuf out_cnt((P + 1) * 4), tot(4);
  r.out_off.alloc((P + 1) * 4);
  launch_join_out_counts(r.final_cnt, P, out_cnt.as<uint32_t>(), s);
  exclusive_scan_u32(out_cnt.as<uint32_t>(), r.out_off.as<uint32_t>(), P, tot.as<uint32_t>(), s);
  const uint64_t M2 = P ? read_u32(s, tot.ptr) : 0;
  DevBuf b3((M2 + 1) * 4), p3((M2 + 1) * 4);
  launch_join_adjust_right(r.b_idx.as<uint32_t>(), r.final_cnt, r.final_off, r.out_off.as<uint32_t>(), P, b3.as<uint32_t>(), p3.as<uint32_t>(), s);
  r.b_idx = std::move(b3);
  r.p_idx = std::move(p3);
  r.M = M2;
  r.final_off = r.out_off.as<uint32_t>();
}

// ---- tail: unmatched build rows (Left / Full / LeftAnti) or matched ones (LeftSemi), ascending build index
void select_tail(Ctx* ctx, const JoinArgs& a, const JoinCall& c, JoinRun& r) {
  const uint64_t B = c.B;
  if (c.has_tail && B > 0) {
    DevBuf tmask(((B + 63) / 64) * 8 + 8), twave((((B + 63) / 64) + 1) * 4);
    launch_mask_from_bits(r.visited.as<uint32_t>(), B, a.join_type == QHIP_JOIN_LEFT_SEMI ? 1 : 0, tmask.as<uint64_t>(), twave.as<uint32_t>(), ctx->stream);
    r.T = select_from_mask(ctx, tmask, twave, (int64_t)B, r.tail_sel);
  }
  r.total_rows = r.M + r.T;
  if (r.total_rows >= kNullIdx) fail(QHIP_UNSUPPORTED, "join output of 2^32 - 1 rows or more is not supported");
}

// ---- index vectors of the whole output: [pairs | tail]
void concat_index_vectors(Ctx* ctx, JoinRun& r) {
  hipStream_t s = ctx->stream;
  const uint64_t M = r.M, T = r.T;
  r.b_all = std::make_shared<DevBuf>();
  r.p_all = std::make_shared<DevBuf>();
  if (T == 0) {
    *r.b_all = std::move(r.b_idx);   // no tail rows: the pair vectors are the output index vectors
    *r.p_all = std::move(r.p_idx);
  } else {
    r.b_all->alloc((r.total_rows + 1) * 4);
    r.p_all->alloc((r.total_rows + 1) * 4);
    if (M) {
      QHIP_HIP_CHECK(hipMemcpyAsync(r.b_all->ptr, r.b_idx.ptr, M * 4, hipMemcpyDeviceToDevice, s));
      QHIP_HIP_CHECK(hipMemcpyAsync(r.p_all->ptr, r.p_idx.ptr, M * 4, hipMemcpyDeviceToDevice, s));
    }
    QHIP_HIP_CHECK(hipMemcpyAsync(r.b_all->as<uint32_t>() + M, r.tail_sel.ptr, T * 4, hipMemcpyDeviceToDevice, s));
    launch_fill_u32(r.p_all->as<uint32_t>() + M, T, kNullIdx, s);
  }
}

// ---- output columns (build_batch_from_indices, utils/batch.rs:18-61): the reference gathers every column of both
// sides; here the gathers are deferred until a column is read (a parent join / aggregate touches only a few)
void make_output_columns(Ctx* ctx, const JoinArgs& a, const JoinTuning& t, const JoinCall& c, JoinRun& r, qhip_table* out) {
  const qhip_table *L = a.L, *R = a.R;
  const uint64_t total_rows = r.total_rows;
  out->ctx = ctx;
  const bool left_nullable = c.pad_right;
  const bool right_nullable = c.has_tail;
  // (an Inner join with unique build keys emits its pairs in probe-row order, one per probe row at most: the probe side's
  // index vector ascends strictly, and a key column read through it keeps its order — key_ascending)
  const bool probe_idx_ascends = a.join_type == QHIP_JOIN_INNER && r.unique_keys && r.T == 0;
  auto add_side = [&](const qhip_table* src, const std::shared_ptr<DevBuf>& idx, bool side_nullable, bool idx_ascends) {
    if (t.eager_gather) for (auto& col : src->cols) out->cols.push_back(gather_column(ctx, col, idx->as<uint32_t>(), total_rows, side_nullable));
    else defer_gather(ctx, src->cols, idx, total_rows, side_nullable, out->cols, idx_ascends);
    for (size_t k = 0; k < src->cols.size(); ++k) {
      out->names.push_back(src->names[k]);
      out->nullable.push_back(src->nullable[k] || side_nullable);
    }
  };
  // owed build rows: b_all holds key indices. The object every build-side column shares keeps the dense table (row_of, or rank +
  // bitmap: the arena, which would otherwise go back to the pool with this call) until the first reader looks the rows up
  std::shared_ptr<LazyIndex> key_idx;
  if (r.lazy_build) {   // (an Inner join: no tail rows, b_all is pass 2's vector)
    key_idx = LazyIndex::of(r.b_all, total_rows);
    auto owed = std::make_shared<LazyIndex>();
    owed->m = total_rows;
    owed->keys = key_idx;
    owed->table = std::make_shared<DevBuf>(std::move(r.arena));
    (c.dense_rank ? owed->rank : owed->row_of) = (const uint32_t*)r.table;
    owed->rank_bits = c.dense_rank ? (const uint32_t*)r.bloom : nullptr;
    owed->build_last = (uint32_t)(c.B - 1);
    defer_gather(ctx, L->cols, owed, total_rows, left_nullable, out->cols, false);
    for (size_t k = 0; k < L->cols.size(); ++k) {
      out->names.push_back(L->names[k]);
      out->nullable.push_back(L->nullable[k] || left_nullable);
    }
  } else {
    add_side(L, r.b_all, left_nullable, false);
  }
  if (!c.semi_anti) add_side(R, r.p_all, right_nullable, probe_idx_ascends);
  if (key_idx && r.mat_key) {
    // ... and the key columns are owed with them: key_min + key index, written as plain columns when somebody reads them
    auto owed_key = [&](const DevColumn& src) {
      DevColumn col;
      col.type = src.type;
      col.length = (int64_t)total_rows;
      col.value_maxabs = src.value_maxabs;
      col.range = src.range;             // (a subset of the source's values: its bounds hold)
      col.range_inherited = true;
      auto d = std::make_shared<DeferredGather>();
      d->src.type = src.type; d->src.value_maxabs = src.value_maxabs; d->src.range = src.range; d->src.range_inherited = true;
      d->key_of = key_idx; d->key_min = c.kmin; d->m = total_rows;
      col.deferred = d;
      return col;
    };
    const qhip_expr& lk = a.lex[a.on_l[0]];
    const size_t rc = (size_t)a.rex[a.on_r[0]].column;
    out->cols[L->cols.size() + rc] = owed_key(R->cols[rc]);
    if (lk.kind == QHIP_EXPR_COLUMN && lk.column >= 0 && lk.column < (int)L->cols.size() && L->cols[(size_t)lk.column].type.id == QHIP_INT64)
      out->cols[(size_t)lk.column] = owed_key(L->cols[(size_t)lk.column]);
  }
  if (r.key_vals) {
    auto plain = [&](const DevColumn& src) {
      DevColumn col;
      col.type = src.type;
      col.length = (int64_t)total_rows;
      col.values = r.key_vals;
      col.value_maxabs = src.value_maxabs;
      col.range = src.range;             // (a subset of the source's values: its bounds hold)
      col.range_inherited = true;
      return col;
    };
    const qhip_expr& lk = a.lex[a.on_l[0]];
    const size_t rc = (size_t)a.rex[a.on_r[0]].column;
    out->cols[L->cols.size() + rc] = plain(R->cols[rc]);
    // ... and the build side's key column holds the same values row for row
    if (lk.kind == QHIP_EXPR_COLUMN && lk.column >= 0 && lk.column < (int)L->cols.size() && L->cols[(size_t)lk.column].type.id == QHIP_INT64)
      out->cols[(size_t)lk.column] = plain(L->cols[(size_t)lk.column]);
  }
  out->num_rows = (int64_t)total_rows;
  if (r.deferred_slot) {   // total_rows is the capacity; the count is what pass 2 left in rows_blk
    out->rows_blk = r.rows_blk;
    out->rows_dev = r.rows_blk->as<uint32_t>();
    out->rows_host = r.deferred_slot + 2 * QS_WORDS;
    out->rows_final = r.rows_final;
  }
}

// ---- output batches: one per non-empty probe batch (hash_join.rs:363-372), then the tail batch
void set_batch_offsets(Ctx* ctx, const JoinArgs& a, const JoinTuning& t, const JoinCall& c, const JoinRun& r, qhip_table* out) {
  const qhip_table* R = a.R;
  out->batch_offsets.clear();
  out->batch_offsets.push_back(0);
  if (!c.semi_anti && R->num_batches() > 0 && r.M > 0) {
    const size_t nb1 = R->offsets().size();
    // first output row of every probe batch, computed on the device and LEFT there (qhip_table::offsets() fetches it when
    // somebody asks: a download, a Filter / Limit / probe side above; a parent's build side or an aggregate never does)
    auto pend = std::make_shared<PendingOffsets>();
    pend->n = nb1;
    pend->skip_empty = true;
    pend->tail = c.has_tail;
    pend->total_rows = (int64_t)r.total_rows;
    if (c.pad_right) {
      pend->pos = std::make_shared<DevBuf>(nb1 * 4);
      launch_lookup_u32(r.final_off, R->device_offsets(), (uint32_t)nb1, c.P, (uint32_t)r.M, pend->pos->as<uint32_t>(), ctx->stream);
    } else {   // the pairs' probe rows ascend: a binary search per batch boundary, run when somebody asks (PendingOffsets)
      pend->search_in = r.p_all;
      pend->search_m = r.M;
      // (the probe side's batch boundaries go along on the host, or as the device copy another operator already made:
      // uploading them here would be a host wait per join for something a parent join or an aggregate never asks for)
      if (R->offsets_dev) pend->bounds = R->offsets_dev;
      else pend->bounds_host.assign(R->offsets().begin(), R->offsets().end());
    }
    out->batch_offsets.clear();
    out->pending_offsets = pend;
    if (t.eager_offsets && !r.deferred_slot) (void)out->offsets();
  } else if (c.has_tail) {
    out->batch_offsets.push_back((int64_t)r.total_rows);   // always present, possibly empty (hash_join.rs:374-381)
  }
}

void set_join_stats(Ctx* ctx, const JoinArgs& a, const JoinCall& c, const JoinRun& r) {
  time_mark(ctx, 1);
  ctx->stats_timing_pending = ctx->timing ? 2 : 0;   // total = ev0..ev1, probe = ev2..ev3, read by qhip_ctx_last_stats
  ctx->stats.rows_in = (int64_t)c.P;
  ctx->stats.rows_out = (int64_t)r.total_rows;
  ctx->stats.groups = (int64_t)r.M;
  ctx->stats.table_capacity = c.dense ? (int64_t)c.dense_n : c.sz.nslots;
  snprintf(ctx->stats.main_kernel_name, sizeof ctx->stats.main_kernel_name, "%s", r.probe_name.c_str());
  // bytes of column data the probe kernel / the build's key evaluation read per row (roofline figures)
  auto bytes_per_row = [&](const qhip_table* t, const KernelBindings& b) {
    double sum = 0;
    for (size_t k = 0; k < b.cols.size(); ++k) {
      const DevColumn& dc = t->cols[(size_t)b.cols[k]];
      const int w = dtype_width(dc.type);
      if (w > 0) sum += k < b.narrow.size() && b.narrow[k] ? (int)b.narrow[k] : w;   // (a key column read as its 4-byte narrow copy)
      else if (dc.type.id == QHIP_BOOL) sum += 0.125;
      else if (dc.type.id == QHIP_UTF8) sum += 4.0 + (t->num_rows > 0 ? (double)dc.data_bytes / (double)t->num_rows : 0.0);
      if (dc.null_count > 0) sum += 0.125;
    }
    return sum;
  };
  ctx->stats.bytes_per_row_read = bytes_per_row(a.R, c.jp->rkp.bind);
  ctx->stats.build_bytes_per_row = bytes_per_row(a.L, c.jp->lkp.bind);
  ctx->stats.build_rows = (int64_t)c.B;
}

// ---------------------------------------------------------------- the driver
// (first: the switches as the caller has just read them, for the first attempt — one look at the environment per call)
qhip_table* hash_join(Ctx* ctx, const JoinArgs& a, const JoinTuning* first = nullptr) {
  bool dense_off = false;   // the dense layout is switched off for the attempts that follow one whose dense table did not fit
  // An attempt that cannot go on says why and the next one starts from the top. The loop ends because each reason removes its own
  // cause: settling drops L->rows_dev; "dense does not fit" sets dense_off; a build side found out of order or with duplicate keys
  // is in the context's hint sets (join_unsorted_builds / join_dup_builds), which switch the sorted build / the speculation off
  // for its dup_hint. A failed attempt's device buffers go back to the pool at the end of the loop body: whoever gets them next
  // runs on the same stream, i.e. afterwards.
  for (Repeat why = Repeat::No;; ) {
    if (why == Repeat::DenseDoesNotFit) dense_off = true;
    trace_point("join: entry");
    QHIP_HIP_CHECK(hipSetDevice(ctx->device));
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    ctx->stats_timing_pending = 0;
    validate_join_args(a);
    // a probe side of deferred size is made exact first; a build side of deferred size is read as it is when the region
    // build takes it (qk_join_scatter stops at the device-side row count), else it is made exact too (settle_build_side)
    settle_rows(a.R);
    const JoinTuning t = first && why == Repeat::No ? *first : read_join_tuning();
    JoinCall c;
    JoinRun r;
    set_join_type_flags(a, c);
    choose_dense_candidate(ctx, a, t, dense_off, c);
    resolve_join_inputs(ctx, a, t, c);
    time_mark(ctx, 0);
    check_scan_filters(a);
    decide_speculation(ctx, a, t, c);
    c.dstat = zeroed_block(ctx);   // (handed out clean from the context's ring — no memset launch per join)
    c.st_build = (uint32_t*)ctx->pinned;
    c.st = c.st_build + QS_WORDS;
    lookup_or_lower_plan(ctx, a, c);
    choose_table_layout(a, t, c);
    if ((why = settle_build_side(a, c)) != Repeat::No) continue;
    if ((why = allocate_table(c, r)) != Repeat::No) continue;

    if (c.dense_sorted) build_dense_sorted(ctx, a, c, r);
    else if (c.dense) build_dense(ctx, a, t, c, r);
    else if (c.region_build) build_regions(ctx, a, t, c, r);
    else build_legacy_insert(ctx, a, c, r);
    if (!c.speculate) read_build_status(ctx, c, r);
    r.unique_keys = c.speculate || (r.max_count <= 1 && !t.force_csr);
    if (!r.unique_keys) build_csr(ctx, c, r);

    r.visited.alloc((((c.B + 63) / 64) * 2 + 2) * 4);
    if (c.has_tail) QHIP_HIP_CHECK(hipMemsetAsync(r.visited.ptr, 0, r.visited.bytes, ctx->stream));
    r.ent_slot.alloc((c.P + 1) * 4);
    r.ent_row.alloc((c.P + 1) * 4);
    r.probe_name = c.dense ? "qk_join_probe_dense" : "qk_join_probe";
    r.mat_key = materializes_key(a, t, c, r);
    r.lazy_build = c.P > 0 && wants_lazy_build(a, t, c, r);   // (without probe rows there is no pass 2 and nothing to owe)
    if (c.P > 0) {
      launch_probe(ctx, a, t, c, r);
      if (c.defer) emit_deferred(ctx, c, r);
      else {
        if ((why = read_probe_status(ctx, a, c, r)) != Repeat::No) continue;
        if (c.want_pairs) emit_pairs(ctx, c, r, nullptr);
      }
      r.tile_tot.release();   // (back to the pool: pass 2 is queued on the same stream)
      r.tile_nent.release();
      r.visited_done = c.mark_in_probe;
    } else if (c.speculate) {
      read_build_status(ctx, c, r);   // (duplicates do not matter without probe rows)
    }
    if (!r.probe_timed) { time_mark(ctx, 2); time_mark(ctx, 3); }

    const bool filtered = apply_residual_filter(ctx, a, r);
    mark_visited_and_count(ctx, c, filtered, r);
    if (c.pad_right) pad_right_rows(ctx, c, r);
    if (c.semi_anti) r.M = 0;   // hash_join.rs:260-262: nothing is emitted while probing
    select_tail(ctx, a, c, r);
    concat_index_vectors(ctx, r);
    std::unique_ptr<qhip_table> out(new qhip_table());
    make_output_columns(ctx, a, t, c, r, out.get());
    set_batch_offsets(ctx, a, t, c, r, out.get());
    set_join_stats(ctx, a, c, r);
    return out.release();
  }
}


// ---------------------------------------------------------------- stage 0: wide join keys
// The reference hashes join keys of any length and any number of columns (utils/array.rs:171-210) and compares them on every
// probe hit (hash_join.rs:191-215); a packed join key has 8 words (a Utf8 key 7 of them). A key that does not fit never reaches
// the join: k_widekey_join_build gives every build row the number of ONE build row with the same key, k_widekey_join_lookup gives
// every probe row the number of the build row that represents its key, or -1 (device/qhip_widekey.inc) — exact, the keys
// themselves are compared; a row with a NULL key column matches nothing — and hash_join runs, with all its layouts, join types,
// residual filter, deferred sizes and output order, over views of both sides whose one key is that Int32 column. The build
// codes lie in [0, B), which the view says (ColRange), so the direct-address layout is taken without a reduction. 16 bytes of
// HBM per BUILD row (the slot table, twice the rows) while the stage runs + 4 per row of either side for the codes. Rows a fused
// scan filter rejects are encoded for nothing; a rejected build row may be a key's representative: the code is only a label.
// mode 1: when the packed key does not fit; 2: every hash join whose keys on both sides are plain columns (tests, fuzzing).
// Runs ONCE per call, outside the driver's attempts. Returns the result, or nullptr when the join runs on its keys as they are.
bool plain_column_keys(const qhip_table* t, const qhip_expr* ex, int nex, const int32_t* on, int n_on) {
  for (int k = 0; k < n_on; ++k) {
    if (on[k] < 0 || on[k] >= nex) return false;
    const qhip_expr& e = ex[on[k]];
    if (e.kind != QHIP_EXPR_COLUMN || e.column < 0 || e.column >= (int)t->cols.size()) return false;
  }
  return true;
}
bool plain_join_keys(const JoinArgs& a) {
  return a.n_on > 0 && a.on_l && a.on_r && plain_column_keys(a.L, a.lex, a.nlex, a.on_l, a.n_on) && plain_column_keys(a.R, a.rex, a.nrex, a.on_r, a.n_on);
}

// one side of the coded join: the side's columns + its code column, the key expression array with ONE key root
struct CodedSide {
  qhip_table view;
  std::vector<qhip_expr> ex;
  int32_t root = 0;
};
void make_coded_side(Ctx* ctx, const qhip_table* t, const qhip_expr* ex, int nex, int pred, const std::shared_ptr<DevBuf>& code, CodedSide& out) {
  qhip_table& v = out.view;
  v.ctx = ctx;
  v.names = t->names;
  v.nullable = t->nullable;
  v.cols = t->cols;
  v.num_rows = t->num_rows;
  v.batch_offsets = t->batch_offsets;        // (the batch structure as it is, fetched or not)
  v.pending_offsets = t->pending_offsets;
  v.offsets_dev = t->offsets_dev;
  DevColumn cc;
  cc.type = DType(QHIP_INT32); cc.length = t->num_rows; cc.values = code;
  v.names.push_back("key_code");
  v.nullable.push_back(false);
  v.cols.push_back(std::move(cc));
  out.ex.assign(ex, ex + nex);
  qhip_expr ce;
  memset(&ce, 0, sizeof ce);
  ce.kind = QHIP_EXPR_COLUMN; ce.column = (int32_t)t->cols.size(); ce.left = ce.right = ce.third = -1;
  // The key columns' own nodes stay in the array. Whatever the scan filter does not reach must not count as a reference any
  // more — the join gathers or uploads the columns its expression arrays name — so those Column nodes now name the code column.
  std::vector<char> reached((size_t)nex, 0);
  std::vector<int32_t> todo;
  if (pred >= 0) todo.push_back(pred);
  while (!todo.empty()) {
    const int32_t k = todo.back();
    todo.pop_back();
    if (k < 0 || k >= nex || reached[(size_t)k]) continue;
    reached[(size_t)k] = 1;
    todo.push_back(out.ex[(size_t)k].left); todo.push_back(out.ex[(size_t)k].right); todo.push_back(out.ex[(size_t)k].third);
  }
  for (int k = 0; k < nex; ++k)
    if (!reached[(size_t)k] && out.ex[(size_t)k].kind == QHIP_EXPR_COLUMN) out.ex[(size_t)k].column = ce.column;
  out.ex.push_back(ce);
  out.root = nex;
}

qhip_table* maybe_encode_wide_join_key(Ctx* ctx, const JoinTuning& tune, int mode, const JoinArgs& a) {
  if (mode <= 0 || !plain_join_keys(a)) return nullptr;
  const int n = a.n_on;
  validate_join_args(a);
  QHIP_HIP_CHECK(hipSetDevice(ctx->device));
  settle_rows(a.R);   // (as the driver does first)
  std::vector<int32_t> lkeys((size_t)n), rkeys((size_t)n);
  for (int k = 0; k < n; ++k) { lkeys[(size_t)k] = a.lex[a.on_l[k]].column; rkeys[(size_t)k] = a.rex[a.on_r[k]].column; }
  if (mode == 1) {   // (what resolve_join_inputs is about to do anyway: nothing is gathered or measured twice)
    resolve_referenced(ctx, a.L, a.lex, a.nlex, true);
    resolve_referenced(ctx, a.R, a.rex, a.nrex);
    std::vector<InputCol> lc = input_cols_of(a.L, true), rc = input_cols_of(a.R);
    ensure_utf8_key_lengths(ctx, a.L, a.lex, a.nlex, a.on_l, n, lc);
    ensure_utf8_key_lengths(ctx, a.R, a.rex, a.nrex, a.on_r, n, rc);
    for (int k = 0; k < n; ++k) {
      InputCol &l = lc[(size_t)lkeys[(size_t)k]], &r = rc[(size_t)rkeys[(size_t)k]];
      l.utf8_max_len = r.utf8_max_len = std::max(l.utf8_max_len, r.utf8_max_len);
      l.has_nulls = r.has_nulls = false;   // (a join key has no null-mask word: plan_keys lays it out without one)
    }
    if (packed_key_fits(lc, lkeys.data(), n) && packed_key_fits(rc, rkeys.data(), n)) return nullptr;
  }
  // the errors the join raises, with its texts, before any kernel of the stage: scan filters, expression typing, key types
  check_scan_filters(a);
  {
    ExprSet les, res;
    les.build(a.lex, a.nlex, input_cols_of(a.L));
    res.build(a.rex, a.nrex, input_cols_of(a.R));
    for (int k = 0; k < n; ++k) check_key_type(les.at(a.on_l[k]).type);
    for (int k = 0; k < n; ++k) check_key_type(res.at(a.on_r[k]).type);
    for (int k = 0; k < n; ++k)
      if (les.at(a.on_l[k]).type != res.at(a.on_r[k]).type)   // arrow's eq (hash_join.rs:203) needs identical types
        fail(QHIP_INVALID_ARGUMENT, "Invalid argument error: Invalid comparison operation: " + dtype_name(les.at(a.on_l[k]).type) + " == " +
                                        dtype_name(res.at(a.on_r[k]).type));
  }
  if (n > kWideKeyCols) fail(QHIP_UNSUPPORTED, "join key of more than 32 columns is not accelerated");
  // 1. exact row counts, the key columns materialised
  settle_rows(a.L);
  const int64_t B = a.L->num_rows, P = a.R->num_rows;
  if (B > ((int64_t)1 << 30)) fail(QHIP_UNSUPPORTED, "wide join key over more than 2^30 build rows is not accelerated");
  WideKeyCols bk, pk;
  memset(&bk, 0, sizeof bk);
  memset(&pk, 0, sizeof pk);
  auto describe = [&](const qhip_table* t, const std::vector<int32_t>& keys, WideKeyCols& wk) {
    for (int k = 0; k < n; ++k) {
      const DevColumn& c = resolved(ctx, t->cols[(size_t)keys[(size_t)k]]);
      WideKeyCol& d = wk.c[k];
      d.v = c.values ? c.values->ptr : nullptr;
      d.d = c.data ? c.data->as<uint8_t>() : nullptr;
      d.n = c.validity ? c.validity->as<uint8_t>() : nullptr;
      d.width = (uint32_t)dtype_width(c.type);   // (0: Utf8 — check_key_type has let nothing else without a width through)
    }
  };
  if (B > 0) describe(a.L, lkeys, bk);
  if (P > 0) describe(a.R, rkeys, pk);
  // 2. the codes
  auto bcode = std::make_shared<DevBuf>((size_t)B * 4), pcode = std::make_shared<DevBuf>((size_t)P * 4);
  const uint32_t nslots = std::max<uint32_t>(1024, pow2_ceil32((uint64_t)std::max<int64_t>(B, 1) * 2));
  struct Events {   // (timings asked for: a pair of the stage's own — the join behind it records the context's)
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipEvent_t operator[](int k) const { return e[k]; }
  } ev;
  if (ctx->timing) for (hipEvent_t& e : ev.e) { QHIP_HIP_CHECK(hipEventCreate(&e)); }
  if (B > 0 || P > 0) {
    DevBuf table((size_t)nslots * 8);
    const int bits = tune.wide_key_hash_bits;
    const uint64_t hash_mask = bits > 0 && bits < 64 ? (1ULL << bits) - 1 : ~0ULL;
    if (ev[0]) (void)hipEventRecord(ev[0], ctx->stream);
    QHIP_HIP_CHECK(hipMemsetAsync(table.ptr, 0, (size_t)nslots * 8, ctx->stream));
    launch_widekey_join_build(bk, n, table.as<uint64_t>(), nslots, hash_mask, bcode->as<int32_t>(), (uint64_t)B, ctx->stream);
    launch_widekey_join_lookup(pk, bk, n, table.as<uint64_t>(), nslots, hash_mask, pcode->as<int32_t>(), (uint64_t)P, ctx->stream);
    if (ev[1]) (void)hipEventRecord(ev[1], ctx->stream);
    // (the table goes back to the pool here; whoever gets it next runs on the same stream, i.e. afterwards)
  }
  // 3. both sides' columns + their code column; 4. the one key of either side is that column
  CodedSide ls, rs;
  make_coded_side(ctx, a.L, a.lex, a.nlex, a.lpred, bcode, ls);
  make_coded_side(ctx, a.R, a.rex, a.nrex, a.rpred, pcode, rs);
  {   // the build codes' range by construction: the direct-address layout without a reduction and a host wait
    ColRange& range = *ls.view.cols.back().range;
    range.known = true; range.min = 0; range.max = std::max<int64_t>(B - 1, 0); range.ascending = false;
  }
  JoinArgs c = a;
  c.L = &ls.view; c.R = &rs.view;
  c.lex = ls.ex.data(); c.nlex = (int)ls.ex.size();
  c.rex = rs.ex.data(); c.nrex = (int)rs.ex.size();
  c.on_l = &ls.root; c.on_r = &rs.root; c.n_on = 1;
  // 5. the join itself, unchanged (scan filters, residual filter and join type as they came). The dense Inner join's key
  // materialisation (materializes_key) asks for an Int64 key column: never taken for the Int32 codes.
  std::unique_ptr<qhip_table> out(hash_join(ctx, c, &tune));
  ++ctx->wide_key_joins;
  if (ev[0] && ev[1] && (B > 0 || P > 0)) {   // the stage's memset + two kernels, in the statistics' build_ms
    float ms = 0;
    if (sync_event(ev[1]) == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ctx->wide_join_stage_ms = ms;
  }
  // 6. without the code columns (deferred gathers nobody has read): [L | code | R | code] -> [L | R]
  auto drop = [&](size_t at) {
    out->cols.erase(out->cols.begin() + (std::ptrdiff_t)at);
    out->names.erase(out->names.begin() + (std::ptrdiff_t)at);
    out->nullable.erase(out->nullable.begin() + (std::ptrdiff_t)at);
  };
  const size_t nl = a.L->cols.size(), nr = a.R->cols.size();
  if (out->cols.size() > nl + 1) drop(nl + 1 + nr);   // (join types that emit the probe side)
  drop(nl);
  return out.release();
}

}  // namespace

extern "C" int qhip_hash_join_execute(qhip_ctx* ctx, const qhip_table* left, const qhip_table* right, int32_t join_type,
                                      const qhip_expr* left_exprs, int32_t n_left_exprs, const qhip_expr* right_exprs, int32_t n_right_exprs,
                                      const int32_t* on_left, const int32_t* on_right, int32_t n_on, const qhip_expr* filter_exprs,
                                      int32_t n_filter_exprs, int32_t filter_root, const int32_t* filter_sides, const int32_t* filter_cols,
                                      int32_t n_filter_cols, int32_t left_scan_filter_root, int32_t right_scan_filter_root, qhip_table** out) {
  if (!ctx || !left || !right || !out) return QHIP_INVALID_ARGUMENT;
  *out = nullptr;
  const JoinArgs a = {left, right, join_type, left_exprs, n_left_exprs, right_exprs, n_right_exprs, on_left, on_right, n_on, filter_exprs, n_filter_exprs,
                      filter_root, filter_sides, filter_cols, n_filter_cols, left_scan_filter_root, right_scan_filter_root};
  return guarded(ctx, [&] {
    try {
      ctx->wide_join_stage_ms = 0;
      const JoinTuning tune = read_join_tuning();
      const int wide_mode = ctx->wide_join_keys_mode >= 0 ? ctx->wide_join_keys_mode : tune.wide_keys;
      if (wide_mode > 0 && (*out = maybe_encode_wide_join_key(ctx, tune, wide_mode, a))) return;
      try {
        *out = hash_join(ctx, a, &tune);
      } catch (const Error& e) {
        // wide keys are on, yet the key that does not fit is computed: the encoding stage takes plain key columns only
        const std::string what = e.what();
        if (wide_mode == 1 && e.code == QHIP_UNSUPPORTED && !plain_join_keys(a) &&
            (what.find("wider than 8 words") != std::string::npos || what.find("longer than 55 bytes") != std::string::npos))
          fail(QHIP_UNSUPPORTED, what + " (wide join keys: computed join keys are not encoded)");
        throw;
      }
    } catch (...) {
      ctx->pending_sizes.clear();   // (joins of deferred size below: whatever they left is void with this call's input)
      throw;
    }
  });
}
