// agg.cpp — qhip_hash_aggregate_execute: HashAggregate / NoGroupingAggregate with the scan filter fused in.
//
// Reference: physical/plan/aggregate/hash.rs:138-170 (execute), :45-87 (GroupAccumulator::update),
// :89-107 (output); aggregate/no_grouping.rs:30-62; accumulators physical/expr/aggregate/*.rs;
// fused predicate = MemoryTable::scan (datasource/memory.rs:90-93) / Filter (physical/plan/filter.rs:28-44).
//
// hash_aggregate (the driver, at the end of the file) is the operator's outline; every stage is a function of this file:
//    1  validate_agg_args
//    2  maybe_encode_wide_key   a key that does not fit the packed key words: one group code per row, then hash_aggregate again on the code
//       maybe_prepartition      mid-sized input, many groups: rows ordered by key hash into parts, then hash_aggregate again over them
//    3  resolve_agg_inputs      deferred columns, Utf8 key lengths, |value| bounds, record copies
//    4  lookup_or_lower_plan    plan cache, twin-plan learning;  bind_plan_to_input: kernel arguments, sizes, page-locked scratch
//    5  decide_launch_shape     LDS slots, wide / cons / parts, grid, the first table's size and replicas
//    6  try_runs                the sorted-runs kernel (falls through to 7 when the input is not of that kind)
//    7  run_table_attempts      clear, kernel, compaction, ONE wait; x16 on overflow
//         launch_partitioned      the three-pass partitioned aggregate (launch_reduce: its reduce pass)
//         enqueue_collect         compaction, speculative device-side assembly, the combined read-back
//    8  collect_slots           dense slots to the host (replicas merged: agg_result.cpp) or kept on the device
//    9  enqueue_device_finalize + finish_device_finalize  |  assemble_host_columns (agg_result.cpp)
//   10  set_stats
// AggTuning holds every environment switch (read once per call), AggCall what is fixed for the call, AggRun what the attempts
// produce for the stages behind them.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "agg_result.hpp"
#include "codegen.hpp"
#include "common.hpp"
#include "device/qhip_status.h"
#include "hostcol.hpp"
#include "jit.hpp"
#include "kargs_host.hpp"
#include "kernels.hpp"
#include "relops.hpp"

namespace qhip {
static uint64_t g_learn_tick = 0;   // orders what twin aggregate plans learnt (AggPlan::learnt_at)

// A host-assembled column -> HBM (runs when a device operator first reads the column; no host wait: the host vectors are kept
// alive in a small ring until an event recorded behind the copies has passed)
DevColumn upload_host_column(Ctx* ctx, const DeferredUpload& u) {
  HostColumn& hc = *std::static_pointer_cast<HostColumn>(u.host_col);
  const int64_t nrows = hc.length;
  DevColumn dc;
  dc.type = hc.type; dc.length = nrows; dc.null_count = hc.null_count;
  auto up = [&](const void* src, size_t n) {
    auto b = std::make_shared<DevBuf>(n);
    if (n) QHIP_HIP_CHECK(hipMemcpyAsync(b->ptr, src, n, hipMemcpyHostToDevice, ctx->stream));
    return b;
  };
  if (hc.null_count > 0 && hc.type.id != QHIP_NULL) {
    hc.validity.resize((size_t)((nrows + 7) / 8 + 8), 0);
    dc.validity = up(hc.validity.data(), hc.validity.size());
  }
  if (hc.type.id == QHIP_UTF8) {
    dc.values = up(hc.offsets.data(), hc.offsets.size() * 4);
    dc.data = up(hc.data.data(), hc.data.size());
    dc.data_bytes = (int64_t)hc.data.size();
  } else if (hc.type.id == QHIP_BOOL) {
    hc.values.resize((size_t)((nrows + 7) / 8 + 8), 0);
    dc.values = up(hc.values.data(), hc.values.size());
  } else if (hc.type.id != QHIP_NULL) {
    dc.values = up(hc.values.data(), hc.values.size());
  }
  // the host vectors may go away with the DeferredUpload while the copies are still queued: park them behind an event
  Ctx::HostKeep& k = ctx->host_keep[ctx->host_keep_next++ % 32];
  if (!k.ev) QHIP_HIP_CHECK(hipEventCreateWithFlags(&k.ev, hipEventDisableTiming));
  else if (k.p && hipEventQuery(k.ev) != hipSuccess) { (void)hipGetLastError(); QHIP_HIP_CHECK(sync_event(k.ev)); }   // (32 uploads ago: long done)
  k.p = u.host_col;
  QHIP_HIP_CHECK(hipEventRecord(k.ev, ctx->stream));
  return dc;
}

// A single-batch (or zero-batch) table from host columns. The columns STAY on the host (an aggregate's few result rows
// are usually exported next, as the reference's results are host batches) and are uploaded when a device operator reads
// them (Sort / Limit / Projection over an aggregate, a join over a subquery result).
qhip_table* table_from_host(Ctx* ctx, const std::vector<std::string>& names, const std::vector<bool>& nullable,
                            std::vector<HostColumn>& cols, int64_t nrows, bool zero_batches) {
  std::unique_ptr<qhip_table> t(new qhip_table());
  t->ctx = ctx;
  t->names = names;
  t->nullable = nullable;
  t->num_rows = nrows;
  t->batch_offsets.push_back(0);
  if (!zero_batches) t->batch_offsets.push_back(nrows);
  for (auto& hc : cols) {
    DevColumn dc;
    dc.type = hc.type; dc.length = nrows; dc.null_count = hc.type.id == QHIP_NULL ? nrows : hc.null_count;
    hc.length = nrows;
    auto u = std::make_shared<DeferredUpload>();
    u->host_col = std::make_shared<HostColumn>(std::move(hc));
    dc.pending_upload = u;
    t->cols.push_back(std::move(dc));
  }
  return t.release();
}

// ---------------------------------------------------------------- helpers shared with other operators
std::vector<InputCol> input_cols_of(const qhip_table* t, bool mark_indirect) {
  std::vector<InputCol> v;
  for (auto& c0 : t->cols) {
    // a deferred column that nobody resolved is not referenced by the plan being typed: its may-have-nulls flag is enough
    const DevColumn& c = (c0.deferred && c0.deferred->done) ? c0.deferred->result : c0;
    InputCol ic; ic.type = c.type; ic.has_nulls = c.null_count > 0; ic.utf8_max_len = c.utf8_max_len;
    ic.indirect = mark_indirect && indirect_eligible(c0);
    if (ic.indirect) ic.has_nulls = false;   // (eligible = a source without NULLs and an index vector without NULL indices)
    v.push_back(ic);
  }
  return v;
}

void fill_kargs(Ctx* ctx, const qhip_table* t, const KernelBindings& b, HKArgs& a, DevBuf& strlit_dev) {
  memset(&a, 0, sizeof(a));
  for (size_t s = 0; s < b.cols.size(); ++s) {
    const DevColumn& c0 = t->cols[(size_t)b.cols[s]];
    if (s < b.indirect.size() && b.indirect[s]) {   // read through the deferred gather's index vector (InputCol::indirect)
      if (!indirect_eligible(c0)) fail(QHIP_HIP_ERROR, "a column planned as an indirect read has been gathered meanwhile (internal error)");
      a.c[s].v = c0.deferred->src.values->ptr;
      a.c[s].d = (const uint8_t*)index_rows(ctx, c0.deferred->idx);   // (looked up / composed now if it was owed)
      if (s < b.rec.size() && b.rec[s]) {   // ... as a field of the source's record copy (ColRange::rec_buf)
        const DevColumn& src = c0.deferred->src;
        const ColRange& sh = *src.range;
        const int w = s < b.narrow.size() && b.narrow[s] ? (int)b.narrow[s] : dtype_width(src.type);
        if (!sh.rec_buf || sh.rec_stride != (int)b.rec[s] || sh.rec_width != w || sh.rec_src != src.values->ptr || sh.rec_rows != src.length)
          fail(QHIP_HIP_ERROR, "an indirect column planned with a record copy has none of that layout (internal error)");
        a.c[s].v = (const uint8_t*)sh.rec_buf->ptr + sh.rec_offset;
        continue;
      }
      if (s < b.narrow.size() && b.narrow[s]) {   // ... from the source's narrow copy (the object every copy of the column shares)
        const DevColumn& src = c0.deferred->src;
        const ColRange& sh = *src.range;
        if (sh.narrow_buf && sh.narrow_bytes == (int)b.narrow[s] && sh.narrow_src == src.values->ptr && sh.narrow_rows == src.length) a.c[s].v = sh.narrow_buf->ptr;
        else if (src.narrow && src.narrow->buf && src.narrow->bytes == (int)b.narrow[s] && src.narrow->src == src.values->ptr && src.narrow->rows == src.length)
          a.c[s].v = src.narrow->buf->ptr;
        else fail(QHIP_HIP_ERROR, "an indirect column planned with a narrow copy has none of that width (internal error)");
      }
      continue;
    }
    const DevColumn& c = resolved(ctx, c0);
    a.c[s].v = c.values ? c.values->ptr : nullptr;
    if (s < b.narrow.size() && b.narrow[s]) {   // the kernel was generated for the column's narrow copy (InputCol::narrow_bytes)
      if (!c.narrow || c.narrow->bytes != (int)b.narrow[s] || !c.values || c.narrow->src != c.values->ptr || c.narrow->rows != c.length)
        fail(QHIP_HIP_ERROR, "a column planned with a narrow copy has none of that width (internal error)");
      a.c[s].v = c.narrow->buf->ptr;
    }
    a.c[s].n = c.validity ? (const uint8_t*)c.validity->ptr : nullptr;
    a.c[s].d = c.data ? (const uint8_t*)c.data->ptr : nullptr;
  }
  for (size_t l = 0; l < b.lit_lo.size(); ++l) { a.lit_lo[l] = b.lit_lo[l]; a.lit_hi[l] = b.lit_hi[l]; }
  for (size_t l = 0; l < b.stroff.size() && l < (size_t)kMaxLits + 1; ++l) a.stroff[l] = b.stroff[l];
  // (a caller that keeps strlit_dev with its cached plan uploads the literals once: same bindings, same bytes)
  if (!strlit_dev.ptr || strlit_dev.bytes != b.strlits.size()) {
    strlit_dev.alloc(b.strlits.size());
    if (!b.strlits.empty())
      QHIP_HIP_CHECK(hipMemcpyAsync(strlit_dev.ptr, b.strlits.data(), b.strlits.size(), hipMemcpyHostToDevice, ctx->stream));
  }
  a.strlit = (const uint8_t*)strlit_dev.ptr;
  a.nrows = t->num_rows;
  a.nrows_dev = t->rows_dev;   // (a join output whose size the host has not waited for: aggregate / join build only)
}

void check_status_words(const uint32_t* st) {
  if (st[QS_KEY_TOO_LONG]) fail(QHIP_UNSUPPORTED, "Utf8 group/join key longer than its packed key words (expression keys: 7 bytes)");
  if (st[QS_DIV_ZERO]) fail(QHIP_EXEC_ERROR, "Arrow error: Divide by zero error");
  if (st[QS_CAST_OVERFLOW]) fail(QHIP_EXEC_ERROR, "Arrow error: Cast error: value out of range for the target type");
  if (st[QS_ARITH_OVERFLOW]) fail(QHIP_EXEC_ERROR, "Arrow error: Arithmetic overflow: Overflow happened on integer division");
}

// ---------------------------------------------------------------- the operator's state
// The input of a mid-sized many-group aggregate, ordered by key hash into one part per workgroup (qk_filter_agg_parts reads part
// p = rows [runs[p * stride], runs[(p + 1) * stride]) of the view and appends its groups to the dense slots: AggLaunch)
struct AggParts { const uint32_t* runs; uint32_t stride; int n_parts; uint64_t hint_key; };

// Every environment switch of the aggregate, read ONCE at the top of a hash_aggregate call (per call, the recursive one over the
// parts included: tests flip them between executions of one process). Nothing below read_agg_tuning looks at the environment.
struct AggTuning {
  bool trace;                 // QHIP_TRACE set: print the host time of the call's stages (measurement)
  int parts_mode;             // QHIP_AGG_PARTS 0 never / 1 auto / 2 always: order a mid-sized input by key hash first (policy; 2 = tests)
  int partition_mode;         // QHIP_AGG_PARTITION 0 never / 1 when the last run says it pays / 2 always: the three-pass aggregate (policy; 2 = tests)
  bool collect_stats;         // QHIP_AGG_STATS: the fused kernel counts its LDS table's occupancy, and keeps to that kernel (measurement)
  bool value_bounds;          // QHIP_AGG_NO_BOUNDS=1 switches the |value| bounds of Int64 / Decimal128 columns off (test forcing)
  int64_t stats_min_rows;     // QHIP_STATS_MIN_ROWS: inputs from this size collect column statistics (policy; tests / the fuzzer lower it)
  int rows_per_thread;        // QHIP_AGG_R: rows per thread of the fused kernel, 0 = by rule (measurement; part of the plan key)
  int hot_keys;               // QHIP_AGG_KC: wave-resident hot keys, -1 = by rule (measurement; part of the plan key)
  bool wide;                  // QHIP_AGG_WIDE=0: never the 1 024-thread fused kernel (test forcing)
  EnvInt lds_bytes;           // QHIP_AGG_LDS_BYTES: LDS budget of the fused kernel's table (test forcing: small tables spill); set at all,
                              // even to nothing: the three-pass reduce keeps the fused kernel's table size
  bool cons;                  // QHIP_AGG_CONS=0: never the consecutive-rows kernel (test forcing)
  EnvInt blocks_per_cu;       // QHIP_AGG_BLOCKS_PER_CU: workgroups per CU of the fused kernel (measurement)
  int initial_slots;          // QHIP_AGG_INITIAL_SLOTS: slots of the first, replicated table (test forcing: overflow and retry)
  int replicas;               // QHIP_AGG_REPLICAS (>= 1): copies of the first table (policy; 1 = tests)
  uint32_t dev_threshold;     // QHIP_AGG_DEVICE_FINALIZE_MIN_GROUPS: from this many groups the output is assembled on the device (policy; 1 = tests)
  int runs_mode;              // QHIP_AGG_RUNS 0 never / 1 by rule / 2 whenever the plan can: the sorted-runs kernel (policy; 2 = tests)
  uint32_t runs_max;          // QHIP_AGG_RUNS_MAX (>= 16): longest run that kernel follows (test forcing)
  EnvInt runs_lds_kb;         // QHIP_AGG_RUNS_LDS_KB: its dynamic LDS (test forcing: the look-ahead's lower limit)
  bool runs_debug;            // QHIP_AGG_RUNS_DEBUG: say why the runs kernel gave up (measurement)
  bool speculative_finalize;  // QHIP_AGG_NO_SPECULATIVE_FINALIZE=1 switches the speculative device-side assembly off (test forcing)
  bool arena;                 // QHIP_AGG_NO_ARENA=1 switches the persistent first-attempt arena off (test forcing)
  bool partition_mid;         // QHIP_AGG_PARTITION_MID: the three passes on mid-sized inputs too, work items computed on the device (policy, off)
  bool part_wide;             // QHIP_AGG_PART_WIDE=0: the 256-thread reduce pass (test forcing)
  EnvInt part_lds_bytes;      // QHIP_AGG_PART_LDS_BYTES: LDS budget of the reduce pass's tables (measurement)
  int part_bins;              // QHIP_AGG_PART_BINS (>= 16 to count): bins of the three-pass aggregate (test forcing)
  int part_wgs_per_cu;        // QHIP_AGG_PART_WGS_PER_CU (>= 1): workgroups per CU of its passes 1 and 2 (measurement)
  bool part_stage;            // QHIP_AGG_PART_STAGE=0: the plain scatter instead of the LDS-staged pass 2 (test forcing)
  uint32_t part_slices;       // QHIP_AGG_PART_SLICES (>= 1): slices per bin of the device-computed work items (measurement)
  EnvInt partition_item;      // QHIP_AGG_PARTITION_ITEM: records per host-computed work item, at least 4 096 (measurement)
  int parts_max_factor;       // QHIP_AGG_PARTS_MAX_FACTOR: a part of more than this many times the average is sliced (policy)
  bool pinned_slots;          // QHIP_AGG_PINNED_SLOTS=0: the first dense slots come back by copy, not straight from the compaction (measurement)
  bool prof;                  // QHIP_AGG_PROF: print the fused kernel's phase timers (measurement; needs a kernel built with P::PROF)
  int wide_keys;              // QHIP_AGG_WIDE_KEYS 0 never / 1 when the packed key does not fit / 2 every grouped aggregate over plain key
                              // columns: keys encoded to group codes first (policy, off; 2 = tests) — the context's own mode goes first
  int wide_key_hash_bits;     // QHIP_AGG_WIDE_KEY_HASH_BITS (1..63): only so many bits of the encoding's hash (test forcing: long probe chains)
};
static AggTuning read_agg_tuning() {
  AggTuning t;
  t.trace = getenv("QHIP_TRACE") != nullptr;
  t.parts_mode = env_int("QHIP_AGG_PARTS", 1);
  t.partition_mode = env_int("QHIP_AGG_PARTITION", 1);
  t.collect_stats = env_int("QHIP_AGG_STATS", 0) != 0;
  t.value_bounds = env_int("QHIP_AGG_NO_BOUNDS", 0) == 0;
  t.stats_min_rows = (int64_t)env_int("QHIP_STATS_MIN_ROWS", 1 << 22);
  t.rows_per_thread = env_int("QHIP_AGG_R", 0);
  t.hot_keys = env_int("QHIP_AGG_KC", -1);
  t.wide = env_int("QHIP_AGG_WIDE", 1) != 0;
  t.lds_bytes = env_opt("QHIP_AGG_LDS_BYTES");
  t.cons = env_int("QHIP_AGG_CONS", 1) != 0;
  t.blocks_per_cu = env_opt("QHIP_AGG_BLOCKS_PER_CU");
  t.initial_slots = env_int("QHIP_AGG_INITIAL_SLOTS", 4096);
  t.replicas = std::max(1, env_int("QHIP_AGG_REPLICAS", 32));
  t.dev_threshold = (uint32_t)env_int("QHIP_AGG_DEVICE_FINALIZE_MIN_GROUPS", 4096);
  t.runs_mode = env_int("QHIP_AGG_RUNS", 1);
  t.runs_max = (uint32_t)std::max(16, env_int("QHIP_AGG_RUNS_MAX", 256));
  t.runs_lds_kb = env_opt("QHIP_AGG_RUNS_LDS_KB");
  t.runs_debug = env_int("QHIP_AGG_RUNS_DEBUG", 0) != 0;
  t.speculative_finalize = env_int("QHIP_AGG_NO_SPECULATIVE_FINALIZE", 0) == 0;
  t.arena = env_int("QHIP_AGG_NO_ARENA", 0) == 0;
  t.partition_mid = env_int("QHIP_AGG_PARTITION_MID", 0) != 0;
  t.part_wide = env_int("QHIP_AGG_PART_WIDE", 1) != 0;
  t.part_lds_bytes = env_opt("QHIP_AGG_PART_LDS_BYTES");
  t.part_bins = env_int("QHIP_AGG_PART_BINS", 0);
  t.part_wgs_per_cu = std::max(1, env_int("QHIP_AGG_PART_WGS_PER_CU", 4));
  t.part_stage = env_int("QHIP_AGG_PART_STAGE", 1) != 0;
  t.part_slices = (uint32_t)std::max(1, env_int("QHIP_AGG_PART_SLICES", 8));
  t.partition_item = env_opt("QHIP_AGG_PARTITION_ITEM");
  t.parts_max_factor = env_int("QHIP_AGG_PARTS_MAX_FACTOR", 4);
  t.pinned_slots = env_int("QHIP_AGG_PINNED_SLOTS", 1) != 0;
  t.prof = env_int("QHIP_AGG_PROF", 0) != 0;
  t.wide_keys = env_int("QHIP_AGG_WIDE_KEYS", 0);
  t.wide_key_hash_bits = env_int("QHIP_AGG_WIDE_KEY_HASH_BITS", 0);
  return t;
}

// What is fixed for one hash_aggregate call once its plan is bound to its input.
struct AggCall {
  Ctx* ctx = nullptr;
  const qhip_table* in = nullptr;
  const AggParts* parts = nullptr;
  AggTuning tune;
  int n_groups = 0, n_aggs = 0;
  uint64_t hint_key = 0;
  std::shared_ptr<AggPlan> plan_ptr;
  std::shared_ptr<Module> mod;             // the plan's main kernel
  HKArgs ka;
  std::vector<std::string> names;          // output schema: keys then aggregates (hash.rs:166-169)
  std::vector<bool> nullable;
  bool zero_batches_in = false;
  int64_t N = 0;
  double bytes_per_row = 0;                // column data the kernel reads per row (for roofline figures)
  int slot_bytes = 0;
  int cell0 = 0;                           // first cell word of a slot
  // the context's page-locked scratch: [status words + counter (64 bytes) | dense slots fetched with them ... | the last 1 024
  // bytes: status words (8) + null counts (<= 248) of a device-side assembly that reads back on its own]
  uint32_t* status_pinned = nullptr;
  uint64_t* pre_host = nullptr;
  uint32_t* fin_pinned = nullptr;
  uint32_t PRE = 0;                        // dense slots that can come back with the status words (one sync)
  std::chrono::steady_clock::time_point t_begin;

  const AggPlan& plan() const { return *plan_ptr; }
  int ncols() const { return n_groups + n_aggs; }
  void* kargs() const { return const_cast<HKArgs*>(&ka); }   // (an element of a launch's argument array: the runtime only reads it)
  void mark(const char* what) const {
    if (tune.trace) fprintf(stderr, "[qhip agg] %-28s %8.1f us\n", what,
                            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_begin).count());
  }
};

// ---- output assembly on the device for many groups (k_agg_finalize): nothing but a few counters crosses PCIe.
struct DevFinal {
  std::unique_ptr<qhip_table> out;
  std::vector<FinCol> fc;
  DevBuf fc_dev;
  const uint32_t* fin_host = nullptr;   // page-locked [status words | null counts] of this finalisation
  std::vector<std::shared_ptr<DevBuf>> valid_bufs;
  bool has_utf8 = false;
};

enum AggKernel { AGG_FUSED = 0, AGG_RUNS, AGG_PARTITIONED };   // (the fused family: plain / wide / cons / parts, by the launch shape)

// The launch shape the call decided on, and what its attempts produced for the stages behind them.
struct AggRun {
  // shape (decide_launch_shape; the attempts grow cap and drop the replicas on overflow)
  uint32_t l_nslots = 0;        // slots of a workgroup's LDS table (0: the slot is too wide for LDS staging)
  bool wide = false, cons = false;
  int block = 256;
  unsigned grid = 1;
  uint32_t cap_max = 1, cap = 1, replicas = 1;
  // attempts
  AggKernel kernel = AGG_FUSED;
  uint32_t guess = 0;           // dense slots there is room for
  DevBuf gtable, dense;
  uint64_t* table_dev = nullptr;
  uint64_t* dense_dev = nullptr;    // [counter | dense slots]
  uint32_t pre_copied = 0;      // dense slots that came back with the status words
  DevFinal spec;                // speculative device-side assembly enqueued behind the compaction
  bool spec_enqueued = false;
  uint32_t status[QS_WORDS];
  int retries = 0;
  float main_ms = 0;
};

static uint64_t agg_hint_key(const qhip_expr* exprs, int n_exprs, int pred_root, const int32_t* group_roots, int n_groups, const qhip_agg* aggs, int n_aggs) {
  uint64_t h = 1469598103934665603ULL;
  auto mix = [&](const void* p, size_t n) { for (size_t k = 0; k < n; ++k) { h ^= ((const unsigned char*)p)[k]; h *= 1099511628211ULL; } };
  for (int k = 0; k < n_exprs; ++k) {
    qhip_expr e = exprs[k];
    const char* str = e.lit_str; const int64_t len = e.lit_len;
    e.lit_str = nullptr;
    mix(&e, sizeof e);
    if (str && len > 0 && e.kind == QHIP_EXPR_LITERAL) mix(str, (size_t)len);
  }
  mix(&pred_root, sizeof pred_root);
  mix(group_roots, sizeof(int32_t) * (size_t)n_groups);
  mix(aggs, sizeof(qhip_agg) * (size_t)n_aggs);
  return h;
}

static qhip_table* hash_aggregate(Ctx* ctx, const qhip_table* in, const qhip_expr* exprs, int n_exprs, int pred_root,
                                  const int32_t* group_roots, int n_groups, const qhip_agg* aggs, int n_aggs,
                                  const char* const* out_names, const AggParts* parts = nullptr, bool key_encoded = false);

// ---------------------------------------------------------------- stage 1: validate
static void validate_agg_args(const qhip_expr* exprs, int n_exprs, int pred_root, const int32_t* group_roots, int n_groups,
                              const qhip_agg* aggs, int n_aggs) {
  if (n_groups < 0 || n_aggs < 0 || (n_groups > 0 && !group_roots) || (n_aggs > 0 && !aggs) || (n_exprs > 0 && !exprs))
    fail(QHIP_INVALID_ARGUMENT, "qhip_hash_aggregate_execute: bad arguments");
  for (int k = 0; k < n_groups; ++k)
    if (group_roots[k] < 0 || group_roots[k] >= n_exprs) fail(QHIP_INVALID_ARGUMENT, "group expression index out of range");
  if (pred_root >= n_exprs) fail(QHIP_INVALID_ARGUMENT, "predicate index out of range");
}

// ---------------------------------------------------------------- stage 2: wide group keys
// The reference hashes group keys of any length and any number of columns (utils/array.rs:171-210); a packed key has 8 words (a
// Utf8 key 7 of them). A key that does not fit never reaches the aggregate: k_widekey_encode (device/qhip_widekey.inc) gives every
// row the number of ONE row with the same key — exact, the keys themselves are compared — and hash_aggregate runs again, with
// all its paths, over a view of the input whose one group key is that Int32 column. The result's code column is then the index
// vector through which the key columns are gathered from the input (deferred, validity included). 16 bytes of HBM per input row
// (the slot table, twice the rows) + 4 for the codes while the stage runs. Rows the scan predicate drops are encoded for nothing.
// mode 1: when the packed key does not fit; 2: every grouped aggregate whose keys are plain columns (tests, fuzzing).
// Returns the result, or nullptr when the input is aggregated as it is.
static bool plain_column_keys(const qhip_table* in, const qhip_expr* exprs, const int32_t* group_roots, int n_groups) {
  for (int k = 0; k < n_groups; ++k) {
    const qhip_expr& e = exprs[group_roots[k]];
    if (e.kind != QHIP_EXPR_COLUMN || e.column < 0 || e.column >= (int)in->cols.size()) return false;
  }
  return true;
}
static qhip_table* maybe_encode_wide_key(Ctx* ctx, const AggTuning& tune, int mode, const qhip_table* in, const qhip_expr* exprs, int n_exprs,
                                         int pred_root, const int32_t* group_roots, int n_groups, const qhip_agg* aggs, int n_aggs,
                                         const char* const* out_names) {
  if (mode <= 0 || n_groups <= 0 || !plain_column_keys(in, exprs, group_roots, n_groups)) return nullptr;
  std::vector<int32_t> key_cols((size_t)n_groups);
  for (int k = 0; k < n_groups; ++k) key_cols[(size_t)k] = exprs[group_roots[k]].column;
  for (int32_t col : key_cols) check_key_type(in->cols[(size_t)col].type);
  if (mode == 1) {   // (what resolve_agg_inputs is about to do anyway: nothing is gathered or measured twice)
    resolve_referenced(ctx, in, exprs, n_exprs, true);
    std::vector<InputCol> icols = input_cols_of(in, true);
    ensure_utf8_key_lengths(ctx, in, exprs, n_exprs, group_roots, n_groups, icols);
    if (packed_key_fits(icols, key_cols.data(), n_groups)) return nullptr;
  }
  if (n_groups > kWideKeyCols) fail(QHIP_UNSUPPORTED, "group key of more than 32 columns is not accelerated");
  // 1. an exact row count, the key columns materialised
  const bool deferred_size = in->rows_dev != nullptr;
  settle_rows(in);
  const int64_t N = in->num_rows;
  if (N > ((int64_t)1 << 30)) fail(QHIP_UNSUPPORTED, "wide group key over more than 2^30 input rows is not accelerated");
  // (a join of deferred size that produced nothing has no output batches, hash_join.rs:363-372)
  const bool zero_batches = in->no_batches() || (deferred_size && N == 0);
  WideKeyCols wk;
  memset(&wk, 0, sizeof wk);
  std::vector<DevColumn> keys;
  for (int k = 0; k < n_groups; ++k) {
    const DevColumn& c = resolved(ctx, in->cols[(size_t)key_cols[(size_t)k]]);
    WideKeyCol& d = wk.c[k];
    d.v = c.values ? c.values->ptr : nullptr;
    d.d = c.data ? c.data->as<uint8_t>() : nullptr;
    d.n = c.validity ? c.validity->as<uint8_t>() : nullptr;
    d.width = (uint32_t)dtype_width(c.type);   // (0: Utf8 — check_key_type has let nothing else without a width through)
    keys.push_back(c);
  }
  // 2. the codes
  auto code = std::make_shared<DevBuf>((size_t)N * 4);
  const uint32_t nslots = std::max<uint32_t>(1024, pow2_ceil32((uint64_t)std::max<int64_t>(N, 1) * 2));
  DevBuf table((size_t)nslots * 8);
  struct Events {   // (timings asked for: a pair of the stage's own — the aggregate behind it records the context's)
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipEvent_t operator[](int k) const { return e[k]; }
  } ev;
  if (ctx->timing) for (hipEvent_t& e : ev.e) { QHIP_HIP_CHECK(hipEventCreate(&e)); }
  if (N > 0) {
    if (ev[0]) (void)hipEventRecord(ev[0], ctx->stream);
    QHIP_HIP_CHECK(hipMemsetAsync(table.ptr, 0, (size_t)nslots * 8, ctx->stream));
    const int bits = tune.wide_key_hash_bits;
    launch_widekey_encode(wk, n_groups, table.as<uint64_t>(), nslots, bits > 0 && bits < 64 ? (1ULL << bits) - 1 : ~0ULL, code->as<int32_t>(), (uint64_t)N, ctx->stream);
    if (ev[1]) (void)hipEventRecord(ev[1], ctx->stream);
  }
  // 3. the input's columns + the code column; 4. the one group key is that column
  qhip_table view;
  view.ctx = ctx;
  view.names = in->names;
  view.nullable = in->nullable;
  view.cols = in->cols;
  view.num_rows = N;
  view.batch_offsets.assign(1, 0);
  if (!zero_batches) view.batch_offsets.push_back(N);
  DevColumn cc;
  cc.type = DType(QHIP_INT32); cc.length = N; cc.values = code;
  view.names.push_back("group_code");
  view.nullable.push_back(false);
  view.cols.push_back(std::move(cc));
  std::vector<qhip_expr> ex(exprs, exprs + n_exprs);
  qhip_expr ce;
  memset(&ce, 0, sizeof ce);
  ce.kind = QHIP_EXPR_COLUMN; ce.column = (int32_t)in->cols.size(); ce.left = ce.right = ce.third = -1;
  ex.push_back(ce);
  const int32_t code_root = n_exprs;
  // The key columns' own nodes stay in the array. Whatever the predicate and the aggregates do not reach must not count as a
  // reference any more — every operator below gathers or uploads the columns its expression array names, and a pre-partitioned
  // input would gather the wide Utf8 keys through its selection vector — so those Column nodes now name the code column.
  {
    std::vector<char> reached((size_t)n_exprs, 0);
    std::vector<int32_t> todo;
    if (pred_root >= 0) todo.push_back(pred_root);
    for (int k = 0; k < n_aggs; ++k) todo.push_back(aggs[k].expr);
    while (!todo.empty()) {
      const int32_t k = todo.back();
      todo.pop_back();
      if (k < 0 || k >= n_exprs || reached[(size_t)k]) continue;
      reached[(size_t)k] = 1;
      todo.push_back(ex[(size_t)k].left); todo.push_back(ex[(size_t)k].right); todo.push_back(ex[(size_t)k].third);
    }
    for (int k = 0; k < n_exprs; ++k)
      if (!reached[(size_t)k] && ex[(size_t)k].kind == QHIP_EXPR_COLUMN) ex[(size_t)k].column = ce.column;
  }
  std::vector<std::string> names;
  for (int k = 0; k < n_groups + n_aggs; ++k) names.push_back(out_names && out_names[k] ? out_names[k] : ("col" + std::to_string(k)));
  std::vector<const char*> inner_names{"group_code"};
  for (int k = 0; k < n_aggs; ++k) inner_names.push_back(names[(size_t)(n_groups + k)].c_str());
  // 5. the aggregate itself, unchanged (scan predicate and aggregate list as they came)
  std::unique_ptr<qhip_table> res(hash_aggregate(ctx, &view, ex.data(), n_exprs + 1, pred_root, &code_root, 1, aggs, n_aggs, inner_names.data(), nullptr, true));
  ++ctx->wide_key_aggregates;
  if (ev[0] && N > 0) {   // the stage's memset + kernel, in the statistics' build_ms
    float ms = 0;
    if (sync_event(ev[1]) == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ctx->stats.build_ms = ms;
  }
  // 6. [code, aggregates ...] -> [the key columns at the representative rows, aggregates ...]
  const int64_t G = res->num_rows;
  std::unique_ptr<qhip_table> out(new qhip_table());
  out->ctx = ctx;
  out->names = names;
  out->nullable.assign(names.size(), true);
  out->num_rows = G;
  out->batch_offsets = res->offsets();
  if (G > 0) {
    const DevColumn& rc = resolved(ctx, res->cols[0]);   // (few groups: assembled on the host, uploaded here)
    defer_gather(ctx, keys, rc.values, (uint64_t)G, false, out->cols);
  } else {
    std::vector<HostColumn> hk((size_t)n_groups);
    for (int k = 0; k < n_groups; ++k) hk[(size_t)k].init_fixed(keys[(size_t)k].type, 0);
    std::unique_ptr<qhip_table> empty(table_from_host(ctx, std::vector<std::string>(names.begin(), names.begin() + n_groups), std::vector<bool>((size_t)n_groups, true), hk, 0, true));
    for (auto& c : empty->cols) out->cols.push_back(std::move(c));
  }
  for (size_t k = 1; k < res->cols.size(); ++k) out->cols.push_back(std::move(res->cols[k]));
  return out.release();
}

// ---------------------------------------------------------------- stage 2: pre-partitioning
// Mid-sized input, many groups (the same aggregate produced them last time): order the rows by key hash into one part per
// workgroup first — the exchange's two partition passes over the ROW NUMBERS (nothing but the parts' selection vector is
// written; the columns are then read through it, composed with whatever index vectors a join below left) — and aggregate
// every part in its workgroup's LDS table alone: no group is shared between workgroups, so nothing is merged into the HBM
// table and no LDS table overflows (configs[4]'s per-rank aggregate, 2 M joined rows -> 200 k groups: round 3 spent 46 % of
// the kernel merging ~1.5 M (workgroup, group) pairs with memory-side atomics). QHIP_AGG_PARTS: 0 never, 1 auto, 2 always.
// Returns the result of the recursive call over the parts, or nullptr when the input is aggregated as it is.
static qhip_table* maybe_prepartition(Ctx* ctx, const AggTuning& tune, uint64_t hint_key, const qhip_table* in, const qhip_expr* exprs, int n_exprs,
                                      int pred_root, const int32_t* group_roots, int n_groups, const qhip_agg* aggs, int n_aggs,
                                      const char* const* out_names) {
  if (n_groups <= 0 || pred_root >= 0 || in->no_batches()) return nullptr;
  const int mode = tune.parts_mode;
  const auto hint = ctx->agg_group_hints.find(hint_key);
  const uint32_t groups_hint = hint != ctx->agg_group_hints.end() ? hint->second : 0u;
  const int64_t N0 = in->num_rows;
  // Only over plain columns. A join output read through index vectors pays ~64 bytes of random sector traffic per row and
  // referenced column; ordering the rows first makes the key columns pay it twice (pass 1 and the aggregate) — measured on
  // configs[4]'s per-rank aggregate (2 M joined rows, 5 columns through 2 index vectors, Zipf keys): pass 1 141 us + pass 2 /
  // index composition 67 us + aggregate 347 us against 307 us for the unpartitioned kernel, whose own floor those gathers
  // are (profiles/r04_q3_sf100_slice_parts_timeline.txt). What that input needs is the aggregate's arguments evaluated where
  // the pairs are emitted (a dense record stream), not another pass over the index vectors.
  bool plain_input = !in->rows_dev;
  for (int k = 0; k < n_exprs; ++k)
    if (exprs[k].kind == QHIP_EXPR_COLUMN && exprs[k].column >= 0 && exprs[k].column < (int)in->cols.size() && in->cols[(size_t)exprs[k].column].deferred)
      plain_input = false;
  const bool three_pass_forced = tune.partition_mode == 2;   // (tests: the three-pass partitioned path keeps precedence)
  // (from 2^20 rows: below, the five launches in front of the kernel cost what the merges did — Q3 at SF10, 0.34 M rows -> 113 k
  // groups: 118 us against 59)
  const bool by_rule = mode == 1 && plain_input && groups_hint >= 16384 && N0 >= ((int64_t)1 << 20) && N0 <= ((int64_t)1 << 22) && !tune.collect_stats;
  if (three_pass_forced || !(mode == 2 ? N0 > 0 : by_rule)) return nullptr;
  // parts: a 1 024-thread workgroup's LDS table (128 KB) at a load of ~0.4
  int slot_words_guess = 8;
  { const auto sw = ctx->agg_slot_words.find(hint_key); if (sw != ctx->agg_slot_words.end()) slot_words_guess = sw->second; }
  uint32_t lslots = 16;
  while ((uint64_t)lslots * 2 * (uint64_t)slot_words_guess * 8 <= 128 * 1024) lslots *= 2;
  // (at least ~3/4 of the CUs' worth of parts: a part is one workgroup's work)
  const int np = (int)std::max<uint64_t>(mode == 2 ? 2 : std::min<uint64_t>(255, (uint64_t)ctx->num_cus * 3 / 4),
                                         std::min<uint64_t>(255, ((uint64_t)std::max<uint32_t>(groups_hint, 1) * 5 / 2 + lslots - 1) / lslots));
  PartitionWork w;
  partition_pass1(ctx, in, exprs, n_exprs, group_roots, n_groups, -1, np, w);
  std::vector<MovedColumn> moved;
  std::vector<size_t> odd;
  std::shared_ptr<DevBuf> sel;
  partition_scatter(ctx, in, nullptr, np, w, (uint64_t)N0, moved, odd, sel, true);
  qhip_table view;
  view.ctx = ctx;
  view.names = in->names;
  view.nullable = in->nullable;
  view.num_rows = N0;
  view.batch_offsets = {0, N0};
  defer_gather(ctx, in->cols, sel, (uint64_t)N0, false, view.cols);
  AggParts ap{w.runs.as<uint32_t>(), w.n_units, np, hint_key};
  qhip_table* out = hash_aggregate(ctx, &view, exprs, n_exprs, pred_root, group_roots, n_groups, aggs, n_aggs, out_names, &ap);
  ctx->stats.rows_in = in->rows_dev ? in->deferred_count() : N0;
  // a join of deferred size that turned out to have produced nothing has no output batches (hash_join.rs:363-372)
  if (in->rows_dev && in->deferred_count() == 0 && out->num_rows == 0) { out->batch_offsets.assign(1, 0); out->pending_offsets.reset(); }
  return out;   // (w / sel go back to the stream-ordered pool: whoever gets them next runs behind the kernels that read them)
}

// ---------------------------------------------------------------- stage 3: inputs and statistics
static std::vector<InputCol> resolve_agg_inputs(Ctx* ctx, const AggTuning& tune, const qhip_table* in, const qhip_expr* exprs, int n_exprs,
                                                const int32_t* group_roots, int n_groups) {
  // (late materialisation: the plain deferred gathers of a join output are read through their index vectors by the kernel)
  resolve_referenced(ctx, in, exprs, n_exprs, true);
  std::vector<InputCol> icols = input_cols_of(in, true);
  ensure_utf8_key_lengths(ctx, in, exprs, n_exprs, group_roots, n_groups, icols);
  // |value| bounds of the Int64 / Decimal128 columns (cached per column; computed only on inputs big enough to pay for the
  // reduction): the generated code multiplies and accumulates in 32 / 64 bits where the bounds allow
  if (tune.value_bounds) ensure_value_bounds(ctx, in, exprs, n_exprs, icols, tune.stats_min_rows);
  // columns read through one index vector: one record per row and source table instead of one array per column
  ensure_indirect_records(ctx, in, exprs, n_exprs, icols, tune.stats_min_rows);
  return icols;
}

// ---------------------------------------------------------------- stage 4: the plan
// Lowered plans are cached per context: a repeated query (same expression PODs over the same column signature) skips
// typing and code generation; literal VALUES are part of the key because they are bound into the plan's KernelBindings
static std::shared_ptr<AggPlan> lookup_or_lower_plan(Ctx* ctx, const AggTuning& tune, const qhip_table* in, const std::vector<InputCol>& icols,
                                                     const qhip_expr* exprs, int n_exprs, int pred_root, const int32_t* group_roots, int n_groups,
                                                     const qhip_agg* aggs, int n_aggs) {
  std::string key = "agg|";
  auto put = [&](const void* p, size_t n) { key.append((const char*)p, n); };
  for (auto& ic : icols) {
    const int v[9] = {ic.type.id, ic.type.precision, ic.type.scale, ic.has_nulls ? 1 : 0, ic.utf8_max_len, ic.utf8_fixed1 ? 1 : 0, ic.indirect ? 1 : 0, ic.narrow_bytes, ic.rec_stride};
    put(&ic.value_maxabs, sizeof ic.value_maxabs);   // (a whole number of bits, see ensure_value_bounds)
    put(v, sizeof v);
  }
  for (int k = 0; k < n_exprs; ++k) {
    qhip_expr e = exprs[k];
    const char* str = e.lit_str; const int64_t len = e.lit_len;
    e.lit_str = nullptr;
    put(&e, sizeof e);
    if (str && len > 0 && e.kind == QHIP_EXPR_LITERAL) put(str, (size_t)len);
  }
  put(&pred_root, sizeof pred_root);
  put(group_roots, sizeof(int32_t) * (size_t)n_groups);
  put(aggs, sizeof(qhip_agg) * (size_t)n_aggs);
  // rows per thread: the register-budget rule of plan_aggregate (R = 2..4) suits inputs that fill the chip many times
  // over; a SMALL input (the 0.3 M joined rows Q3 aggregates) is a latency chain per row — fewer rows per thread and more
  // workgroups shorten it (Q3's aggregate kernel: 73 -> 49 us)
  const int64_t small_rows = (int64_t)256 * ctx->num_cus * 8;
  const int r_env = tune.rows_per_thread ? tune.rows_per_thread : in->num_rows <= small_rows ? 1 : in->num_rows <= 2 * small_rows ? 2 : 0;
  const int kc_env = tune.hot_keys;
  put(&r_env, sizeof r_env); put(&kc_env, sizeof kc_env);
  const int dev_rows = in->rows_dev ? 1 : 0;   // (a join output of deferred size: the kernel variant that reads the row count on the device)
  std::string sibling_key = key;
  put(&dev_rows, sizeof dev_rows);
  { const int other = 1 - dev_rows; sibling_key.append((const char*)&other, sizeof other); }
  std::shared_ptr<AggPlan> plan_ptr;
  auto cached = ctx->plan_cache.find(key);
  if (cached != ctx->plan_cache.end()) plan_ptr = std::static_pointer_cast<AggPlan>(cached->second);
  else {
    ExprSet es;
    es.build(exprs, n_exprs, icols);
    plan_ptr = std::make_shared<AggPlan>();
    plan_aggregate(es, icols, pred_root, group_roots, n_groups, aggs, n_aggs, r_env, *plan_ptr, dev_rows != 0);

    if (ctx->plan_cache.size() > 4096) ctx->plan_cache.clear();
    ctx->plan_cache[key] = plan_ptr;
  }
  // the same aggregate over an input whose row count is / is not on the device is a twin plan (another kernel variant):
  // what either learnt about the data (groups, occupied slots) serves both
  const AggPlan& plan = *plan_ptr;
  auto sib = ctx->plan_cache.find(sibling_key);
  if (sib != ctx->plan_cache.end()) {
    const AggPlan& o = *std::static_pointer_cast<AggPlan>(sib->second);
    if (o.learnt_at > plan.learnt_at) { plan.last_groups = o.last_groups; plan.last_dense = o.last_dense; plan.learnt_at = o.learnt_at; }
  }
  return plan_ptr;
}

// the plan's kernel and its arguments over this input, the sizes every later stage uses, the page-locked scratch
static void bind_plan_to_input(AggCall& c, const std::vector<InputCol>& icols) {
  Ctx* ctx = c.ctx;
  const AggPlan& plan = c.plan();
  if (!plan.module) plan.module = get_module(ctx, plan.source, plan.kernel_name);
  c.mod = std::static_pointer_cast<Module>(plan.module);
  if (!plan.strlit) plan.strlit = std::make_shared<DevBuf>();
  DevBuf& strlit = *std::static_pointer_cast<DevBuf>(plan.strlit);
  fill_kargs(ctx, c.in, plan.bind, c.ka, strlit);
  c.mark("module + kargs");

  const int64_t N = c.N = c.in->num_rows;
  c.bytes_per_row = 0;
  for (int col : plan.bind.cols) {
    const DevColumn& dc = c.in->cols[(size_t)col];
    const int w = dtype_width(dc.type);
    if (w > 0) c.bytes_per_row += icols[(size_t)col].narrow_bytes ? icols[(size_t)col].narrow_bytes : w;
    else if (dc.type.id == QHIP_BOOL) c.bytes_per_row += 0.125;
    else if (dc.type.id == QHIP_UTF8) c.bytes_per_row += icols[(size_t)col].utf8_fixed1 ? 1.0 : 4.0 + (N > 0 ? (double)dc.data_bytes / (double)N : 0.0);
    if (dc.null_count > 0) c.bytes_per_row += 0.125;
  }
  c.slot_bytes = plan.slot_words * 8;
  c.cell0 = 1 + plan.W;
  // dense slots fetched together with the status words (one sync), through the context's page-locked scratch
  // (256 of them, or what the plan produced last time plus a quarter while that stays a host-side result)
  const size_t pre_want = plan.last_groups > 4096 ? 256 : std::max<size_t>(256, std::min<size_t>(4096, (size_t)plan.last_dense + (size_t)plan.last_dense / 4));
  c.PRE = (uint32_t)std::min<size_t>(pre_want, (ctx->pinned_bytes - 64 - 8 - 1024) / (size_t)c.slot_bytes);
  c.status_pinned = (uint32_t*)ctx->pinned;
  c.pre_host = (uint64_t*)((uint8_t*)ctx->pinned + 64);
  c.fin_pinned = (uint32_t*)((uint8_t*)ctx->pinned + ctx->pinned_bytes - 1024);   // [status words (8) | null counts (<= 248)]
}

static qhip_table* no_batches_out(const AggCall& c) {   // hash.rs:146-148: no input batches -> no output batches
  std::vector<HostColumn> cols((size_t)c.ncols());
  for (int k = 0; k < c.n_groups; ++k) cols[(size_t)k].init_fixed(c.plan().keys[(size_t)k].type, 0);
  for (int k = 0; k < c.n_aggs; ++k) cols[(size_t)(c.n_groups + k)].init_fixed(c.plan().aggs[(size_t)k].ret, 0);
  return table_from_host(c.ctx, c.names, c.nullable, cols, 0, true);
}

// ---------------------------------------------------------------- stage 5: the launch shape
static void decide_launch_shape(const AggCall& c, AggRun& r) {
  Ctx* ctx = c.ctx;
  const AggPlan& plan = c.plan();
  const AggTuning& tune = c.tune;
  const int64_t N = c.N;
  const int slot_bytes = c.slot_bytes;
  // LDS-staged table: as many slots as fit the per-workgroup LDS budget
  if (plan.W > 0) {
    // Many groups (the plan's previous run says so) on a mid-sized input: every workgroup's LDS table ends up full and is
    // merged slot by slot into the HBM table at the end, the heavy keys by EVERY workgroup — same-slot atomic traffic that
    // grows with the number of workgroups, and with ~1000 workgroups x 512 slots as many HBM updates as the input has
    // rows. One workgroup per CU with a 64 KB table halves the merges and quarters the contention (Q3 with Zipf(1.1)
    // keys, 1.35 M rows -> 175 k groups: kernel 0.456 -> 0.264 ms). On inputs far bigger than the merge (50 M rows ->
    // 1 M groups, tools/highcard_timing.py) the rows that miss the LDS table dominate and more workgroups hide their
    // latency better (4.7 vs 5.3 ms), so the default shape stays.
    const bool merge_heavy = plan.last_groups > 4096 && N > 2 * (int64_t)256 * ctx->num_cus * 8 && N <= (int64_t)1 << 22;
    // ... and since round 3 that one workgroup per CU has 1024 threads (qk_filter_agg_wide) and a table of up to 128 KB: PMC
    // on configs[4]'s slice showed the four wavefronts per CU of the 256-thread shape waiting 77 % of their time (1.6 M HBM
    // atomics and 0.4 GB of random reads in 0.35 ms: neither a throughput limit) — a latency chain per row with too few rows in
    // flight; more 256-thread workgroups hide it but multiply the end-of-kernel merges (1 / 2 / 4 / 8 per CU: 352 / 399 / 557 /
    // 683 us), sixteen wavefronts on ONE table do not
    r.wide = merge_heavy && tune.wide;
    const int lds_budget = tune.lds_bytes.or_default(r.wide ? 128 * 1024 : merge_heavy ? 64 * 1024 : 32 * 1024);
    r.l_nslots = 16;
    while ((uint64_t)r.l_nslots * 2 * slot_bytes <= (uint64_t)lds_budget) r.l_nslots *= 2;
    if ((uint64_t)r.l_nslots * slot_bytes > (r.wide ? 128 : 64) * 1024) r.l_nslots = 0;   // slot too wide for LDS staging
    if (r.l_nslots == 0) r.wide = false;
  }
  if (c.parts) {   // one 1 024-thread workgroup per part on the biggest LDS table that fits
    r.l_nslots = 16;
    while ((uint64_t)r.l_nslots * 2 * slot_bytes <= 128 * 1024) r.l_nslots *= 2;
    r.wide = true;
  }
  ctx->agg_slot_words[c.hint_key] = plan.slot_words;
  r.block = r.wide ? 1024 : 256;
  // the consecutive-rows form (a lane owns RC adjacent rows: one wide load per column; plan.RC > 0 = every referenced column is
  // plain and narrow): a table of at least a few tiles per workgroup, the 256-thread shape, a row count known on the host
  r.cons = plan.RC > 0 && !c.parts && !r.wide && !c.in->rows_dev && N >= (int64_t)256 * plan.RC * 64 && tune.cons;
  const int64_t tile_rows = (int64_t)r.block * (r.cons ? plan.RC : plan.R);
  const int64_t ntiles = (N + tile_rows - 1) / tile_rows;
  const bool merge_heavy_grid = plan.W > 0 && plan.last_groups > 4096 && N > 2 * (int64_t)256 * ctx->num_cus * 8 && N <= (int64_t)1 << 22;
  const int bpc = tune.blocks_per_cu.or_default(N <= 2 * (int64_t)256 * ctx->num_cus * 8 ? 8 : merge_heavy_grid ? 1 : 4);
  r.grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)ctx->num_cus * bpc));
  if (c.parts) r.grid = (unsigned)c.parts->n_parts;

  // First attempt: a SMALL table (4096 slots) replicated 32 times, workgroup b merging into replica b % 32. Clearing and
  // compacting cost time proportional to the table size, and with few groups (Q1: 4) the ~1000 workgroups would
  // otherwise all merge into the same handful of slots at the end of the kernel (measured: ~45 us of a 470 us kernel).
  // The host merges the replicas (<= 32 x G slots). More groups than the small table holds -> the kernel bails out
  // early on the overflow flag -> one un-replicated table sized for the row count, x16 until it fits.
  const uint32_t cap_max = r.cap_max = plan.W == 0 ? 1 : std::max<uint32_t>(1024, pow2_ceil32((uint64_t)std::max<int64_t>(N, 1) * 2));
  r.cap = plan.W == 0 ? 1 : std::min<uint32_t>(cap_max, (uint32_t)tune.initial_slots);
  r.replicas = plan.W == 0 ? 1 : (uint32_t)tune.replicas;
  if (plan.W > 0 && tune.partition_mode == 2) {   // tests: the partitioned path on every grouped aggregate
    r.replicas = 1;
    r.cap = std::min<uint32_t>(cap_max, std::max<uint32_t>(r.cap, 4096));
  }
  if (c.parts) {   // the HBM table only takes what an LDS table cannot hold (a part with more groups than planned)
    r.replicas = 1;
    r.cap = std::min<uint32_t>(cap_max, std::max<uint32_t>(1u << 16, pow2_ceil32((uint64_t)plan.last_groups / 2 + 1)));   // (+ the sliced parts' groups; grown x16 on overflow like any table)
  } else if (plan.W > 0 && plan.last_groups > r.cap / 4) {
    // the same plan produced many groups last time: go straight to one table with room for them
    r.cap = std::min<uint32_t>(cap_max, std::max<uint32_t>(1u << 16, pow2_ceil32((uint64_t)plan.last_groups * 2)));
    r.replicas = 1;
  } else if (plan.W > 0 && plan.last_groups > 0 && plan.last_groups * 16 < r.cap) {
    // ... or very few (Q1: 4): 16 slots per expected group are plenty, and clearing + compacting the replicated table
    // (both proportional to its size, both on the critical path of the call) shrink with it
    r.cap = std::min<uint32_t>(r.cap, std::max<uint32_t>(64, pow2_ceil32((uint64_t)plan.last_groups * 16)));
  }
}

// ---------------------------------------------------------------- device-side assembly
// enqueue: allocate the output columns for up to `cap_rows` groups and launch; the number of groups is either known
// (g_dev == nullptr) or read by the kernel from the compaction counter (speculative launch right behind the compaction,
// so that a repeated many-group query needs ONE synchronisation). finish: after the stream has been synchronised.
// fin_dev: zeroed device words [status | null count per column] the caller provides and reads back itself (the speculative
// launch: they sit in the call's own status block and travel in its ONE read-back, fin_host = where they land); nullptr:
// a block of their own, read back here
static void enqueue_device_finalize(const AggCall& c, DevFinal& F, const uint64_t* dense, uint32_t cap_rows, const uint32_t* g_dev, uint32_t* fin_dev,
                                    const uint32_t* fin_host) {
  Ctx* ctx = c.ctx;
  const AggPlan& plan = c.plan();
  const int ncols = c.ncols();
  F.fc = describe_fin_cols(plan, c.n_groups, c.n_aggs);
  F.out.reset(new qhip_table());
  F.out->ctx = ctx;
  F.out->names = c.names;
  F.out->nullable = c.nullable;
  const size_t vwords = ((size_t)cap_rows + 63) / 64 + 1;
  for (int k = 0; k < ncols; ++k) {
    FinCol& f = F.fc[(size_t)k];
    DevColumn col;
    col.type = k < c.n_groups ? plan.keys[(size_t)k].type : plan.aggs[(size_t)(k - c.n_groups)].ret;
    if (f.kind == F_KEY_UTF8_LEN) F.has_utf8 = true;
    col.values = std::make_shared<DevBuf>(f.kind == F_KEY_UTF8_LEN ? ((size_t)cap_rows + 1) * 4 : (size_t)cap_rows * f.width);
    auto vb = std::make_shared<DevBuf>(vwords * 8);
    f.out_values = col.values->ptr;
    f.out_valid = vb->as<uint64_t>();
    F.valid_bufs.push_back(vb);
    F.out->cols.push_back(std::move(col));
  }
  // the column descriptors travel as a kernel argument (up to kFinColsByValue of them: no upload), else through a buffer
  const FinCol* fc_dev = nullptr;
  if (ncols > kFinColsByValue) {
    F.fc_dev.alloc(F.fc.size() * sizeof(FinCol));
    QHIP_HIP_CHECK(hipMemcpyAsync(F.fc_dev.ptr, F.fc.data(), F.fc.size() * sizeof(FinCol), hipMemcpyHostToDevice, ctx->stream));
    fc_dev = (const FinCol*)F.fc_dev.ptr;
  }
  // [status words | null count per column], zeroed, from the context's ring; read back together
  if (ncols > 240) fail(QHIP_UNSUPPORTED, "more than 240 output columns in an aggregate assembled on the device");
  const bool own = fin_dev == nullptr;
  if (own) fin_dev = zeroed_block(ctx, (QS_WORDS + ncols + 31) / 32);
  launch_agg_finalize(dense, cap_rows, g_dev, plan.slot_words, plan.null_mask_word ? 1 : 0, F.fc.data(), fc_dev, ncols,
                      fin_dev + QS_WORDS, fin_dev, ctx->stream);
  F.fin_host = own ? c.fin_pinned : fin_host;
  if (own) QHIP_HIP_CHECK(hipMemcpyAsync(c.fin_pinned, fin_dev, (size_t)(QS_WORDS + ncols) * 4, hipMemcpyDeviceToHost, ctx->stream));
}

// (call after the stream has been synchronised at least up to the read-backs above)
static qhip_table* finish_device_finalize(const AggCall& c, DevFinal& F, const uint64_t* dense, uint32_t groups, bool synced) {
  Ctx* ctx = c.ctx;
  const int ncols = c.ncols();
  if (!synced) QHIP_HIP_CHECK(sync_stream(ctx->stream));   // (the speculative launch sat in front of the call's one wait)
  if (F.fin_host[QS_ARITH_OVERFLOW]) fail(QHIP_EXEC_ERROR, "AVG(Decimal128): scaled sum overflows the result type (reference yields a mistyped NULL, avg.rs:105-116)");
  F.out->num_rows = groups;
  F.out->batch_offsets = {0, (int64_t)groups};
  for (int k = 0; k < ncols; ++k) {
    DevColumn& col = F.out->cols[(size_t)k];
    col.length = groups;
    col.null_count = F.fin_host[QS_WORDS + k];
    if (col.null_count > 0) col.validity = F.valid_bufs[(size_t)k];
    if (F.fc[(size_t)k].kind == F_KEY_UTF8_LEN) {
      // lengths -> offsets (exclusive scan) -> bytes
      uint32_t* off = col.values->as<uint32_t>();
      DevBuf total(4);
      exclusive_scan_u32(off, off, groups, total.as<uint32_t>(), ctx->stream);
      uint32_t nbytes = 0;
      copy_sync(ctx->stream, &nbytes, total.ptr, 4, hipMemcpyDeviceToHost);
      QHIP_HIP_CHECK(hipMemcpyAsync(off + groups, total.ptr, 4, hipMemcpyDeviceToDevice, ctx->stream));
      col.data = std::make_shared<DevBuf>((size_t)nbytes);
      col.data_bytes = nbytes;
      launch_agg_utf8_key_bytes(dense, groups, c.plan().slot_words, F.fc[(size_t)k].src_word, off, col.data->as<uint8_t>(), ctx->stream);
    }
  }
  if (F.has_utf8) QHIP_HIP_CHECK(sync_stream(ctx->stream));   // the dense slots are released on return
  return F.out.release();
}

// A plan that produced many groups last time will most likely do so again: its output columns are assembled on the device right
// behind the kernel that fills the dense slots (k_agg_finalize reads the group count from the counter) — one synchronisation in
// all, and no slot crosses PCIe. Not with Utf8 keys: their bytes need the group count on the host.
static bool wants_speculative_finalize(const AggCall& c) {
  bool utf8_key = false;
  for (auto& kd : c.plan().keys) utf8_key = utf8_key || kd.type.id == QHIP_UTF8;
  return c.plan().last_groups >= c.tune.dev_threshold && !utf8_key && c.tune.speculative_finalize;
}

// ---------------------------------------------------------------- stage 6: sorted runs
// An input whose equal keys are adjacent (qh_agg_runs_body): no table, no compaction — the kernel writes the dense slots.
// Tried when the plan produced many SHORT runs' worth of groups last time (>= 4096 groups, on average <= 16 rows each) and no
// execution has found its input unsorted; the kernel verifies the order and the host falls through to the hashed path when
// it does not hold. QHIP_AGG_RUNS: 0 never, 1 (default) by that rule, 2 whenever the plan has the entry point (tests).
// Leaves r.kernel == AGG_RUNS when the dense slots are there; returns a table only for an input that turned out to be empty.
static qhip_table* try_runs(const AggCall& c, AggRun& r) {
  Ctx* ctx = c.ctx;
  const AggPlan& plan = c.plan();
  const int64_t N = c.N;
  const bool eligible = plan.has_runs && !c.parts && plan.W > 0 && N > 0 && N < ((int64_t)1 << 31) && (uint64_t)N * c.slot_bytes <= (256ull << 20) && !plan.not_sorted;
  const bool worth = plan.last_groups >= 4096 && (uint64_t)plan.last_groups * 16 >= (uint64_t)N;
  if (!(eligible && (c.tune.runs_mode == 2 || (c.tune.runs_mode == 1 && worth)))) return nullptr;
  r.guess = (uint32_t)N;                          // one slot per row at worst: nothing can be lost
  r.dense.alloc((size_t)r.guess * c.slot_bytes + 8);
  r.dense_dev = r.dense.as<uint64_t>();
  const int ncols = c.ncols();
  uint32_t* status_dev = zeroed_block(ctx, (32 + QS_WORDS + ncols + 31) / 32);
  uint32_t* const counter_dev = status_dev + 16;
  HRunsLaunch rl;
  rl.dense_out = r.dense_dev + 1; rl.counter = counter_dev; rl.status = status_dev; rl.flags = status_dev + 20;
  rl.cap = r.guess; rl.max_run = c.tune.runs_max;
  // dynamic LDS: the evaluated rows of a workgroup's four wavefronts + their look-ahead (4 x 320 Row structs; a Row is at
  // most 8 + 8 W + 24 bytes per argument — the kernel sizes the look-ahead from what it gets and gives up below 264 rows)
  const size_t row_bound = 8 + 8 * (size_t)plan.W + 24 * plan.args.size();
  const int lds_kb = c.tune.runs_lds_kb.or_default((int)std::min<size_t>(160, std::max<size_t>(32, (4 * 320 * row_bound + 16383) / 16384 * 16)));
  rl.lds_bytes = (uint32_t)std::max(16, std::min(160, lds_kb)) * 1024u;
  void* rargs[] = {c.kargs(), &rl};
  std::shared_ptr<Module> rmod = get_module(ctx, plan.source, "qk_agg_runs");
  const unsigned rgrid = (unsigned)((N + 1023) / 1024);
  time_mark(ctx, 0);
  QHIP_HIP_CHECK(hipModuleLaunchKernel(rmod->fn, rgrid, 1, 1, 256, 1, 1, rl.lds_bytes, ctx->stream, rargs, nullptr));
  time_mark(ctx, 1);
  if (wants_speculative_finalize(c)) {
    r.spec = DevFinal();
    enqueue_device_finalize(c, r.spec, r.dense_dev + 1, r.guess, counter_dev, status_dev + 32, c.status_pinned + 32);
    r.spec_enqueued = true;
  }
  // ONE read-back: status + counter + the order flags (word 20) + the finalisation's status and null counts
  QHIP_HIP_CHECK(hipMemcpyAsync(c.status_pinned, status_dev, (size_t)(32 + QS_WORDS + ncols) * 4, hipMemcpyDeviceToHost, ctx->stream));
  QHIP_HIP_CHECK(sync_stream(ctx->stream));
  memcpy(r.status, c.status_pinned, sizeof(r.status));
  verify_pending_sizes(ctx);
  if (c.in->rows_dev && c.in->deferred_count() == 0 && c.n_groups > 0) return no_batches_out(c);
  if (ctx->timing) QHIP_HIP_CHECK(hipEventElapsedTime(&r.main_ms, ctx->ev[0], ctx->ev[1]));
  if (c.status_pinned[20] == 0) {
    check_status_words(r.status);
    r.kernel = AGG_RUNS;
    r.replicas = 1;
    r.cap = r.guess;
    r.grid = rgrid;
    r.l_nslots = 0;
  } else {
    // not that kind of input (or a few long runs): remember, and aggregate it through the table
    if (c.tune.runs_debug) fprintf(stderr, "[qhip agg runs] rows %lld: flags %u (1 = order, 2 = run too long), runs counted %u\n", (long long)N, c.status_pinned[20], c.status_pinned[16]);
    plan.not_sorted = true;
    r.spec = DevFinal();
    r.spec_enqueued = false;
    r.dense = DevBuf();
    r.dense_dev = nullptr;
    ++r.retries;
  }
  return nullptr;
}

// ---------------------------------------------------------------- stage 7a: the three-pass partitioned aggregate
// the reduce pass over `rl`'s work items: 1 024-thread workgroups with `wgs_per_cu` of them per CU, or 256-thread ones with twice as many
static void launch_reduce(const AggCall& c, const std::shared_ptr<Module>& m_red, HReduceLaunch& rl, HAggLaunch& Lp, bool wide, unsigned wgs_per_cu) {
  Ctx* ctx = c.ctx;
  void* rargs[] = {&rl, &Lp};
  const unsigned lds = (unsigned)((size_t)Lp.l_nslots * c.slot_bytes);
  if (wide) {
    std::shared_ptr<Module> m_wide = get_module(ctx, c.plan().source, "qk_agg_reduce_wide");
    QHIP_HIP_CHECK(hipModuleLaunchKernel(m_wide->fn, std::min<unsigned>(rl.n_items, (unsigned)ctx->num_cus * wgs_per_cu), 1, 1, 1024, 1, 1, lds, ctx->stream, rargs, nullptr));
  } else {
    QHIP_HIP_CHECK(hipModuleLaunchKernel(m_red->fn, std::min<unsigned>(rl.n_items, (unsigned)ctx->num_cus * wgs_per_cu * 2), 1, 1, 256, 1, 1, lds, ctx->stream, rargs, nullptr));
  }
}

// Many groups on a big input: partition the rows by key hash first, so that every bin's groups fit an LDS table and the
// HBM table is touched once per GROUP instead of once per row (device/qhip_device.hpp, "partitioned aggregation"):
// histogram, scan, staged or plain scatter of the rows' records into bins, and the reduce pass over work items — bins or slices
// of them — that the host computes from the scanned histogram (one extra wait) or, `device_items`, the reduce kernel itself.
// `records` (as big as the input's key + argument columns) and `item_first` belong to the caller: they live until the attempt's
// next synchronisation. Returns false, with nothing launched, when HBM cannot hold the records: the fused kernel runs then.
static bool launch_partitioned(const AggCall& c, const AggRun& r, const HAggLaunch& L, bool device_items, DevBuf& records,
                               std::vector<uint32_t>& item_first) {
  Ctx* ctx = c.ctx;
  const AggPlan& plan = c.plan();
  const AggTuning& tune = c.tune;
  const int64_t N = c.N;
  const int slot_bytes = c.slot_bytes;
  try {
    records.alloc((size_t)N * (slot_bytes - 8) + 8);
  } catch (const Error& e) {
    if (e.code != QHIP_OUT_OF_MEMORY) throw;
    return false;
  }
  hipStream_t s = ctx->stream;
  // (QHIP_AGG_PART_LDS_BYTES: bigger LDS tables in the reduce pass = fewer bins = longer runs per tile in pass 2 — measured:
  // pass 2 gains less than the reduce pass loses with one or two workgroups per CU: 50 M rows -> 1 M groups 1.86 -> 2.23 ms
  // at 64 KB, 2.98 ms at 128 KB; off by default)
  uint32_t l_nslots_p = r.l_nslots;
  // the reduce pass as 1 024-thread workgroups with 128 KB LDS tables (one per CU, 16 wavefronts): four times the groups
  // per bin = a quarter of the bins = 4x longer runs per tile in pass 2, and the reduce pass itself keeps its occupancy
  // (with 256-thread workgroups bigger tables lost more than pass 2 gained). 50 M rows -> 1 M groups 1.87 -> 1.56 ms,
  // Zipf(1.1) keys 1.69 -> 1.50 ms (QHIP_AGG_PART_WIDE=0: the 256-thread reduce pass)
  const bool wide = tune.part_wide && !tune.lds_bytes.set && plan.part_pr > 0 && (uint64_t)slot_bytes * 64 <= 128 * 1024;
  if (!tune.lds_bytes.set)
    while ((uint64_t)l_nslots_p * 2 * slot_bytes <= (uint64_t)tune.part_lds_bytes.or_default(wide ? 128 * 1024 : 0)) l_nslots_p *= 2;
  const uint32_t per_bin = std::max<uint32_t>(16, l_nslots_p * (l_nslots_p > r.l_nslots ? 5 : 3) / 8);   // groups a bin should hold
  uint32_t n_bins = 16;
  while (n_bins < 4096 && (uint64_t)n_bins * per_bin < std::max<uint32_t>(plan.last_groups, 1)) n_bins *= 2;
  if (tune.part_bins >= 16) n_bins = (uint32_t)pow2_ceil32((uint64_t)std::min(4096, tune.part_bins));
  uint64_t g1 = std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)N + 255) / 256, (uint64_t)ctx->num_cus * (uint64_t)tune.part_wgs_per_cu));
  const uint64_t rows_per_wg = ((((uint64_t)N + g1 - 1) / g1) + 255) / 256 * 256;
  g1 = ((uint64_t)N + rows_per_wg - 1) / rows_per_wg;
  const uint64_t n_hist = (uint64_t)n_bins * g1;
  DevBuf hist((n_hist + 1) * 4), items_dev;   // (both go back to the stream-ordered pool on return)
  std::shared_ptr<Module> m_hist = get_module(ctx, plan.source, "qk_agg_part_hist");
  std::shared_ptr<Module> m_scat = get_module(ctx, plan.source, "qk_agg_part_scatter");
  std::shared_ptr<Module> m_red = get_module(ctx, plan.source, "qk_agg_reduce");
  HPartLaunch pl;
  pl.hist = hist.as<uint32_t>();
  pl.records = records.as<uint64_t>();
  pl.status = L.status;
  pl.n_bins = n_bins;
  pl.rows_per_wg = (uint32_t)rows_per_wg;
  void* pargs[] = {c.kargs(), &pl};
  QHIP_HIP_CHECK(hipModuleLaunchKernel(m_hist->fn, (unsigned)g1, 1, 1, 256, 1, 1, n_bins * 4, s, pargs, nullptr));
  exclusive_scan_u32(hist.as<uint32_t>(), hist.as<uint32_t>(), n_hist, hist.as<uint32_t>() + n_hist, s);
  // pass 2: LDS-staged (records of a tile ordered by bin, written out as runs) when a tile of records fits LDS
  if (plan.part_pr > 0 && tune.part_stage) {
    std::shared_ptr<Module> m_stage = get_module(ctx, plan.source, "qk_agg_part_stage");
    const size_t tile = (size_t)1024 * (size_t)plan.part_pr;
    const size_t stage_lds = (size_t)n_bins * 12 + 8 + tile * ((size_t)(plan.slot_words - 1) * 8 + 2) + 16;
    QHIP_HIP_CHECK(hipModuleLaunchKernel(m_stage->fn, (unsigned)g1, 1, 1, 1024, 1, 1, (unsigned)stage_lds, s, pargs, nullptr));
  } else
    QHIP_HIP_CHECK(hipModuleLaunchKernel(m_scat->fn, (unsigned)g1, 1, 1, 256, 1, 1, n_bins * 4, s, pargs, nullptr));
  HReduceLaunch rl;
  rl.records = records.as<uint64_t>();
  HAggLaunch Lp = L;
  Lp.l_nslots = l_nslots_p;
  if (device_items) {
    // the bins' slices as work items, computed by the reduce kernel itself from the scanned histogram: a bin of `cnt`
    // records is cut into `slices` slices of at least 4 096 records (a heavy key's bin is aggregated by several
    // workgroups, each merging its LDS table into the HBM table); empty slices return at once
    rl.item_first = nullptr;
    rl.slices = tune.part_slices;
    rl.n_items = n_bins * rl.slices;
    rl.hist = hist.as<uint32_t>();
    rl.g1 = (uint32_t)g1; rl.n_bins = n_bins; rl.min_slice = 4096;
    launch_reduce(c, m_red, rl, Lp, wide, 8);
    // (hist / records go back to the stream-ordered pool: no wait; the call's one synchronisation follows in the caller)
    return true;
  }
  // first record of every bin (= of its first workgroup's run) + the record total: one strided read-back
  uint32_t* first = (uint32_t*)((uint8_t*)ctx->pinned + 128);
  QHIP_HIP_CHECK(hipMemcpy2DAsync(first, 4, hist.ptr, (size_t)g1 * 4, 4, n_bins, hipMemcpyDeviceToHost, s));
  QHIP_HIP_CHECK(hipMemcpyAsync(first + n_bins, hist.as<uint32_t>() + n_hist, 4, hipMemcpyDeviceToHost, s));
  QHIP_HIP_CHECK(sync_stream(s));
  verify_pending_sizes(ctx);   // (an input of deferred size: did the joins below have room? — else QHIP_RETRY)
  // work items: a bin, or a slice of a big one (a heavy key's bin is aggregated by several workgroups, each merging
  // its LDS table into the HBM table: the key is merged once per slice, not once per row)
  // (work items of 128 k records for the wide reduce pass: 256 k is better for uniform keys, 64 k for skewed ones)
  const uint32_t max_item = (uint32_t)std::max(4096, tune.partition_item.or_default(wide ? 131072 : 32768));
  for (uint32_t b = 0; b < n_bins; ++b)
    for (uint32_t rec = first[b]; rec < first[b + 1]; rec += max_item) item_first.push_back(rec);
  const uint32_t n_items = (uint32_t)item_first.size();
  item_first.push_back(first[n_bins]);
  if (n_items) {
    items_dev.alloc(item_first.size() * 4);
    QHIP_HIP_CHECK(hipMemcpyAsync(items_dev.ptr, item_first.data(), item_first.size() * 4, hipMemcpyHostToDevice, s));
    rl.item_first = items_dev.as<uint32_t>();
    rl.n_items = n_items;
    launch_reduce(c, m_red, rl, Lp, wide, 2);
    QHIP_HIP_CHECK(sync_stream(s));   // hist / items go back to the pool here; item_first is pageable
  }
  return true;
}

// ---------------------------------------------------------------- stage 7b: what follows an attempt's kernel on the stream
// Speculative compaction right behind the kernel: [counter | dense slots]; the common case (few groups, no overflow) then
// needs a single synchronisation for status + result. arena: the persistent arena the table sits in (else null).
static void enqueue_collect(const AggCall& c, AggRun& r, uint32_t* status_dev, DevBuf* arena, size_t zero_bytes) {
  Ctx* ctx = c.ctx;
  const AggPlan& plan = c.plan();
  const int slot_bytes = c.slot_bytes;
  const uint32_t total_slots = r.cap * r.replicas;
  uint32_t* const counter_dev = status_dev + 16;   // (page-locked mirror: status_pinned = pinned + 0, pre_host[0] = pinned + 64)
  r.pre_copied = 0;
  if (plan.W == 0) {
    QHIP_HIP_CHECK(hipMemcpyAsync(c.status_pinned, status_dev, sizeof(r.status), hipMemcpyDeviceToHost, ctx->stream));
    QHIP_HIP_CHECK(hipMemcpyAsync(c.pre_host, r.table_dev, (size_t)slot_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return;
  }
  if (arena) {
    // counter at +64 (zeroed with the arena), dense slots behind the table; the 8 bytes in front of the slots are a
    // copy target only in the read-back below, so read counter and slots separately
    r.dense_dev = (uint64_t*)(arena->as<uint8_t>() + zero_bytes);
    // the first pre_copied dense slots land in page-locked host memory straight from the compaction kernel (no
    // device-to-host copy of the slots behind it: that copy goes through the DMA engine, ~25 us with its hand-over gaps)
    r.pre_copied = std::min(c.PRE, r.guess);
    const bool direct = c.tune.pinned_slots;
    launch_compact_slots(r.table_dev, total_slots, plan.slot_words, r.dense_dev + 1, counter_dev, r.guess, ctx->stream, direct ? c.pre_host + 1 : nullptr, r.pre_copied);
    QHIP_HIP_CHECK(hipMemcpyAsync(c.status_pinned, status_dev, 64 + 8, hipMemcpyDeviceToHost, ctx->stream));   // status + counter
    if (!direct) QHIP_HIP_CHECK(hipMemcpyAsync(c.pre_host + 1, r.dense_dev + 1, (size_t)r.pre_copied * slot_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return;
  }
  if (!c.parts) { r.dense.alloc((size_t)r.guess * slot_bytes + 8); r.dense_dev = r.dense.as<uint64_t>(); }   // (parts: allocated in front of the kernel, which appends to it)
  r.spec_enqueued = false;
  const bool will_spec = r.replicas == 1 && wants_speculative_finalize(c);
  // (a host-side result: its first dense slots go to page-locked host memory straight from the compaction kernel)
  // (parts: the workgroups appended most slots themselves — the first ones are copied out of the dense buffer instead)
  const bool direct = !will_spec && !c.parts && c.tune.pinned_slots;
  launch_compact_slots(r.table_dev, total_slots, plan.slot_words, r.dense_dev + 1, counter_dev, r.guess, ctx->stream, direct ? c.pre_host + 1 : nullptr,
                       std::min(c.PRE, r.guess));
  if (will_spec) {
    r.spec = DevFinal();
    enqueue_device_finalize(c, r.spec, r.dense_dev + 1, r.guess, counter_dev, status_dev + 32, c.status_pinned + 32);
    r.spec_enqueued = true;
    // ONE read-back: status + counter + the finalisation's status and null counts
    QHIP_HIP_CHECK(hipMemcpyAsync(c.status_pinned, status_dev, (size_t)(32 + QS_WORDS + c.ncols()) * 4, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    QHIP_HIP_CHECK(hipMemcpyAsync(c.status_pinned, status_dev, 64 + 8, hipMemcpyDeviceToHost, ctx->stream));   // status + counter
    r.pre_copied = std::min(c.PRE, r.guess);
    if (!direct) QHIP_HIP_CHECK(hipMemcpyAsync(c.pre_host + 1, r.dense_dev + 1, (size_t)r.pre_copied * slot_bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
}

// ---------------------------------------------------------------- stage 7: the table attempts
// One attempt = clear the table, run the kernel family the shape asks for, compact, read back, wait once. An overflowing table is
// tried again un-replicated and 16 times as big. Returns a table only for an input that turned out to be empty.
static qhip_table* run_table_attempts(const AggCall& c, AggRun& r) {
  Ctx* ctx = c.ctx;
  const AggPlan& plan = c.plan();
  const AggTuning& tune = c.tune;
  const AggParts* parts = c.parts;
  const int64_t N = c.N;
  const int slot_bytes = c.slot_bytes;
  const size_t lds_bytes = (size_t)r.l_nslots * slot_bytes;
  for (;;) {
    const size_t table_bytes = (size_t)r.cap * r.replicas * slot_bytes;
    const uint32_t total_slots = r.cap * r.replicas;
    // (a plan that produced many groups last time gets a dense buffer that should hold them all at once)
    r.guess = plan.W == 0 ? 0 : std::min<uint32_t>(total_slots, std::max<uint32_t>(8192, plan.last_groups + plan.last_groups / 4));
    if (parts) r.guess = (uint32_t)std::max<int64_t>(N, 1);   // (the workgroups append their groups themselves: room for one group per row, nothing can be lost)
    // Small replicated attempt: a persistent arena [status | counter | table | dense slots] that the PREVIOUS call left
    // zeroed, so the kernel launch is the first thing on the stream. (total_slots <= guess there: one compaction always
    // suffices and the table is not needed again after it.)
    const bool use_arena = !parts && plan.W > 0 && r.replicas > 1 && total_slots <= 8192 && table_bytes <= (1u << 20) && tune.arena;
    // [status words (64 bytes) | compaction counter]: in the arena, else a zeroed block of the context's ring; read back together
    uint32_t* status_dev = nullptr;
    std::shared_ptr<DevBuf> arena;
    const size_t zero_bytes = 128 + table_bytes;   // status (64) + counter (64) + table
    if (use_arena) {
      const size_t need = zero_bytes + (size_t)r.guess * slot_bytes + 64;
      arena = std::static_pointer_cast<DevBuf>(plan.arena);
      if (!arena || plan.arena_bytes != need) {
        arena = std::make_shared<DevBuf>(need);
        plan.arena = arena;
        plan.arena_bytes = need;
        plan.arena_clean = false;
      }
      if (!plan.arena_clean) QHIP_HIP_CHECK(hipMemsetAsync(arena->ptr, 0, zero_bytes, ctx->stream));
      plan.arena_clean = false;
      status_dev = arena->as<uint32_t>();
      r.table_dev = (uint64_t*)(arena->as<uint8_t>() + 128);
    } else {
      r.gtable.alloc(table_bytes);
      QHIP_HIP_CHECK(hipMemsetAsync(r.gtable.ptr, 0, table_bytes, ctx->stream));
      // [status words (16) | counter (2) | .. | words 32..: the speculative finalisation's status (8) + null counts]
      status_dev = zeroed_block(ctx, (32 + QS_WORDS + c.ncols() + 31) / 32);
      r.table_dev = r.gtable.as<uint64_t>();
    }
    HAggLaunch L;
    L.gtable = r.table_dev;
    L.g_nslots = r.cap;
    L.l_nslots = r.l_nslots;
    L.status = status_dev;
    L.replicas = r.replicas;
    L.collect_stats = tune.collect_stats ? 1u : 0u;
    void* args[] = {c.kargs(), &L};
    if (!parts) time_mark(ctx, 0);   // (parts: the clock started in front of the partition passes)
    // The three-pass partitioned aggregate. QHIP_AGG_PARTITION: 0 never, 1 when the plan's previous run says it pays (default), 2
    // always (tests). (an instrumented run, QHIP_AGG_STATS, measures the fused kernel's LDS table and keeps to it)
    // Mid-sized inputs (2^18 .. 2^22 rows with >= 16 k groups — BASELINE configs[4]'s per-rank aggregate: 2 M joined rows ->
    // 200 k groups, LDS tables 100 % full, 0.27-0.35 ms in the fused kernel) CAN take the same three passes without a host
    // round trip in between (QHIP_AGG_PARTITION_MID=1: the reduce pass derives its work items — bin slices — from the scanned
    // histogram on the device). Measured on that aggregate (round 3, rocprofv3): histogram 71 us + staged pass 168 us + reduce
    // pass 317 us = 0.57 ms against the fused kernel's 0.35 ms — the input is read through the joins' index vectors (twice
    // here) and Zipf's heavy keys serialise the LDS atomics of their bins, which the fused kernel's wave-resident hot keys
    // avoid. Off by default; what this size needs is a combiner in front of the partitioning, not fewer host waits.
    const int pa_mode = tune.partition_mode;
    const bool mid = N < ((int64_t)1 << 22);
    const bool mid_on = tune.partition_mid;
    const bool partitioned = !parts && plan.W > 0 && N > 0 && r.replicas == 1 && r.l_nslots >= 64 && !use_arena && !L.collect_stats &&
                             (pa_mode == 2 || (pa_mode == 1 && N >= ((int64_t)1 << 22) && plan.last_groups >= 32768) ||
                              (pa_mode == 1 && mid && N >= ((int64_t)1 << 18) && plan.last_groups >= 16384 && mid_on));
    const bool device_items = partitioned && mid && (mid_on || pa_mode == 2);
    std::vector<uint32_t> item_first;   // (kept alive until the call's next synchronisation)
    DevBuf pa_records;                  // (back to the stream-ordered pool at the end of the attempt)
    if (partitioned && launch_partitioned(c, r, L, device_items, pa_records, item_first)) {
      r.kernel = AGG_PARTITIONED;
    } else if (N > 0 && parts) {
      r.dense.alloc((size_t)r.guess * slot_bytes + 8);
      r.dense_dev = r.dense.as<uint64_t>();
      L.part_runs = parts->runs; L.part_stride = parts->stride;
      L.dense_out = r.dense_dev + 1; L.dense_counter = status_dev + 16; L.dense_cap = r.guess;
      // a part of more than 4x the average is sliced (heavy keys): at most n_parts / 4 + 1 slices in all
      L.n_parts = (uint32_t)parts->n_parts;
      L.part_max = (uint32_t)std::max<int64_t>(1024, tune.parts_max_factor * ((N + parts->n_parts - 1) / parts->n_parts));
      const unsigned pgrid = r.grid + (unsigned)((uint64_t)N / L.part_max) + 1;
      std::shared_ptr<Module> pmod = get_module(ctx, plan.source, "qk_filter_agg_parts");
      QHIP_HIP_CHECK(hipModuleLaunchKernel(pmod->fn, pgrid, 1, 1, 1024, 1, 1, (unsigned)lds_bytes, ctx->stream, args, nullptr));
    } else if (N > 0) {
      if (r.wide) {
        std::shared_ptr<Module> wmod = get_module(ctx, plan.source, "qk_filter_agg_wide");
        QHIP_HIP_CHECK(hipModuleLaunchKernel(wmod->fn, r.grid, 1, 1, 1024, 1, 1, (unsigned)lds_bytes, ctx->stream, args, nullptr));
      } else if (r.cons) {
        std::shared_ptr<Module> cmod = get_module(ctx, plan.source, "qk_filter_agg_cons");
        QHIP_HIP_CHECK(hipModuleLaunchKernel(cmod->fn, r.grid, 1, 1, 256, 1, 1, (unsigned)lds_bytes, ctx->stream, args, nullptr));
      } else {
        QHIP_HIP_CHECK(hipModuleLaunchKernel(c.mod->fn, r.grid, 1, 1, 256, 1, 1, (unsigned)lds_bytes, ctx->stream, args, nullptr));
      }
    }
    time_mark(ctx, 1);
    enqueue_collect(c, r, status_dev, use_arena ? arena.get() : nullptr, zero_bytes);
    if (use_arena) {
      // wait for the read-backs only; the arena is zeroed for the next call behind them
      QHIP_HIP_CHECK(hipEventRecord(ctx->ev[2], ctx->stream));
      QHIP_HIP_CHECK(hipMemsetAsync(arena->ptr, 0, zero_bytes, ctx->stream));
      plan.arena_clean = true;
      c.mark("launched");
      QHIP_HIP_CHECK(sync_event(ctx->ev[2]));
    } else {
      c.mark("launched");
      QHIP_HIP_CHECK(sync_stream(ctx->stream));
    }
    memcpy(r.status, c.status_pinned, sizeof(r.status));
    if (tune.prof) {   // phase timers of the fused kernel (P::PROF): mean cycles per wavefront, in units of 256
      const double waves = (double)r.grid * (r.block / 64);
      fprintf(stderr, "[qhip agg prof] rows %lld grid %u x %d: loads+eval %.0f  cache %.0f  table updates %.0f  cached keys -> table %.0f  merge %.0f  (x256 cycles per wavefront)\n",
              (long long)N, r.grid, r.block, c.status_pinned[8] / waves, c.status_pinned[9] / waves, c.status_pinned[10] / waves, c.status_pinned[11] / waves, c.status_pinned[12] / waves);
    }
    c.mark("synchronised");
    trace_point("aggregate: back from its wait");
    verify_pending_sizes(ctx);   // (an input of deferred size: did the joins below have room? — else QHIP_RETRY)
    // a join of deferred size that turned out to have produced nothing has no output batches (hash_join.rs:363-372)
    if (c.in->rows_dev && c.in->deferred_count() == 0 && c.n_groups > 0) return no_batches_out(c);
    if (ctx->timing) QHIP_HIP_CHECK(hipEventElapsedTime(&r.main_ms, ctx->ev[0], ctx->ev[1]));
    check_status_words(r.status);
    if (!r.status[QS_OVERFLOW]) return nullptr;
    if (r.replicas == 1 && r.cap >= r.cap_max) fail(QHIP_HIP_ERROR, "group table overflow at maximum capacity (internal error)");
    r.cap = r.replicas > 1 ? std::min<uint32_t>(r.cap_max, std::max<uint32_t>(r.cap * 16, 1u << 18)) : (uint32_t)std::min<uint64_t>((uint64_t)r.cap * 16, r.cap_max);
    r.replicas = 1;
    ++r.retries;
  }
}

// ---------------------------------------------------------------- stage 10: statistics
static void set_stats(const AggCall& c, const AggRun& r, uint32_t G) {
  qhip_exec_stats& st = c.ctx->stats;
  st.main_kernel_ms = r.main_ms;
  st.total_device_ms = r.main_ms;
  st.rows_in = c.N;
  st.rows_out = G;
  st.groups = G;
  st.table_capacity = (int64_t)r.cap * r.replicas;
  st.retries = r.retries;
  st.lds_table_slots = (int32_t)r.l_nslots;
  st.bytes_per_row_read = c.bytes_per_row;
  st.workgroups = (int32_t)r.grid;
  st.lds_spilled = r.status[QS_LDS_SPILL] != 0 ? 1 : 0;
  st.hbm_table_load = r.cap ? (double)G / ((double)r.cap * r.replicas) : 0.0;
  st.lds_occupancy = (c.tune.collect_stats && r.l_nslots) ? (double)r.status[QS_LDS_USED] / ((double)r.grid * r.l_nslots) : -1.0;
  snprintf(st.main_kernel_name, sizeof st.main_kernel_name, "%s",
           r.kernel == AGG_PARTITIONED ? "qk_agg_part_hist+scatter+reduce" : c.parts ? "qk_part_ids+qk_part_scatter+qk_filter_agg_parts" :
           r.kernel == AGG_RUNS ? "qk_agg_runs" : r.cons ? "qk_filter_agg_cons" : c.plan().kernel_name.c_str());
}

// what this execution learnt about the data: sizes the next one's table, read-back and pre-partitioning
static void remember_groups(const AggCall& c, uint32_t G) {
  c.plan().last_groups = G; c.plan().learnt_at = ++g_learn_tick;
  if (c.ctx->agg_group_hints.size() > 4096) c.ctx->agg_group_hints.clear();
  c.ctx->agg_group_hints[c.hint_key] = G;
}

// ---------------------------------------------------------------- stage 8: the dense slots
// Dense slots -> host (few groups: `slots`, replicas merged) or kept on the device (many groups: `dense_keep` = [counter | dense
// slots]). Sets G. Returns a table when the speculative device-side assembly is the result (statistics set), else nullptr.
static qhip_table* collect_slots(const AggCall& c, AggRun& r, uint32_t& G, std::vector<uint64_t>& slots, DevBuf& dense_keep) {
  Ctx* ctx = c.ctx;
  const AggPlan& plan = c.plan();
  if (plan.W == 0) {
    G = 1;
    slots.assign(c.pre_host, c.pre_host + plan.slot_words);
    return nullptr;
  }
  G = (uint32_t)c.pre_host[0];
  plan.last_dense = G;
  const uint32_t total_slots = r.cap * r.replicas;
  // (the speculative assembly holds what fitted the buffer it was enqueued with: after a re-compaction its columns are short —
  // a plan whose remembered group count came from a much smaller table, the same plan key at another scale factor)
  const bool spec_fits = G <= r.guess;
  if (G > r.guess) {
    // more groups than the speculative buffer holds: compact again with the exact size
    r.guess = G;
    r.dense.alloc((size_t)r.guess * c.slot_bytes + 8);
    r.dense_dev = r.dense.as<uint64_t>();
    launch_compact_slots(r.table_dev, total_slots, plan.slot_words, r.dense_dev + 1, zeroed_block(ctx), r.guess, ctx->stream);
    QHIP_HIP_CHECK(sync_stream(ctx->stream));
    r.pre_copied = 0;
  }
  if (r.spec_enqueued && spec_fits && r.replicas == 1 && G >= c.tune.dev_threshold) {
    // the speculative device-side assembly is the result
    remember_groups(c, G);
    qhip_table* result = finish_device_finalize(c, r.spec, r.dense_dev + 1, G, true);
    set_stats(c, r, G);
    return result;
  }
  if (r.replicas == 1 && G >= c.tune.dev_threshold) {
    dense_keep = std::move(r.dense);
  } else if (G <= r.pre_copied) {
    slots.assign(c.pre_host + 1, c.pre_host + 1 + (size_t)G * plan.slot_words);
  } else {
    slots.resize((size_t)G * plan.slot_words);
    copy_sync(ctx->stream, slots.data(), r.dense_dev + 1, (size_t)G * c.slot_bytes, hipMemcpyDeviceToHost);
  }
  if (r.replicas > 1 && G > 1) G = merge_replica_slots(plan, slots, G);
  return nullptr;
}

// ---------------------------------------------------------------- the driver
static qhip_table* hash_aggregate(Ctx* ctx, const qhip_table* in, const qhip_expr* exprs, int n_exprs, int pred_root,
                                  const int32_t* group_roots, int n_groups, const qhip_agg* aggs, int n_aggs,
                                  const char* const* out_names, const AggParts* parts, bool key_encoded) {
  AggCall c;
  c.tune = read_agg_tuning();
  c.t_begin = std::chrono::steady_clock::now();
  c.ctx = ctx; c.in = in; c.parts = parts; c.n_groups = n_groups; c.n_aggs = n_aggs;
  trace_point("aggregate: entry");
  QHIP_HIP_CHECK(hipSetDevice(ctx->device));
  validate_agg_args(exprs, n_exprs, pred_root, group_roots, n_groups, aggs, n_aggs);
  memset(&ctx->stats, 0, sizeof(ctx->stats));
  ctx->stats_timing_pending = 0;

  c.hint_key = parts ? parts->hint_key : agg_hint_key(exprs, n_exprs, pred_root, group_roots, n_groups, aggs, n_aggs);
  const int wide_mode = key_encoded || parts ? 0 : ctx->wide_keys_mode >= 0 ? ctx->wide_keys_mode : c.tune.wide_keys;
  if (wide_mode)
    if (qhip_table* t = maybe_encode_wide_key(ctx, c.tune, wide_mode, in, exprs, n_exprs, pred_root, group_roots, n_groups, aggs, n_aggs, out_names)) return t;
  if (!parts)
    if (qhip_table* t = maybe_prepartition(ctx, c.tune, c.hint_key, in, exprs, n_exprs, pred_root, group_roots, n_groups, aggs, n_aggs, out_names)) return t;

  const std::vector<InputCol> icols = resolve_agg_inputs(ctx, c.tune, in, exprs, n_exprs, group_roots, n_groups);
  try {
    c.plan_ptr = lookup_or_lower_plan(ctx, c.tune, in, icols, exprs, n_exprs, pred_root, group_roots, n_groups, aggs, n_aggs);
  } catch (const Error& e) {
    // wide keys are on, yet the key that does not fit is computed: the encoding stage takes plain key columns only
    if (wide_mode == 1 && e.code == QHIP_UNSUPPORTED && !plain_column_keys(in, exprs, group_roots, n_groups))
      fail(QHIP_UNSUPPORTED, std::string(e.what()) + " (wide group keys: computed key expressions are not encoded)");
    throw;
  }
  c.mark("planned");

  for (int k = 0; k < n_groups + n_aggs; ++k) {
    c.names.push_back(out_names && out_names[k] ? out_names[k] : ("col" + std::to_string(k)));
    c.nullable.push_back(true);
  }
  c.zero_batches_in = in->no_batches();
  if (n_groups > 0 && c.zero_batches_in) return no_batches_out(c);
  bind_plan_to_input(c, icols);

  AggRun r;
  decide_launch_shape(c, r);
  if (qhip_table* t = try_runs(c, r)) return t;
  if (r.kernel != AGG_RUNS)
    if (qhip_table* t = run_table_attempts(c, r)) return t;

  uint32_t G = 0;
  std::vector<uint64_t> slots;
  DevBuf dense_keep;
  if (qhip_table* t = collect_slots(c, r, G, slots, dense_keep)) return t;
  remember_groups(c, G);
  if (dense_keep.ptr) {
    // many groups: assemble the output columns on the device (k_agg_finalize), nothing crosses PCIe
    DevFinal fin;
    enqueue_device_finalize(c, fin, dense_keep.as<uint64_t>() + 1, G, nullptr, nullptr, nullptr);
    qhip_table* result = finish_device_finalize(c, fin, dense_keep.as<uint64_t>() + 1, G, false);
    set_stats(c, r, G);
    return result;
  }
  // few groups: assemble the output columns on the host
  std::vector<HostColumn> cols = assemble_host_columns(c.plan(), slots, G, n_groups, n_aggs, c.zero_batches_in);
  set_stats(c, r, G);
  c.mark("assembled");
  qhip_table* result = table_from_host(ctx, c.names, c.nullable, cols, G, false);
  c.mark("result table");
  return result;
}

}  // namespace qhip

using namespace qhip;

extern "C" int qhip_hash_aggregate_execute(qhip_ctx* ctx, const qhip_table* input, const qhip_expr* exprs, int32_t n_exprs,
                                           int32_t predicate_root, const int32_t* group_roots, int32_t n_groups, const qhip_agg* aggs,
                                           int32_t n_aggs, const char* const* out_names, qhip_table** out) {
  if (!ctx || !input || !out) return QHIP_INVALID_ARGUMENT;
  *out = nullptr;
  return guarded(ctx, [&] {
    try {
      std::unique_ptr<qhip_table> r(hash_aggregate(ctx, input, exprs, n_exprs, predicate_root, group_roots, n_groups, aggs, n_aggs, out_names));
      if (!ctx->pending_sizes.empty()) {   // (a path that never waited: the joins of deferred size below are checked all the same)
        QHIP_HIP_CHECK(sync_stream(ctx->stream));
        verify_pending_sizes(ctx);
      }
      *out = r.release();
      trace_point("aggregate: return");
    } catch (...) {
      ctx->pending_sizes.clear();
      throw;
    }
  });
}
