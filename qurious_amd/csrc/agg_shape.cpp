// agg_shape.cpp — the fused aggregate's tuning policy (agg_shape.hpp): plain arithmetic over the plan's cells and arguments.
#include "agg_shape.hpp"

#include <algorithm>

namespace qhip {

AggShape agg_shape(int W, int slot_words, const std::vector<CellDesc>& cells, const std::vector<ArgDesc>& args, bool narrow_copies, bool dev_rows,
                   bool cons_columns, int rows_per_thread, const AggShapeTuning& t) {
  AggShape s;
  // Decimal128 arguments whose magnitude is known (ENode::maxabs) travel and accumulate narrower: a value below 2^63 is kept
  // as i64 in the Row; a SUM over values below 2^39 is accumulated per lane in 64 bits (a lane sees at most 2^24 of a
  // table's < 2^32 rows, so the lane sum stays below 2^63) and widened when the lanes are reduced at the end of the kernel
  for (const ArgDesc& a : args) {
    s.arg64.push_back(a.type.id == QHIP_DECIMAL128 && a.maxabs < ((u128)1 << 63));
    s.arg_acc64.push_back(a.type.id == QHIP_DECIMAL128 && a.maxabs < ((u128)1 << 39));
  }
  // hot-key cache size: lane-private accumulators for KC keys must fit the register file next to R rows
  for (auto& c : cells) if (c.kind != CELL_ROWS) s.part_regs += s.acc64(c) ? 2 : 2 * c.words - (c.kind == CELL_MAXORD128 ? 2 : 0);
  const int part_regs = s.part_regs;
  s.KC = W == 0 ? 0 : (part_regs * 4 <= 96 ? 4 : part_regs * 2 <= 96 ? 2 : 0);
  // every SUM narrow (64-bit lane accumulators): a cached key then costs its compare plus two VALU instructions per cell and
  // row, and what counts is the number of PASSES over the tile's rows. Measured on TPC-H Q1's list (5 narrow sums, 4 groups
  // of 49 / 25 / 25 / 1 % of the rows; kernel time for SF10's rows): KC 0 0.680 ms, 1 0.648, 2 0.641 (R = 3), 3 0.717,
  // 4 0.719 — two cached keys and the LDS table for the rest beat four passes; a single narrow sum (q1_mini) still wants
  // every group cached (KC 3-4 0.323 ms, KC 2 0.403).
  bool all_narrow = W > 0 && !cells.empty();
  for (auto& c : cells) if (c.kind != CELL_ROWS && !s.acc64(c)) all_narrow = false;
  if (all_narrow && part_regs > 0) s.KC = std::max(1, std::min(4, 24 / part_regs));
  // ... and when the kernel streams NARROW COPIES of its decimal columns (InputCol::narrow_bytes: 22 instead of 70 bytes per row
  // for Q1) it is no longer HBM that bounds it but the LDS: PMC on Q1 at KC = 2 — the quarter of the rows that miss the two
  // cached keys keep the CU's LDS pipeline busy 76 % of the time (same-address DS atomics: SQ_LDS_BANK_CONFLICT = 26 % of the
  // CU's cycles). Measured then, kernel + host per query: KC 2 0.522 ms, 3 0.409-0.422, 4 0.298 (R = 2; R = 1: 0.355, 3: 0.349).
  if (all_narrow && narrow_copies && part_regs > 0) s.KC = std::max(1, std::min(4, 48 / part_regs));
  if (t.kc.given && W > 0) s.KC = t.kc.value;   // tuning experiments only
  s.row_regs = 1 + 2 * W;
  for (size_t a = 0; a < args.size(); ++a) {
    if (args[a].value_needed) s.row_regs += s.arg64[a] ? 2 : std::max(1, args[a].width / 4);
    if (args[a].nullable) s.row_regs += 1;
  }
  s.R = rows_per_thread;
  if (s.R <= 0) {
    // rows per thread per tile: all loads of a tile are in flight together, so more rows = more memory-level
    // parallelism, until registers cut the occupancy. One Row costs 1 + 2 W + (argument dwords) VGPRs, the cache
    // KC x part_regs. Measured on MI355X: q1_mini (7 regs/row) best at R = 4, Q1 (25 regs/row, 80 cache regs) at R = 2.
    s.R = std::max(1, std::min(4, ((all_narrow ? 72 : 144) - s.KC * part_regs) / s.row_regs));   // (narrow Q1: R = 3, 0.641 ms; 2: 0.666; 4: 0.659)
  }
  // rows per thread of the partitioned path's staged scatter (qh_agg_part_stage_body): what a 1 024-thread workgroup can stage
  // in LDS beside 4 096 bins' counters (160 KB per CU), at most 4; 0 = records too wide, per-lane stores
  s.part_pr = std::min(4, (int)((163840 - 4096 * 12 - 1024) / (1024 * ((slot_words - 1) * 8 + 2))));
  if (t.part_pr.set) s.part_pr = std::min(s.part_pr, std::max(1, t.part_pr.value));   // (experiments)
  // The consecutive-rows form (qh_filter_agg_body<.., CONS>): for inputs whose referenced columns are all plain (no index
  // vectors, no validity bitmaps, no Booleans, strings only as one-byte flags) and at most 8 bytes wide in the layout that is
  // streamed — a lane's RC values of a column are then adjacent bytes and load as one instruction.
  // QHIP_AGG_CONS: 0 never, 1 (default) when the registers allow, 2 whenever the columns allow. Measured on MI355X, one box
  // (profiles/r04_q1_consecutive_rows.txt): q1_mini (100 M rows, 9 B per row, one narrow SUM: 84-120 VGPRs) rows r*256+tid 0.225 ms,
  // consecutive rows x 4 with two register sets 0.200 ms (0.50 -> 0.56 of the HBM peak); TPC-H Q1's list at SF10 (22 B per row,
  // five SUMs x four cached keys) 0.268 ms against 0.291-0.368 ms — a quarter of the load instructions and twice the bytes in
  // flight per wavefront do not pay for 147-235 VGPRs against 127 (three or two wavefronts per SIMD instead of four). Hence the
  // rule: the cached keys' accumulators + four evaluated rows within 64 VGPRs.
  const bool cons_fits = s.KC * part_regs + 4 * s.row_regs <= 64;
  if (!dev_rows && cons_columns && (t.cons == 2 || (t.cons == 1 && cons_fits))) s.RC = std::max(1, std::min(8, t.cons_r));
  return s;
}

}  // namespace qhip
