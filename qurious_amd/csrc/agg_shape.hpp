// agg_shape.hpp — the fused aggregate's tuning policy: which Decimal128 arguments travel and accumulate in 64 bits, how many
// hot keys a wavefront caches (KC), how many rows a thread evaluates per tile (R), whether the plan gets the consecutive-rows
// form (RC) and how many rows the partitioned path stages per thread (PART_PR) — all from a register budget. Plain host
// code: no HIP runtime call, no Ctx and no environment (the QHIP_AGG_* switches come in as one AggShapeTuning), so it runs (and is
// tested, tests/cpp/agg_shape_tests.cpp) without a GPU. plan_aggregate (codegen.cpp) is the only caller.
#pragma once
#include <vector>

#include "common.hpp"

namespace qhip {

enum CellKind { CELL_ROWS = 0, CELL_SUM_I128, CELL_SUM_U64, CELL_SUM_F64, CELL_CNT, CELL_MAXORD64, CELL_MAXORD128 };

struct ArgDesc {
  int root; DType type; bool nullable;
  bool value_needed;   // some cell reads the value (not only whether it is NULL): the Row carries it
  u128 maxabs;         // ENode::maxabs of the argument
  int width;           // dtype_width(type)
};
struct CellDesc {
  int kind; int arg;   // arg = index into args (-1 for CELL_ROWS)
  bool is_min;         // MAXORD cells: true stores ~ord(v) so that the running maximum is the minimum
  int off;             // word offset inside the slot's cell area
  int words;
};

// the switches of the aggregate's generated code (tuning experiments and measurements only), read once by plan_aggregate
struct AggShapeTuning {
  EnvInt kc;            // QHIP_AGG_KC: hot keys of a grouped plan
  EnvInt part_pr;       // QHIP_AGG_PART_PR: a cap (at least 1) on the staged scatter's rows per thread
  int cons = 1;         // QHIP_AGG_CONS: the consecutive-rows form 0 never, 1 when the registers allow, 2 whenever the columns allow
  int cons_r = 4;       // QHIP_AGG_CONS_R: its rows per lane (clamped to 1..8)
  int cons_sb = 4, cons_pipe = 1, prof = 0, pipe = 0, waves = 0;   // QHIP_AGG_CONS_SB, _CONS_PIPE, _PROF, _PIPE, _WAVES: constants of the source
};

struct AggShape {
  std::vector<bool> arg64, arg_acc64;   // per argument: an i64 in the Row; its SUM accumulated per lane in 64 bits
  int part_regs = 0;                    // VGPRs of one cached key's accumulators
  int row_regs = 0;                     // VGPRs of one evaluated row: pass flag, key words, argument dwords
  int KC = 0, R = 0, RC = 0, part_pr = 0;   // AggPlan's fields of the same names
  bool acc64(const CellDesc& c) const { return c.kind == CELL_SUM_I128 && arg_acc64[(size_t)c.arg]; }
};
// W key words; slot_words = 1 + W + cell words; narrow_copies: the input streams narrow copies of its Decimal128 columns;
// cons_columns: every referenced column allows the consecutive-rows form; rows_per_thread > 0 fixes R
AggShape agg_shape(int W, int slot_words, const std::vector<CellDesc>& cells, const std::vector<ArgDesc>& args, bool narrow_copies, bool dev_rows,
                   bool cons_columns, int rows_per_thread, const AggShapeTuning& t);

}  // namespace qhip
