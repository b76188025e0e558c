// The fused aggregate's tuning policy (qurious_amd/csrc/agg_shape.cpp) without a GPU: KC, R, RC and PART_PR at the catalog's Q1
// and Q3 shapes and on both sides of every threshold of the rules. Every expected value was READ from the generated source of the
// commit before the policy moved out of plan_aggregate (the constants of `struct P`, the types of Row and Acc, whether
// qk_filter_agg_cons exists) for the same input — none is computed from the code under test.
#include <cstdio>
#include <vector>

#include "agg_shape.hpp"

using namespace qhip;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                 \
  do {                                                                              \
    ++g_checked;                                                                    \
    if (!(cond)) { ++g_failed; fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static const u128 kUnknown = ~(u128)0;   // ENode::maxabs of an unbounded value
static const u128 kSmall = ((u128)1 << 20) - 1;

// a GROUP BY over W key words with n SUM(Decimal128) cells over n distinct arguments of the given bound; nullable arguments
// also get their CELL_CNT
struct Plan {
  int W = 0, slot_words = 0;
  std::vector<CellDesc> cells;
  std::vector<ArgDesc> args;
};
static Plan sums(int W, int n, u128 maxabs, bool nullable = false) {
  Plan p;
  p.W = W;
  int off = 0;
  auto cell = [&](int kind, int arg, int words) { p.cells.push_back(CellDesc{kind, arg, false, off, words}); off += words; };
  cell(CELL_ROWS, -1, 1);
  for (int a = 0; a < n; ++a) {
    p.args.push_back(ArgDesc{a, DType(QHIP_DECIMAL128, 15, 2), nullable, true, maxabs, 16});
    cell(CELL_SUM_I128, a, 2);
    if (nullable) cell(CELL_CNT, a, 1);
  }
  p.slot_words = 1 + W + off;
  return p;
}
static AggShape shape(const Plan& p, bool narrow_copies, bool cons_columns, const AggShapeTuning& t = AggShapeTuning(), bool dev_rows = false, int rows_per_thread = 0) {
  return agg_shape(p.W, p.slot_words, p.cells, p.args, narrow_copies, dev_rows, cons_columns, rows_per_thread, t);
}
#define CHECK_SHAPE(s, kc, r, rc, pr) CHECK((s).KC == (kc) && (s).R == (r) && (s).RC == (rc) && (s).part_pr == (pr))

// ---------------------------------------------------------------- the catalog's shapes
static void test_catalog_shapes() {
  // q1_mini: one key word, one SUM; over the 16-byte layout, then with its values bounded (narrow copies, consecutive rows)
  CHECK(sums(1, 1, kUnknown).slot_words == 5);
  CHECK_SHAPE(shape(sums(1, 1, kUnknown), false, false), 4, 4, 0, 3);
  CHECK_SHAPE(shape(sums(1, 1, kSmall), true, true), 4, 4, 4, 3);
  // q1_full / q1_partial: two key words, five SUM cells
  CHECK(sums(2, 5, kUnknown).slot_words == 14);
  CHECK_SHAPE(shape(sums(2, 5, kUnknown), false, false), 4, 2, 0, 1);
  CHECK_SHAPE(shape(sums(2, 5, kSmall), true, true), 4, 2, 0, 1);      // bounded values, narrow copies
  CHECK_SHAPE(shape(sums(2, 5, kSmall), false, false), 2, 3, 0, 1);    // bounded values, Arrow layout
  // Q3's aggregate: three key words, one SUM; automatic R, one row per thread, and over a join output of deferred size
  CHECK(sums(3, 1, kUnknown).slot_words == 7);
  CHECK_SHAPE(shape(sums(3, 1, kUnknown), false, false), 4, 4, 0, 2);
  CHECK_SHAPE(shape(sums(3, 1, kUnknown), false, false, AggShapeTuning(), false, 1), 4, 1, 0, 2);
  CHECK_SHAPE(shape(sums(3, 1, kUnknown), false, false, AggShapeTuning(), true, 1), 4, 1, 0, 2);
  // no key: nothing to cache, whatever QHIP_AGG_KC says
  AggShapeTuning kc2;
  kc2.kc = EnvInt{true, true, 2};
  CHECK_SHAPE(shape(sums(0, 1, kUnknown), false, false, kc2), 0, 4, 0, 4);
}

// ---------------------------------------------------------------- maxabs at 2^39 and 2^63
static void test_argument_widths() {
  struct Row { u128 maxabs; bool arg64, acc64; };
  const Row rows[] = {{((u128)1 << 39) - 1, true, true}, {(u128)1 << 39, true, false}, {((u128)1 << 63) - 1, true, false}, {(u128)1 << 63, false, false}};
  for (const Row& w : rows) {
    const Plan p = sums(1, 1, w.maxabs);
    const AggShape s = shape(p, false, true);
    CHECK(s.arg64.size() == 1 && s.arg64[0] == w.arg64);
    CHECK(s.arg_acc64.size() == 1 && s.arg_acc64[0] == w.acc64);
    CHECK(s.acc64(p.cells[1]) == w.acc64 && !s.acc64(p.cells[0]));
    CHECK_SHAPE(s, 4, 4, 4, 3);
  }
  // a SUM(Int64): one u64 cell, nothing to narrow
  Plan p = sums(1, 1, kUnknown);
  p.args[0].type = DType(QHIP_INT64); p.args[0].width = 8; p.cells[1].kind = CELL_SUM_U64; p.cells[1].words = 1; p.slot_words = 4;
  const AggShape s = shape(p, false, true);
  CHECK(!s.arg64[0] && !s.arg_acc64[0]);
  CHECK_SHAPE(s, 4, 4, 4, 4);
}

// ---------------------------------------------------------------- the register budgets of the hot-key cache
static void test_hot_key_budgets() {
  struct Row { int n, kc, r, pr; };
  // wide sums (4 VGPRs per cell): KC 4 while 4 x part_regs <= 96, KC 2 while 2 x part_regs <= 96, else none
  const Row wide[] = {{5, 4, 2, 1}, {6, 4, 1, 0}, {7, 2, 2, 0}, {12, 2, 1, 0}, {13, 0, 2, 0}};
  for (const Row& w : wide) CHECK_SHAPE(shape(sums(1, w.n, kUnknown), false, false), w.kc, w.r, 0, w.pr);
  // every sum narrow (2 VGPRs per cell), 16-byte layout: KC = 24 / part_regs within 1..4
  const Row narrow24[] = {{3, 4, 4, 1}, {4, 3, 4, 1}, {6, 2, 3, 0}, {7, 1, 3, 0}, {12, 1, 1, 0}, {13, 1, 1, 0}};
  for (const Row& w : narrow24) CHECK_SHAPE(shape(sums(1, w.n, kSmall), false, false), w.kc, w.r, 0, w.pr);
  // ... streaming narrow copies: KC = 48 / part_regs within 1..4
  const Row narrow48[] = {{6, 4, 1, 0}, {7, 3, 1, 0}, {8, 3, 1, 0}, {9, 2, 1, 0}, {12, 2, 1, 0}, {13, 1, 1, 0}};
  for (const Row& w : narrow48) CHECK_SHAPE(shape(sums(1, w.n, kSmall), true, true), w.kc, w.r, 0, w.pr);
  // one wide cell among them (a nullable argument's count is a u64 cell): not "all narrow" — the 96-register rule again
  CHECK_SHAPE(shape(sums(1, 7, kSmall, true), true, false), 2, 3, 0, 0);
  CHECK_SHAPE(shape(sums(1, 13, kSmall, true), true, false), 0, 3, 0, 0);
}

// ---------------------------------------------------------------- the consecutive-rows form
static void test_consecutive_rows_rule() {
  // cached accumulators + four rows within 64 VGPRs: three narrow sums (4 x 6 + 4 x 9 = 60) have it, four (4 x 8 + 4 x 11 = 76) do not
  CHECK_SHAPE(shape(sums(1, 3, kSmall), true, true), 4, 4, 4, 1);
  CHECK_SHAPE(shape(sums(1, 4, kSmall), true, true), 4, 3, 0, 1);
  // ... and never when the columns do not allow it, for a device-side row count, or with QHIP_AGG_CONS=0
  AggShapeTuning t;
  CHECK_SHAPE(shape(sums(1, 1, kUnknown), false, false, t), 4, 4, 0, 3);
  CHECK_SHAPE(shape(sums(1, 1, kSmall), false, true, t, true), 4, 4, 0, 3);
  t.cons = 2;
  CHECK_SHAPE(shape(sums(1, 1, kSmall), false, true, t, true), 4, 4, 0, 3);
  CHECK_SHAPE(shape(sums(1, 1, kUnknown), false, false, t), 4, 4, 0, 3);
  CHECK_SHAPE(shape(sums(1, 1, kSmall), true, true, t), 4, 4, 4, 3);
  t.cons = 0;
  CHECK_SHAPE(shape(sums(1, 1, kSmall), false, true, t), 4, 4, 0, 3);
  CHECK_SHAPE(shape(sums(1, 1, kSmall), true, true, t), 4, 4, 0, 3);
  // a Q1-like list (two key words, four narrow sums over narrow copies: 4 x 8 + 4 x 13 VGPRs) gets it only when forced
  // (QHIP_AGG_CONS=2, RC = QHIP_AGG_CONS_R within 1..8) or with fewer cached keys
  const Plan q = sums(2, 4, kSmall);
  CHECK(q.slot_words == 12);
  t = AggShapeTuning();
  CHECK_SHAPE(shape(q, true, true, t), 4, 3, 0, 1);
  t.cons = 2;
  CHECK_SHAPE(shape(q, true, true, t), 4, 3, 4, 1);
  const int cons_r[][2] = {{2, 2}, {8, 8}, {0, 1}, {64, 8}};
  for (auto& w : cons_r) { t.cons_r = w[0]; CHECK_SHAPE(shape(q, true, true, t), 4, 3, w[1], 1); }
  t = AggShapeTuning();
  t.kc = EnvInt{true, true, 1};
  CHECK_SHAPE(shape(q, true, true, t), 1, 4, 4, 1);
  t.kc = EnvInt{true, true, 3};
  CHECK_SHAPE(shape(q, true, true, t), 3, 3, 0, 1);
  t.kc = EnvInt{true, true, 0};
  CHECK_SHAPE(shape(q, true, true, t), 0, 4, 4, 1);
  t.kc = EnvInt{true, false, 0};   // set to nothing: the rule's value
  CHECK_SHAPE(shape(q, true, true, t), 4, 3, 0, 1);
  CHECK_SHAPE(shape(q, false, false), 3, 3, 0, 1);   // (the same list over the 16-byte layout)
}

// ---------------------------------------------------------------- the staged scatter's rows per thread, down to 0
static void test_part_pr() {
  Plan count = sums(1, 0, kUnknown);   // COUNT(*) alone: 3 slot words
  CHECK(count.slot_words == 3);
  CHECK_SHAPE(shape(count, false, true), 4, 4, 4, 4);
  CHECK(shape(sums(1, 1, kUnknown), false, false).part_pr == 3);    // 5 slot words
  CHECK(shape(sums(3, 1, kUnknown), false, false).part_pr == 2);    // 7
  CHECK(shape(sums(1, 5, kUnknown), false, false).part_pr == 1);    // 13
  CHECK(shape(sums(2, 5, kUnknown), false, false).part_pr == 1);    // 14: the widest record that is staged
  CHECK(shape(sums(1, 6, kUnknown), false, false).part_pr == 0);    // 15: per-lane stores
  CHECK(shape(sums(1, 4, kSmall, true), true, false).part_pr == 0);
  // QHIP_AGG_PART_PR caps it (at least 1; set to nothing counts as 0)
  struct Row { EnvInt e; int pr; };
  const Row rows[] = {{EnvInt{true, true, 2}, 2}, {EnvInt{true, true, 0}, 1}, {EnvInt{true, true, 9}, 3}, {EnvInt{true, false, 0}, 1}, {EnvInt(), 3}};
  for (const Row& w : rows) {
    AggShapeTuning t;
    t.part_pr = w.e;
    CHECK_SHAPE(shape(sums(1, 1, kSmall), false, true, t), 4, 4, 4, w.pr);
  }
  // a given R is taken as it is
  CHECK_SHAPE(shape(sums(1, 1, kSmall), false, true, AggShapeTuning(), false, 8), 4, 8, 4, 3);
}

int main() {
  test_catalog_shapes();
  test_argument_widths();
  test_hot_key_budgets();
  test_consecutive_rows_rule();
  test_part_pr();
  printf("agg_shape_tests: %d checked, %d failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
