// agg_result.hpp — what the hash aggregate does with its group slots on the host: merging the replicas of the small first-attempt
// table, turning slots into output columns, describing the columns for the device-side assembly. Plain host code: no HIP
// runtime call and no Ctx, so all of it runs (and is tested, tests/cpp/agg_result_tests.cpp) without a GPU.
//
// A slot is plan.slot_words u64 words: [occupancy word | W key words (the first one the null mask when plan.null_mask_word) |
// cells at CellDesc::off].
#pragma once
#include <cstdint>
#include <vector>

#include "codegen.hpp"
#include "common.hpp"
#include "hostcol.hpp"
#include "kernels.hpp"

namespace qhip {

// the double whose order-preserving image (sign bit flipped / all bits complemented) is k
double ord_to_f64(uint64_t k);

// `slots` = G slots out of several table replicas: slots with the same key words become one (in the order of first appearance),
// every cell merged as the commutative monoid it is (wrapping adds, max). Returns the number of groups and shrinks `slots` to them.
uint32_t merge_replica_slots(const AggPlan& plan, std::vector<uint64_t>& slots, uint32_t G);

// the output columns (keys, then aggregates) of G merged slots. Throws Error for a Decimal AVG that overflows.
std::vector<HostColumn> assemble_host_columns(const AggPlan& plan, const std::vector<uint64_t>& slots, uint32_t G, int n_groups, int n_aggs,
                                              bool zero_batches_in);

// the same columns as k_agg_finalize's descriptors (out_values / out_valid left null: the caller allocates the columns)
std::vector<FinCol> describe_fin_cols(const AggPlan& plan, int n_groups, int n_aggs);

}  // namespace qhip
