// codegen.cpp — expression tree -> HIP policy struct source: one planner per kernel family.
//
// Only the per-row expression code (load columns, compare, decimal arithmetic, pack keys) is generated;
// every algorithmic piece (wave dedup, DPP reductions, LDS/HBM tables, atomics) is the hand-written
// template code of device/qhip_device.hpp that these policies plug into. Literal VALUES never appear
// in the generated text (they travel in KArgs.lit_*), so `l_shipdate < DATE x` compiles once for all x.
// The expression statements themselves come from ExprGen (exprgen.cpp), the aggregate's tuning values from agg_shape.cpp.
#include "codegen.hpp"

#include <algorithm>
#include <cstdlib>

#include "device/qhip_status.h"

namespace qhip {

// ---------------------------------------------------------------- shared by the planners of the software-pipelined kernels
// (plan_aggregate, plan_predicate_mask, plan_keys' raw kernels: ExprGen::use_tile_loads, then these)
static void check_predicate(const ExprSet& es, int root) {   // (root < 0: no filter)
  if (root >= 0 && es.at(root).type.id != QHIP_BOOL) fail(QHIP_INVALID_ARGUMENT, "filter predicate must be Boolean, got " + dtype_name(es.at(root).type));
}
// a row passes when the predicate is valid and true
static std::string pass_expr(const ExprGen& g, int root) { return g.ok(root) + " && " + g.val(root); }
// `struct Raw` (what load() leaves of a row) and load(): branch-free, issued for a whole tile before any row is evaluated
static std::string raw_loads(const ExprGen& g) {
  return "  struct Raw {\n" + g.raw_fields + "    int unused_;\n  };\n"
         "  __device__ static __forceinline__ void load(const KArgs& a, const i64 tb, const u32 o, Raw& w) {\n" + g.load_code + "    w.unused_ = 0;\n  }\n";
}

// ---------------------------------------------------------------- key packing shared by aggregate / join / partition kernels
// Key types: the reference's create_hashes (utils/array.rs:190-210) hashes Int64, UInt8, Int32, Utf8, Date32 / Date64,
// Time32 / Time64, Decimal128 and Decimal256 and raises an InternalError for anything else. The HIP path takes the same list
// MINUS Decimal256 (out of scope, DESIGN §8: no such type id crosses the C ABI): a plan with such a key gets the reference's
// own error text here and the shim keeps the CPU node — a documented gap, not a drop-in.
void check_key_type(const DType& t) {
  switch (t.id) {
    case QHIP_INT64: case QHIP_UINT8: case QHIP_INT32: case QHIP_UTF8: case QHIP_DATE32: case QHIP_DATE64: case QHIP_DECIMAL128:
    case QHIP_TIME32_S: case QHIP_TIME32_MS: case QHIP_TIME64_US: case QHIP_TIME64_NS:
      return;
    default:
      fail(QHIP_INVALID_ARGUMENT, "Internal error: Unsupported data type in hasher: " + dtype_name(t));
  }
}

int packed_key_words(const DType& t, int utf8_max_len) {
  if (t.id == QHIP_UTF8) return std::max(1, (utf8_max_len + 1 + 7) / 8);
  return t.id == QHIP_DECIMAL128 ? 2 : 1;
}

// words of a packed Utf8 key: the bytes little-endian across the words, the length in the top byte of the last word
static int utf8_key_words(const ExprSet& es, const std::vector<InputCol>& input, int root) {
  const ENode& nd = es.at(root);
  int maxlen = 7;
  if (nd.kind == QHIP_EXPR_COLUMN && input[(size_t)nd.column].utf8_max_len >= 0) maxlen = input[(size_t)nd.column].utf8_max_len;
  else if (nd.kind == QHIP_EXPR_LITERAL) maxlen = (int)nd.s.size();
  const int words = packed_key_words(nd.type, maxlen);
  // (up to 7 words = 55 bytes + the length byte per Utf8 key — round 4; rounds 1-3: 4 words — inside the 8 words a whole key may have)
  if (words > kMaxUtf8KeyWords) fail(QHIP_UNSUPPORTED, "Utf8 group/join key longer than 55 bytes is not accelerated");
  return words;
}

bool packed_key_fits(const std::vector<InputCol>& input, const int32_t* cols, int n) {
  int W = 0;
  bool mask_word = false;
  for (int k = 0; k < n; ++k) {
    const InputCol& ic = input[(size_t)cols[k]];
    mask_word = mask_word || ic.has_nulls || ic.type.id == QHIP_NULL;
    const int words = packed_key_words(ic.type, ic.utf8_max_len >= 0 ? ic.utf8_max_len : 7);
    if (ic.type.id == QHIP_UTF8 && words > kMaxUtf8KeyWords) return false;
    W += words;
  }
  return W + (mask_word ? 1 : 0) <= kMaxKeyWords;
}

static void layout_keys(const ExprSet& es, const std::vector<InputCol>& input, const int32_t* roots, int n, bool with_null_mask,
                        std::vector<KeyDesc>& keys, int& W, bool& mask_word) {
  keys.clear();
  mask_word = false;
  if (with_null_mask)
    for (int k = 0; k < n; ++k) if (es.at(roots[k]).nullable) mask_word = true;
  int off = mask_word ? 1 : 0;
  for (int k = 0; k < n; ++k) {
    const ENode& nd = es.at(roots[k]);
    check_key_type(nd.type);
    KeyDesc kd;
    kd.root = roots[k]; kd.type = nd.type; kd.nullable = nd.nullable; kd.word_off = off;
    kd.words = nd.type.id == QHIP_UTF8 ? utf8_key_words(es, input, roots[k]) : packed_key_words(nd.type, 0);
    off += kd.words;
    keys.push_back(kd);
  }
  W = off;
  if (n > 60) fail(QHIP_UNSUPPORTED, "more than 60 key columns");
}

// statements storing the key words of the current row into `dst[...]`; `valid_all` receives the conjunction of validities
static void emit_key_words(ExprGen& g, const ExprSet& es, const std::vector<KeyDesc>& keys, bool mask_word, const std::string& dst,
                           std::string& out, std::string* valid_all) {
  std::ostringstream o;
  std::string all = "true";
  if (mask_word) o << "    u64 nm = 0;\n";
  for (size_t k = 0; k < keys.size(); ++k) {
    const KeyDesc& kd = keys[k];
    std::string code;
    g.emit(kd.root, code);
    o << code;
    const std::string okx = g.ok(kd.root);
    const std::string w = dst + "[" + std::to_string(kd.word_off) + "]";
    std::string value;
    if (kd.type.id == QHIP_UTF8) {
      if (g.raw_key_prefetched(kd.root))
        o << "    u64 ks" << k << "[" << kd.words << "]; qh_pack_words<" << kd.words << ">(w.k" << kd.root << ", " << g.len(kd.root) << ", ks" << k << ");\n";
      else
        o << "    u64 ks" << k << "[" << kd.words << "]; qh_pack_str<" << kd.words << ">(" << g.ptr(kd.root) << ", " << g.len(kd.root) << ", ks" << k << ");\n";
      o << "    if (" << okx << " && " << g.len(kd.root) << " > " << 8 * kd.words - 1 << ") err |= " << (1u << QS_KEY_TOO_LONG) << "u;\n";
      for (int w2 = 0; w2 < kd.words; ++w2)
        o << "    " << dst << "[" << kd.word_off + w2 << "] = " << (kd.nullable ? okx + " ? " : std::string("")) << "ks" << k << "[" << w2 << "]"
          << (kd.nullable ? " : 0ULL" : "") << ";\n";
      if (kd.nullable) { if (mask_word) o << "    nm |= " << okx << " ? 0ULL : " << (1ULL << k) << "ULL;\n"; all += " && " + okx; }
      continue;
    } else if (kd.type.id == QHIP_DECIMAL128) {
      value = "(u64)(u128)" + g.val(kd.root);
    } else {
      value = "(u64)(i64)" + g.val(kd.root);
    }
    if (kd.nullable) {
      o << "    " << w << " = " << okx << " ? " << value << " : 0ULL;\n";
      if (kd.type.id == QHIP_DECIMAL128)
        o << "    " << dst << "[" << kd.word_off + 1 << "] = " << okx << " ? (u64)((u128)" << g.val(kd.root) << " >> 64) : 0ULL;\n";
      if (mask_word) o << "    nm |= " << okx << " ? 0ULL : " << (1ULL << k) << "ULL;\n";
      all += " && " + okx;
    } else {
      o << "    " << w << " = " << value << ";\n";
      if (kd.type.id == QHIP_DECIMAL128) o << "    " << dst << "[" << kd.word_off + 1 << "] = (u64)((u128)" << g.val(kd.root) << " >> 64);\n";
    }
  }
  if (mask_word) o << "    " << dst << "[0] = nm;\n";
  out += o.str();
  if (valid_all) *valid_all = all;
}

// ---------------------------------------------------------------- aggregate policy
static std::string ord64(const DType& t, const std::string& v) {
  if (dtype_is_float(t)) return "qh_f64_ord((double)" + v + ")";
  if (signed_intlike(t)) return "((u64)(i64)" + v + " ^ 0x8000000000000000ULL)";
  return "(u64)" + v;
}

// stage 2: validates the aggregates and lays out P.args (shared by equal expressions), P.cells (cell 0 counts the rows of the
// group; shared by equal (kind, argument) pairs; with their word offsets), P.aggs and P.slot_words
static void agg_cells(const ExprSet& es, const qhip_agg* aggs, int n_aggs, AggPlan& P) {
  auto add_cell = [&](int kind, int arg, bool is_min, int words) {
    for (size_t c = 0; c < P.cells.size(); ++c)
      if (P.cells[c].kind == kind && P.cells[c].arg == arg && P.cells[c].is_min == is_min) return (int)c;
    CellDesc cd; cd.kind = kind; cd.arg = arg; cd.is_min = is_min; cd.words = words; cd.off = 0;
    P.cells.push_back(cd);
    return (int)P.cells.size() - 1;
  };
  add_cell(CELL_ROWS, -1, false, 1);
  auto arg_index = [&](int root) {
    const ENode& nd = es.at(root);
    for (size_t a = 0; a < P.args.size(); ++a) if (es.at(P.args[a].root).canon == nd.canon) return (int)a;
    ArgDesc ad; ad.root = root; ad.type = nd.type; ad.nullable = nd.nullable; ad.value_needed = false; ad.maxabs = nd.maxabs; ad.width = dtype_width(nd.type);
    P.args.push_back(ad);
    return (int)P.args.size() - 1;
  };
  for (int k = 0; k < n_aggs; ++k) {
    const qhip_agg& a = aggs[k];
    if (a.expr < 0 || a.expr >= (int)es.nodes.size()) fail(QHIP_INVALID_ARGUMENT, "aggregate argument index out of range");
    const ENode& arg = es.at(a.expr);
    AggDesc ad; ad.kind = a.kind; ad.ret = DType(a.return_type); ad.value_cell = -1; ad.count_cell = 0;
    // a NULL-typed / all-null literal argument never contributes
    ad.arg = arg_index(a.expr);
    const bool nullable = arg.nullable;
    auto count_cell = [&]() { return nullable ? add_cell(CELL_CNT, ad.arg, false, 1) : 0; };
    switch (a.kind) {
      case QHIP_AGG_COUNT:
        ad.ret = DType(QHIP_INT64);
        ad.count_cell = count_cell();
        break;
      case QHIP_AGG_SUM: {
        // sum.rs:36-51: only these return types have an accumulator, and the argument array is downcast to it
        if (!(ad.ret.id == QHIP_UINT64 || ad.ret.id == QHIP_INT64 || ad.ret.id == QHIP_FLOAT64 || ad.ret.id == QHIP_DECIMAL128))
          fail(QHIP_INVALID_ARGUMENT, "Internal error: Sum not supported for " + arg.canon + ": " + dtype_name(ad.ret));
        if (arg.type.id != ad.ret.id)
          fail(QHIP_INVALID_ARGUMENT, "SUM argument type " + dtype_name(arg.type) + " does not match return type " + dtype_name(ad.ret));
        const int kind = ad.ret.id == QHIP_DECIMAL128 ? CELL_SUM_I128 : ad.ret.id == QHIP_FLOAT64 ? CELL_SUM_F64 : CELL_SUM_U64;
        ad.value_cell = add_cell(kind, ad.arg, false, kind == CELL_SUM_I128 ? 2 : 1);
        ad.count_cell = count_cell();
        break;
      }
      case QHIP_AGG_AVG: {
        // avg.rs:36-61
        if (arg.type.id == QHIP_DECIMAL128 && ad.ret.id == QHIP_DECIMAL128) {
          ad.value_cell = add_cell(CELL_SUM_I128, ad.arg, false, 2);
        } else if (arg.type.id == QHIP_FLOAT64 && ad.ret.id == QHIP_FLOAT64) {
          ad.value_cell = add_cell(CELL_SUM_F64, ad.arg, false, 1);
        } else {
          fail(QHIP_INVALID_ARGUMENT, "Internal error: Unsupported data type [" + dtype_name(ad.ret) + "] for AVG aggregate over " + dtype_name(arg.type));
        }
        ad.count_cell = count_cell();
        break;
      }
      case QHIP_AGG_MIN:
      case QHIP_AGG_MAX: {
        if (arg.type != ad.ret) fail(QHIP_INVALID_ARGUMENT, "MIN/MAX argument type differs from return type");
        const bool is_min = a.kind == QHIP_AGG_MIN;
        if (arg.type.id == QHIP_DECIMAL128) ad.value_cell = add_cell(CELL_MAXORD128, ad.arg, is_min, 3);
        else if (intlike(arg.type) || dtype_is_float(arg.type)) ad.value_cell = add_cell(CELL_MAXORD64, ad.arg, is_min, 1);
        else fail(QHIP_UNSUPPORTED, "MIN/MAX over " + dtype_name(arg.type));
        ad.count_cell = count_cell();
        break;
      }
      default:
        fail(QHIP_INVALID_ARGUMENT, "unknown aggregate kind " + std::to_string(a.kind));
    }
    P.aggs.push_back(ad);
  }
  int off = 0;
  for (auto& c : P.cells) {
    c.off = off; off += c.words;
    if (c.arg >= 0 && c.kind != CELL_CNT) P.args[(size_t)c.arg].value_needed = true;
  }
  P.slot_words = 1 + P.W + off;
}

static AggShapeTuning agg_tuning_from_env() {
  AggShapeTuning t;
  t.kc = env_opt("QHIP_AGG_KC"); t.part_pr = env_opt("QHIP_AGG_PART_PR");
  t.cons = env_int("QHIP_AGG_CONS", 1); t.cons_r = env_int("QHIP_AGG_CONS_R", 4); t.cons_sb = env_int("QHIP_AGG_CONS_SB", 4);
  t.cons_pipe = env_int("QHIP_AGG_CONS_PIPE", 1); t.prof = env_int("QHIP_AGG_PROF", 0); t.pipe = env_int("QHIP_AGG_PIPE", 0); t.waves = env_int("QHIP_AGG_WAVES", 0);
  return t;
}

// whether every column the plan references allows the consecutive-rows form (agg_shape.cpp): plain (no index vector, no validity
// bitmap, no Boolean, strings only as one-byte flags) and at most 8 bytes wide in the layout that is streamed
static bool cons_columns(const ExprSet& es, const std::vector<InputCol>& input, std::vector<int> todo) {
  bool ok = !input.empty();
  int widest = 0;
  std::vector<char> used(es.nodes.size(), 0);
  while (!todo.empty()) {
    const int k = todo.back();
    todo.pop_back();
    if (k < 0 || k >= (int)es.nodes.size() || used[(size_t)k]) continue;
    used[(size_t)k] = 1;
    todo.push_back(es.nodes[(size_t)k].left); todo.push_back(es.nodes[(size_t)k].right); todo.push_back(es.nodes[(size_t)k].third);
  }
  for (size_t c = 0; c < es.nodes.size(); ++c) {
    const ENode& nd = es.nodes[c];
    if (!used[c] || nd.kind != QHIP_EXPR_COLUMN || nd.type.id == QHIP_NULL) continue;
    const InputCol& ic = input[(size_t)nd.column];
    if (ic.indirect || nd.nullable || nd.type.id == QHIP_BOOL) ok = false;
    else if (nd.type.id == QHIP_UTF8) { if (!ic.utf8_fixed1) ok = false; else widest = std::max(widest, 1); }
    else {
      const int nb = (nd.type.id == QHIP_DECIMAL128 || (nd.type.id == QHIP_INT64 && ic.narrow_bytes == 4)) ? ic.narrow_bytes : 0;
      const int w = nb ? nb : dtype_width(nd.type);
      if (w <= 0 || w > 8) ok = false;
      widest = std::max(widest, w);
    }
  }
  return ok && widest > 0;
}

// stage 4: `struct P {` and its constants
static void emit_agg_constants(std::ostringstream& s, const AggPlan& P, const AggShapeTuning& t) {
  s << "struct P {\n";
  s << "  static constexpr int W = " << P.W << ";\n  static constexpr int R = " << P.R << ";\n  static constexpr int SLOT_WORDS = " << P.slot_words << ";\n";
  s << "  static constexpr int PROF = " << (t.prof != 0 ? 1 : 0) << ";   // phase timers (s_memtime) summed into status words 8..12 (measurements only)\n";
  s << "  static constexpr int PIPE = " << (t.pipe != 0 ? 1 : 0) << ";   // two register sets: the next tile's loads fly while a tile is evaluated\n";
  s << "  static constexpr int PART_PR = " << P.part_pr << ";\n";
  // how the sorted-run kernel orders two key words (any total order makes "non-decreasing" imply "equal keys adjacent"; these
  // make the usual sort orders — signed integers, bytewise strings — pass): Utf8 words compare byte-swapped (the bytes are packed
  // little-endian), signed integer words with the sign bit flipped
  unsigned long long swap_mask = 0, sign_mask = 0;
  for (auto& kd : P.keys) {
    for (int w2 = 0; w2 < kd.words; ++w2) {
      if (kd.type.id == QHIP_UTF8) swap_mask |= 1ull << (kd.word_off + w2);
      else if (kd.words == 1 && kd.type.id != QHIP_UINT8) sign_mask |= 1ull << (kd.word_off + w2);
    }
  }
  s << "  static constexpr unsigned long long KEY_SWAP_MASK = " << swap_mask << "ULL, KEY_SIGN_MASK = " << sign_mask << "ULL;\n";
  s << "  static constexpr int RC = " << std::max(1, P.RC) << ";\n";
  s << "  static constexpr int CSB = " << std::max(1, std::min(4, t.cons_sb)) << ";\n";
  s << "  static constexpr int CPIPE = " << (t.cons_pipe != 0 ? 1 : 0) << ";\n";
  s << "  static constexpr int KC = " << P.KC << ";\n";
}

static const char* cell_ctype(int kind, bool narrow) {
  return kind == CELL_SUM_I128 ? (narrow ? "i64" : "i128") : kind == CELL_SUM_F64 ? "double" : kind == CELL_MAXORD128 ? "u128" : "u64";
}

// stage 5: Row (what eval() leaves of a row), Part (one value per cell)
static void emit_agg_structs(std::ostringstream& s, const AggPlan& P, const AggShape& sh) {
  s << "  struct Row {\n    bool pass;\n    u64 key[" << (P.W > 0 ? P.W : 1) << "];\n";
  for (size_t a = 0; a < P.args.size(); ++a) {
    const ArgDesc& ad = P.args[a];
    if (ad.value_needed) s << "    " << (sh.arg64[a] ? std::string("i64") : ExprGen::ctype(ad.type)) << " a" << a << ";\n";
    if (ad.nullable) s << "    bool h" << a << ";\n";
  }
  s << "  };\n";
  s << "  struct Part {\n";
  for (size_t c = 0; c < P.cells.size(); ++c) s << "    " << cell_ctype(P.cells[c].kind, false) << " c" << c << ";\n";
  s << "  };\n";
}

// stage 6: two phases per row: load() is branch-free and only issues the row's loads into `Raw w` (the kernel calls it for all R
// rows of a tile first, so their memory latencies overlap); eval() computes predicate, keys and aggregate arguments
// from w and may contain control flow (string compares, the tiered decimal multiply) without serialising any load
static void emit_agg_eval(std::ostringstream& s, ExprGen& g, const ExprSet& es, int predicate_root, const AggPlan& P, const AggShape& sh) {
  std::string ev;
  if (predicate_root >= 0) {
    g.emit(predicate_root, ev);
    ev += "    r.pass = " + pass_expr(g, predicate_root) + ";\n";
    g.set_err_gate("r.pass");   // keys and arguments raise only for rows the fused filter passes (the predicate itself: every row)
  } else {
    ev += "    r.pass = true;\n";
  }
  emit_key_words(g, es, P.keys, P.null_mask_word, "r.key", ev, nullptr);
  for (size_t a = 0; a < P.args.size(); ++a) {
    const ArgDesc& ad = P.args[a];
    g.emit(ad.root, ev);
    if (ad.value_needed) ev += "    r.a" + std::to_string(a) + " = " + (sh.arg64[a] ? "(i64)(u64)(u128)" : "") + g.val(ad.root) + ";\n";
    if (ad.nullable) ev += "    r.h" + std::to_string(a) + " = " + g.ok(ad.root) + ";\n";
  }
  s << raw_loads(g);
  s << "  __device__ static __forceinline__ void eval(const KArgs& a, const Raw& w, Row& r, u32& err) {\n" << ev << "  }\n";
}

// stage 7: part_add (narrow = false) / acc_add (narrow = true)
// ROWS = false: the caller knows the row count from ballot popcounts (part_set_rows) and saves the per-lane adds.
// Sums are written as `if (take) acc += v` so that the compiler can run the adds under the EXEC mask instead of
// paying a v_cndmask per dword on top of every add. Acc = the lane-private accumulators of the hot-key cache (and of the
// ungrouped aggregate): Part with the narrow SUM cells in 64 bits.
static void emit_agg_add(std::ostringstream& s, const AggPlan& P, const AggShape& sh, bool narrow) {
  if (narrow) {
    s << "  struct Acc {\n";
    for (size_t c = 0; c < P.cells.size(); ++c) s << "    " << cell_ctype(P.cells[c].kind, sh.acc64(P.cells[c])) << " c" << c << ";\n";
    s << "  };\n";
  }
  s << "  __device__ static __forceinline__ void " << (narrow ? "acc_init(Acc& p" : "part_init(Part& p") << ") {\n";
  for (size_t c = 0; c < P.cells.size(); ++c) s << "    p.c" << c << " = 0;\n";
  s << "  }\n";
  if (narrow) {
    s << "  __device__ static __forceinline__ void acc_to_part(const Acc& a, Part& p) {\n";
    for (size_t c = 0; c < P.cells.size(); ++c) s << "    p.c" << c << " = " << (sh.acc64(P.cells[c]) ? "(i128)" : "") << "a.c" << c << ";\n";
    s << "  }\n";
  }
  s << "  template <bool ROWS> __device__ static __forceinline__ void " << (narrow ? "acc_add(Acc& p" : "part_add(Part& p") << ", const Row& r, const bool m) {\n";
  for (size_t c = 0; c < P.cells.size(); ++c) {
    const CellDesc& cd = P.cells[c];
    const std::string C = "p.c" + std::to_string(c);
    if (cd.kind == CELL_ROWS) { s << "    if (ROWS) " << C << " += m ? 1ULL : 0ULL;\n"; continue; }
    const ArgDesc& ad = P.args[(size_t)cd.arg];
    const std::string A = "r.a" + std::to_string(cd.arg);
    const std::string take = ad.nullable ? "(m && r.h" + std::to_string(cd.arg) + ")" : std::string("m");
    switch (cd.kind) {
      case CELL_SUM_I128:
        if (narrow && sh.acc64(cd)) s << "    if (" << take << ") " << C << " = (i64)((u64)" << C << " + (u64)" << A << ");\n";
        else s << "    if (" << take << ") " << C << " = (i128)((u128)" << C << " + (u128)(i128)" << A << ");\n";
        break;
      case CELL_SUM_U64: s << "    if (" << take << ") " << C << " += (u64)" << A << ";\n"; break;
      case CELL_SUM_F64: s << "    if (" << take << ") " << C << " += (double)" << A << ";\n"; break;
      case CELL_CNT: s << "    " << C << " += " << take << " ? 1ULL : 0ULL;\n"; break;
      case CELL_MAXORD64: {
        const std::string o = std::string(cd.is_min ? "~" : "") + ord64(ad.type, A);
        s << "    { const u64 o = " << take << " ? " << o << " : 0ULL; " << C << " = o > " << C << " ? o : " << C << "; }\n";
        break;
      }
      case CELL_MAXORD128: {
        const std::string o = std::string(cd.is_min ? "~" : "") + "((u128)(i128)" + A + " ^ ((u128)1 << 127))";
        s << "    { const u128 o = " << take << " ? " << o << " : (u128)0; " << C << " = o > " << C << " ? o : " << C << "; }\n";
        break;
      }
    }
  }
  s << "  }\n";
}

// per CellKind: how a cell combines: its wave reduction is qh_wave_<op>_<type>, its slot update qh_acc_add_<type> / qh_acc_max_<type>
static const char* const kCellOp[] = {"sum_u64", "sum_i128", "sum_u64", "sum_f64", "sum_u64", "max_u64", "max_u128"};

// stage 8: part_set_rows; part_reduce: a wavefront's lanes into one Part
static void emit_agg_reduce(std::ostringstream& s, const AggPlan& P) {
  s << "  __device__ static __forceinline__ void part_set_rows(Part& p, const u64 n) { p.c0 = n; }\n";
  s << "  template <bool ROWS> __device__ static __forceinline__ void part_reduce(Part& p) {\n";
  for (size_t c = 0; c < P.cells.size(); ++c)
    s << "    " << (P.cells[c].kind == CELL_ROWS ? "if (ROWS) " : "") << "p.c" << c << " = qh_wave_" << kCellOp[P.cells[c].kind] << "(p.c" << c << ");\n";
  s << "  }\n";
}

// stage 9: slot_update: Part -> a table slot (atomics of memory space M); part_from_slot / part_to_slot: a slot-shaped record
// (plain memory) <-> Part; slot_merge: LDS slot (plain reads, after the workgroup barrier) -> HBM slot; and the struct's end
static void emit_agg_slot(std::ostringstream& s, const AggPlan& P) {
  s << "  template <class M> __device__ static __forceinline__ void slot_update(u64* slot, const Part& p) {\n";
  s << "    u64* cell = slot + " << 1 + P.W << ";\n";
  for (size_t c = 0; c < P.cells.size(); ++c) {
    const CellDesc& cd = P.cells[c];
    const std::string C = "p.c" + std::to_string(c);
    const bool max = cd.kind == CELL_MAXORD64 || cd.kind == CELL_MAXORD128;   // (a maximum of 0 = no value: nothing to store)
    s << "    " << (max ? "if (" + C + ") qh_acc_max_" : "qh_acc_add_") << (kCellOp[cd.kind] + 4) << "<M>(cell + " << cd.off << ", " << C << ");\n";
  }
  s << "  }\n";
  s << "  __device__ static __forceinline__ void part_from_slot(const u64* ls, Part& q) {\n";
  s << "    const u64* cell = ls + " << 1 + P.W << ";\n";
  for (size_t c = 0; c < P.cells.size(); ++c) {
    const CellDesc& cd = P.cells[c];
    const std::string at = "cell[" + std::to_string(cd.off) + "]", at1 = "cell[" + std::to_string(cd.off + 1) + "]";
    switch (cd.kind) {
      case CELL_SUM_I128: s << "    q.c" << c << " = qh_mk128(" << at << ", (i64)" << at1 << ");\n"; break;
      case CELL_SUM_F64: s << "    q.c" << c << " = qh_f64(" << at << ");\n"; break;
      case CELL_MAXORD128: s << "    q.c" << c << " = ((u128)" << at1 << " << 64) | (u128)" << at << ";\n"; break;
      default: s << "    q.c" << c << " = " << at << ";\n"; break;
    }
  }
  s << "  }\n";
  s << "  __device__ static __forceinline__ void part_to_slot(u64* ls, const Part& q) {\n";
  s << "    u64* cell = ls + " << 1 + P.W << ";\n";
  for (size_t c = 0; c < P.cells.size(); ++c) {
    const CellDesc& cd = P.cells[c];
    const std::string at = "cell[" + std::to_string(cd.off) + "]", at1 = "cell[" + std::to_string(cd.off + 1) + "]", C = "q.c" + std::to_string(c);
    switch (cd.kind) {
      case CELL_SUM_I128: case CELL_MAXORD128: s << "    " << at << " = (u64)(u128)" << C << "; " << at1 << " = (u64)((u128)" << C << " >> 64);\n"; break;
      case CELL_SUM_F64: s << "    " << at << " = (u64)__double_as_longlong(" << C << ");\n"; break;
      default: s << "    " << at << " = " << C << ";\n"; break;
    }
  }
  s << "  }\n";
  s << "  __device__ static __forceinline__ void slot_merge(u64* gs, const u64* ls) {\n    Part q;\n    part_from_slot(ls, q);\n";
  s << "    slot_update<MemHbm>(gs, q);\n  }\n";
  s << "};\n";
}

// stage 10: the kernels that instantiate the hand-written bodies with P; sets P.has_runs
static void emit_agg_entry_points(std::ostringstream& s, AggPlan& P, bool filtered, bool dev_rows, int waves) {
  const char* dr = dev_rows ? ", true" : "";   // the instantiation that reads the row count from the device (a join output of deferred size)
  const std::string wattr = waves > 0 ? "__attribute__((amdgpu_waves_per_eu(" + std::to_string(waves) + "))) " : std::string();
  s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) " << wattr << "void qk_filter_agg(KArgs a, AggLaunch L) { qh_filter_agg_body<P" << dr << ">(a, L); }\n";
  // 1024-thread workgroups, one per CU, sharing one LDS table of up to 128 KB (mid-sized many-group inputs, agg.cpp)
  if (P.W > 0)
    s << "extern \"C\" __global__ __launch_bounds__(1024) void qk_filter_agg_wide(KArgs a, AggLaunch L) { qh_filter_agg_body<P, " << (dev_rows ? "true" : "false")
      << ", 1024>(a, L); }\n";
  // ... an input whose equal keys are adjacent (checked on the device): runs instead of a hash table
  if (P.W > 0 && !filtered) {
    P.has_runs = true;
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_agg_runs(KArgs a, RunsLaunch L) { qh_agg_runs_body<P" << dr << ">(a, L); }\n";
  }
  // ... a lane owning RC consecutive rows (narrow plain layouts: wide loads)
  if (P.RC > 0)
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) " << wattr << "void qk_filter_agg_cons(KArgs a, AggLaunch L) { qh_filter_agg_body<P, false, QH_BLOCK, false, true>(a, L); }\n";
  // ... and over an input pre-partitioned by key hash, one part per workgroup (AggLaunch::part_runs; agg.cpp)
  if (P.W > 0 && !dev_rows)
    s << "extern \"C\" __global__ __launch_bounds__(1024) void qk_filter_agg_parts(KArgs a, AggLaunch L) { qh_filter_agg_body<P, false, 1024, true>(a, L); }\n";
  if (P.W == 0) return;
  // the partitioned path for many groups on a big input (same policy, three more entry points of the same module)
  s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_agg_part_hist(KArgs a, PartLaunch L) { qh_agg_part_body<P, false" << dr << ">(a, L); }\n";
  s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_agg_part_scatter(KArgs a, PartLaunch L) { qh_agg_part_body<P, true" << dr << ">(a, L); }\n";
  if (P.part_pr > 0)
    s << "extern \"C\" __global__ __launch_bounds__(QH_STAGE_BLOCK) void qk_agg_part_stage(KArgs a, PartLaunch L) { qh_agg_part_stage_body<P" << dr << ">(a, L); }\n";
  s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_agg_reduce(ReduceLaunch R, AggLaunch L) { qh_agg_reduce_body<P>(R, L); }\n";
  s << "extern \"C\" __global__ __launch_bounds__(1024) void qk_agg_reduce_wide(ReduceLaunch R, AggLaunch L) { qh_agg_reduce_body<P, 1024>(R, L); }\n";
}

// plan_aggregate, stage by stage (every stage is a function above; the text they append is the policy `struct P` that
// device/qhip_device.hpp's aggregate bodies are instantiated with, and their entry points):
//    1. check_predicate, layout_keys   the filter is Boolean; the group key's words (at most kMaxKeyWords with the null mask)
//    2. agg_cells                      validates the aggregates; P.args, P.cells with their offsets, P.aggs, P.slot_words
//    3. agg_shape (agg_shape.cpp)      the tuning policy: KC, R, RC, PART_PR and the 64-bit arguments, from the register
//                                      budget, the QHIP_AGG_* switches (agg_tuning_from_env) and what the columns allow
//    4. emit_agg_constants             `struct P {`, W, R, SLOT_WORDS, ..., KC
//    5. emit_agg_structs               Row, Part
//    6. emit_agg_eval                  Raw, load(), eval(): the only stage that generates expression code (ExprGen)
//    7. emit_agg_add                   part_init, part_add; then Acc, acc_init, acc_to_part, acc_add
//    8. emit_agg_reduce                part_set_rows, part_reduce
//    9. emit_agg_slot                  slot_update, part_from_slot, part_to_slot, slot_merge; `};`
//   10. emit_agg_entry_points          qk_filter_agg and the variants the plan's shape allows
void plan_aggregate(const ExprSet& es, const std::vector<InputCol>& input, int predicate_root, const int32_t* group_roots, int n_groups,
                    const qhip_agg* aggs, int n_aggs, int rows_per_thread, AggPlan& P, bool dev_rows) {
  P = AggPlan();
  check_predicate(es, predicate_root);
  layout_keys(es, input, group_roots, n_groups, true, P.keys, P.W, P.null_mask_word);
  if (P.W > kMaxKeyWords) fail(QHIP_UNSUPPORTED, "group key wider than 8 words");
  agg_cells(es, aggs, n_aggs, P);

  const AggShapeTuning tuning = agg_tuning_from_env();
  bool narrow_copies = false;
  for (auto& ic : input) if (ic.narrow_bytes > 0 && !ic.indirect) narrow_copies = true;
  std::vector<int> roots(group_roots, group_roots + n_groups);
  roots.push_back(predicate_root);
  for (int k = 0; k < n_aggs; ++k) roots.push_back(aggs[k].expr);
  const AggShape sh = agg_shape(P.W, P.slot_words, P.cells, P.args, narrow_copies, dev_rows, cons_columns(es, input, roots), rows_per_thread, tuning);
  P.KC = sh.KC; P.R = sh.R; P.RC = sh.RC; P.part_pr = sh.part_pr;

  ExprGen g(es, input);
  g.use_tile_loads(P.keys);
  std::ostringstream s;
  emit_agg_constants(s, P, tuning);
  emit_agg_structs(s, P, sh);
  emit_agg_eval(s, g, es, predicate_root, P, sh);
  emit_agg_add(s, P, sh, false);
  emit_agg_add(s, P, sh, true);
  emit_agg_reduce(s, P);
  emit_agg_slot(s, P);
  emit_agg_entry_points(s, P, predicate_root >= 0, dev_rows, tuning.waves);
  P.kernel_name = "qk_filter_agg";
  P.source = s.str();
  P.bind = g.bind;
}

void plan_predicate_mask(const ExprSet& es, const std::vector<InputCol>& input, int root, MaskPlan& out) {
  if (root < 0 || root >= (int)es.nodes.size()) fail(QHIP_INVALID_ARGUMENT, "predicate root out of range");
  check_predicate(es, root);
  ExprGen g(es, input);
  // the mask kernel is software-pipelined over its tiles: a row's column loads (load(): branch-free, tile-relative
  // addressing) are issued two tiles before the predicate is evaluated from them (pred())
  g.use_tile_loads({});
  std::string code;
  g.emit(root, code);
  std::ostringstream s;
  out.mask_r = std::max(1, std::min(16, env_int("QHIP_MASK_R", 4)));
  s << "struct P {\n  static constexpr int MASK_R = " << out.mask_r << ";\n";
  s << raw_loads(g);
  s << "  __device__ static __forceinline__ bool pred(const KArgs& a, const Raw& w, u32& err) {\n" << code;
  s << "    return " << pass_expr(g, root) << ";\n  }\n};\n";
  s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_pred_mask(KArgs a, u64* mask, u32* wave_count, u32* status) { "
       "qh_pred_mask_body<P>(a, mask, wave_count, status); }\n";
  out.source = s.str();
  out.kernel_name = "qk_pred_mask";
  out.bind = g.bind;
}

void plan_keys(const ExprSet& es, const std::vector<InputCol>& input, const int32_t* roots, int n, KeysPlan& out, int predicate_root,
               int kernel, bool dev_rows, int n_parts) {
  out = KeysPlan();
  layout_keys(es, input, roots, n, false, out.keys, out.W, out.null_mask_word);
  if (out.W > kMaxKeyWords) fail(QHIP_UNSUPPORTED, "join key wider than 8 words");
  ExprGen g(es, input);
  const bool raw = kernel == KEYS_KERNEL_PROBE || kernel == KEYS_KERNEL_DENSE_PROBE || kernel == KEYS_KERNEL_PARTITION;
  if (kernel == KEYS_KERNEL_PARTITION && (n_parts < 1 || n_parts > 255)) fail(QHIP_INVALID_ARGUMENT, "partition kernel: 1 .. 255 parts");
  // the probe kernel is software-pipelined over its tiles: a row's column loads are issued one stage (load(), branch-free,
  // tile-relative addressing) before its filter / key words are computed from them (keys())
  if (raw) g.use_tile_loads(out.keys);
  std::string code, all;
  // scan filter fused into the key evaluation: a row the predicate rejects gets an invalid key, i.e. it is never
  // inserted into / probed against the join table — the filtered batch is never materialised
  check_predicate(es, predicate_root);
  if (predicate_root >= 0) {
    g.emit(predicate_root, code);
    g.set_err_gate(pass_expr(g, predicate_root));   // key expressions raise only for rows the fused scan filter passes
  }
  emit_key_words(g, es, out.keys, false, "k", code, &all);
  const std::string key_all = all;   // (the keys alone, before a fused scan filter joins in)
  const std::string pass = predicate_root >= 0 ? "(" + pass_expr(g, predicate_root) + ")" : std::string("true");
  // (the exchange's partition kernel tells "rejected by the filter" (the row is dropped) from "NULL key" (the row travels, hashed
  // as all-zero key words): bit 1 / bit 0 of what keys() returns)
  if (kernel == KEYS_KERNEL_PARTITION) all = "(" + pass + " ? 2u : 0u) | ((" + all + ") ? 1u : 0u)";
  else if (predicate_root >= 0) all = pass + " && " + all;
  std::ostringstream s;
  s << "struct P {\n  static constexpr int W = " << out.W << ";\n";
  if (raw) {
    // (dense probe: a lane owns R consecutive rows, 16 bytes of an 8-byte key column at R = 2 — and of its 4-byte narrow copy at
    // R = 4: Q3's lineitem probe 112 -> 104 us)
    bool narrow_key = false;
    for (auto& ic : input) if (ic.narrow_bytes == 4 && ic.type.id == QHIP_INT64 && !ic.indirect) narrow_key = true;
    out.probe_r = std::max(1, std::min(8, kernel == KEYS_KERNEL_DENSE_PROBE ? env_int("QHIP_DENSE_PROBE_R", narrow_key ? 4 : 2) : env_int("QHIP_PROBE_R", 4)));
    s << "  static constexpr int PROBE_R = " << out.probe_r << ";\n";
    if (kernel == KEYS_KERNEL_PARTITION)
      s << "  static constexpr int NP = " << n_parts << ";\n  static constexpr int PART_R = " << std::max(1, std::min(8, env_int("QHIP_PART_R", 4))) << ";\n";
    s << raw_loads(g);
    s << "  __device__ static __forceinline__ " << (kernel == KEYS_KERNEL_PARTITION ? "u32" : "bool") << " keys(const KArgs& a, const Raw& w, u64* k, u32& err) {\n" << code;
  } else {
    s << "  __device__ static __forceinline__ bool keys(const KArgs& a, const i64 i, u64* k, u32& err) {\n" << code;
  }
  s << "    return " << all << ";\n  }\n";
  // the sorted dense build tells a NULL key (bit 0 clear) from a row its fused scan filter rejects (bit 1 clear)
  if (kernel == KEYS_KERNEL_DENSE_BUILD)
    s << "  __device__ static __forceinline__ u32 key_state(const KArgs& a, const i64 i, u64* k, u32& err) {\n" << code
      << "    return ((" << key_all << ") ? 1u : 0u) | ((" << all << ") ? 2u : 0u);\n  }\n";
  s << "};\n";
  if (kernel == KEYS_KERNEL_PROBE) {
    const int waves = env_int("QHIP_PROBE_WAVES", out.probe_r >= 4 ? 5 : out.probe_r == 3 ? 6 : 8);
    // two entry points: the region layout of the LDS-staged build (the rule) and the one-table legacy layout. Five waves per
    // SIMD (<= 96 VGPRs): the three tiles in flight need ~90; at 98 the kernel fell to four waves and ran 10-20 % slower
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) __attribute__((amdgpu_waves_per_eu(" << waves << "))) void qk_join_probe(KArgs a, ProbeLaunch L) { qh_join_probe_body<P, true>(a, L); }\n";
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) __attribute__((amdgpu_waves_per_eu(" << waves << "))) void qk_join_probe_onetable(KArgs a, ProbeLaunch L) { qh_join_probe_body<P, false>(a, L); }\n";
  } else if (kernel == KEYS_KERNEL_DENSE_PROBE) {
    // the dense stages keep ~half the state of the hashed ones (no key words / filter masks / slot images across stages)
    const int waves = env_int("QHIP_DENSE_PROBE_WAVES", 0);   // (0: no occupancy attribute — the kernels need <= 64 VGPRs anyway, and pinning 8 waves caps the SGPRs at 80: ~30 spills)
    const std::string wattr = waves > 0 ? "__attribute__((amdgpu_waves_per_eu(" + std::to_string(waves) + "))) " : std::string();
    // qk_join_probe_dense: any table (rows r * 64 + lane, clamped per row); _wide: a lane owns R consecutive rows (16-byte
    // column loads; tables of at least one tile); _lds / _hybrid: 1 024-thread workgroups with the bitmap (its first
    // L.lds_words words) staged in LDS, wide loads
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) " << wattr << "void qk_join_probe_dense(KArgs a, ProbeLaunch L) { qh_join_probe_dense_body<P, 0, false>(a, L); }\n";
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) " << wattr << "void qk_join_probe_dense_wide(KArgs a, ProbeLaunch L) { qh_join_probe_dense_body<P, 0, true>(a, L); }\n";
    s << "extern \"C\" __global__ __launch_bounds__(1024) void qk_join_probe_dense_lds(KArgs a, ProbeLaunch L) { qh_join_probe_dense_body<P, 1, false>(a, L); }\n";
    s << "extern \"C\" __global__ __launch_bounds__(1024) void qk_join_probe_dense_hybrid(KArgs a, ProbeLaunch L) { qh_join_probe_dense_body<P, 2, false>(a, L); }\n";
  } else if (kernel == KEYS_KERNEL_PARTITION) {
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_part_ids(KArgs a, PartIdsLaunch L) { qh_part_ids_body<P, " << (dev_rows ? "true" : "false") << ", false>(a, L); }\n";
    // (tables of at least one tile: a lane owns PART_R consecutive rows — 16-byte column loads, one 4-byte store of its part bytes)
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_part_ids_wide(KArgs a, PartIdsLaunch L) { qh_part_ids_body<P, " << (dev_rows ? "true" : "false") << ", true>(a, L); }\n";
  } else if (kernel == KEYS_KERNEL_DENSE_BUILD) {
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_join_dense_build(KArgs a, DenseBuildLaunch L) { qh_join_dense_build_body<P" << (dev_rows ? ", true" : "") << ">(a, L); }\n";
    // ... and the build over strictly ascending keys (no atomics, no cleared bitmap), launched when the key is known to ascend
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_join_dense_build_sorted(KArgs a, DenseSortedLaunch L) { qh_join_dense_build_sorted_body<P" << (dev_rows ? ", true" : "") << ">(a, L); }\n";
  } else if (kernel == KEYS_KERNEL_SCATTER)
    s << "extern \"C\" __global__ __launch_bounds__(QH_SCATTER_BLOCK) void qk_join_scatter(KArgs a, ScatterLaunch L) { qh_join_scatter_body<P" << (dev_rows ? ", true" : "") << ">(a, L); }\n";
  else
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_eval_keys(KArgs a, u64* keys, u64* keyvalid, u32* status) { "
         "qh_eval_keys_body<P>(a, keys, keyvalid, status); }\n";
  out.source = s.str();
  out.kernel_name = kernel == KEYS_KERNEL_PROBE ? "qk_join_probe" : kernel == KEYS_KERNEL_SCATTER ? "qk_join_scatter" :
                    kernel == KEYS_KERNEL_DENSE_PROBE ? "qk_join_probe_dense" : kernel == KEYS_KERNEL_DENSE_BUILD ? "qk_join_dense_build" :
                    kernel == KEYS_KERNEL_PARTITION ? "qk_part_ids" : "qk_eval_keys";
  out.bind = g.bind;
}

// ---------------------------------------------------------------- exchange, pass 2
void plan_part_scatter(const std::vector<int>& widths, const std::vector<char>& indirect, int n_parts, bool dev_rows, PartScatterPlan& out, bool unstable) {
  out = PartScatterPlan();
  if (widths.empty() || widths.size() > 8) fail(QHIP_INVALID_ARGUMENT, "partition scatter: 1 .. 8 columns per launch");
  auto T = [](int w) { return w == 1 ? "u8" : w == 2 ? "u16" : (w == 4 || w == 0) ? "u32" : w == 8 ? "u64" : "qh_v4u"; };
  int maxw = 4;
  for (int w : widths) maxw = std::max(maxw, w);
  const int R = std::max(1, std::min(8, env_int("QHIP_PART_SCATTER_R", 4)));
  out.rows_per_lane = R;
  std::ostringstream s;
  // measurement switches: stores straight from the registers (no LDS staging: every lane writes its own value to its place in
  // the part's run), one tile at a time instead of the two-stage loop, the stores left out altogether (results wrong)
  const bool direct = env_int("QHIP_PART_SCATTER_DIRECT", 0) != 0, no_stores = env_int("QHIP_PART_SCATTER_NOSTORE", 0) != 0;
  const bool nt_store = env_int("QHIP_PART_SCATTER_NT", 0) != 0;
  const int tb = std::max(256, std::min(1024, env_int("QHIP_PART_SCATTER_TB", 512))) / 64 * 64;
  s << "struct P {\n  static constexpr int TB = " << tb << ";\n  static constexpr int NC = " << widths.size() << ", R = " << R << ", NPT = " << (unstable ? -1 : n_parts <= 8 ? 8 : n_parts <= 16 ? 16 : 0)
    << ", MAXW = " << maxw << ", DIRECT = " << (direct ? 1 : 0) << ", PIPE = " << (env_int("QHIP_PART_SCATTER_PIPE", 1) != 0 ? 1 : 0) << ";\n";
  s << "  struct Vals {\n";
  for (size_t c = 0; c < widths.size(); ++c) s << "    " << T(widths[c]) << " c" << c << "[R];\n";
  s << "  };\n";
  s << "  __device__ static __forceinline__ void load(const PartScatterLaunch& L, const i64 tb, const i64 last, const int lane, Vals& v) {\n";
  s << "#pragma unroll\n    for (int r = 0; r < R; ++r) {\n      i64 row = tb + r * 64 + lane;\n      row = row < last ? row : last - 1;\n";
  for (size_t c = 0; c < widths.size(); ++c) {
    const std::string t = T(widths[c]);
    if (widths[c] == 0) s << "      v.c" << c << "[r] = (u32)row;\n";
    else if (indirect[c]) s << "      v.c" << c << "[r] = ((const " << t << "*)L.src[" << c << "])[L.idx[" << c << "][row]];\n";
    else s << "      v.c" << c << "[r] = __builtin_nontemporal_load((const " << t << "*)L.src[" << c << "] + row);\n";
  }
  s << "    }\n  }\n";
  s << "  __device__ static __forceinline__ void move(const PartScatterLaunch& L, const Vals& v, const i64 tb, const u32* id, const u32* pos, const u32* dst,\n"
       "                                              const u32 total, u8* sval, const u32* sdst, const int lane) {\n";
  // every store is UNCONDITIONAL (a lane beyond the tile's rows stores the tile's last row again — same value, same address — and a
  // tile without rows stores into the launch's scratch line): a store behind a branch is one the compiler cannot count, and it
  // then waits for ALL older stores' acknowledgements before the next tile's loads (s_waitcnt vmcnt(loads only))
  if (!direct) s << "    u32 d[R], jj[R];\n#pragma unroll\n    for (int k = 0; k < R; ++k) { const u32 j = (u32)k * 64u + (u32)lane; jj[k] = j < total ? j : (total ? total - 1u : 0u); d[k] = total ? sdst[jj[k]] : (u32)lane; }\n";
  for (size_t c = 0; c < widths.size(); ++c) {
    const std::string t = T(widths[c]);
    if (direct) {
      if (!no_stores && nt_store) s << "#pragma unroll\n    for (int r = 0; r < R; ++r) if (id[r] != 0xFFu) __builtin_nontemporal_store(v.c" << c << "[r], (" << t << "*)L.out[" << c << "] + dst[r]);\n";
      else if (!no_stores) s << "#pragma unroll\n    for (int r = 0; r < R; ++r) if (id[r] != 0xFFu) ((" << t << "*)L.out[" << c << "])[dst[r]] = v.c" << c << "[r];\n";
      else s << "#pragma unroll\n    for (int r = 0; r < R; ++r) if (id[r] == 0xFEu) ((" << t << "*)L.out[" << c << "])[dst[r]] = v.c" << c << "[r];\n";
      continue;
    }
    s << "#pragma unroll\n    for (int r = 0; r < R; ++r) if (id[r] != 0xFFu) ((" << t << "*)sval)[pos[r]] = v.c" << c << "[r];\n";
    s << "    asm volatile(\"\" ::: \"memory\");\n";
    if (env_int("QHIP_PART_SCATTER_TRASH", 0))   // (measurement: every store lands in the 1 KB scratch line — the store path without HBM writes)
      s << "    { " << t << "* const o = (" << t << "*)L.trash;\n#pragma unroll\n    for (int k = 0; k < R; ++k) d[k] &= 63u;\n";
    else
    s << "    { " << t << "* const o = total ? (" << t << "*)L.out[" << c << "] : (" << t << "*)L.trash;\n";
    s << "#pragma unroll\n    for (int k = 0; k < R; ++k) { const " << t << " x = ((const " << t << "*)sval)[jj[k]]; "
      << (no_stores ? "if (lane > 64) " : "") << (nt_store ? "__builtin_nontemporal_store(x, o + d[k])" : "o[d[k]] = x") << "; } }\n";
    s << "    asm volatile(\"\" ::: \"memory\");\n";
  }
  s << "  }\n";
  // workgroup form: the tile of TB * R rows is laid out in LDS column by column and written out by all threads; every store is
  // unconditional here too (see above)
  s << "  __device__ static __forceinline__ void move_wg(const PartScatterLaunch& L, const Vals& v, const u32* id, const u32* pos, u8* sval, const u32* sdst,\n"
       "                                                 const u32* stotal, const int tid) {\n";
  s << "    u32 d[R], jj[R];\n    u32 total = 0;\n";
  for (size_t c = 0; c < widths.size(); ++c) {
    const std::string t = T(widths[c]);
    s << "#pragma unroll\n    for (int r = 0; r < R; ++r) if (id[r] != 0xFFu) ((" << t << "*)sval)[pos[r]] = v.c" << c << "[r];\n";
    s << "    __syncthreads();\n";
    if (c == 0)
      s << "    total = *stotal;\n#pragma unroll\n    for (int k = 0; k < R; ++k) { const u32 j = (u32)k * (u32)TB + (u32)tid; jj[k] = j < total ? j : (total ? total - 1u : 0u); "
           "d[k] = total ? sdst[jj[k]] : (u32)(tid & 63); }\n";
    s << "    { " << t << "* const o = total ? (" << t << "*)L.out[" << c << "] : (" << t << "*)L.trash;\n";
    s << "#pragma unroll\n    for (int k = 0; k < R; ++k) { const " << t << " x = ((const " << t << "*)sval)[jj[k]]; "
      << (no_stores ? "if (tid > 4096) " : "") << (nt_store ? "__builtin_nontemporal_store(x, o + d[k])" : "o[d[k]] = x") << "; } }\n";
    s << "    __syncthreads();\n";
  }
  s << "  }\n};\n";
  s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_part_scatter(PartScatterLaunch L) { qh_part_scatter_body<P" << (dev_rows ? ", true" : "")
    << ">(L); }\n";
  s << "extern \"C\" __global__ __launch_bounds__(" << tb << ") void qk_part_scatter_wg(PartScatterLaunch L) { qh_part_scatter_wg_body<P" << (dev_rows ? ", true" : "")
    << ">(L); }\n";
  out.wg_threads = tb;
  out.source = s.str();
  out.kernel_name = "qk_part_scatter";
}

// ---------------------------------------------------------------- projection
void plan_projection(const ExprSet& es, const std::vector<InputCol>& input, const int32_t* roots, int n, ProjectionPlan& out) {
  out = ProjectionPlan();
  if (n > 24) fail(QHIP_UNSUPPORTED, "more than 24 computed projection expressions");
  ExprGen g(es, input);
  std::ostringstream body;
  for (int k = 0; k < n; ++k) {
    const ENode& nd = es.at(roots[k]);
    ProjOutDesc od;
    od.root = roots[k]; od.type = nd.type; od.nullable = nd.nullable;
    std::string code;
    g.emit(od.root, code);
    body << code;
    const std::string okx = g.ok(od.root);
    if (nd.type.id == QHIP_NULL)
      fail(QHIP_UNSUPPORTED, "projection of a computed " + dtype_name(nd.type) + " expression is not accelerated");
    if (nd.type.id == QHIP_UTF8) {
      // a computed string (CASE over literals / columns, a literal): pass 0 stores its length, the host scans the lengths into
      // offsets, pass 1 copies the bytes (both passes evaluate the same generated code)
      out.has_utf8 = true;
      const std::string lenx = std::string(od.nullable ? "(" + okx + " ? " : "(") + g.len(od.root) + (od.nullable ? " : 0)" : ")");
      body << "    if (MODE == 0 && inb) ((int*)o.v[" << k << "])[row] = " << lenx << ";\n";
      body << "    if (MODE == 1 && inb" << (od.nullable ? " && " + okx : std::string("")) << ") { u8* dst = o.d[" << k << "] + ((const int*)o.v[" << k
           << "])[row]; const u8* src = " << g.ptr(od.root) << "; const int nb = " << g.len(od.root) << "; for (int b = 0; b < nb; ++b) dst[b] = src[b]; }\n";
    } else if (nd.type.id == QHIP_BOOL) {
      body << "    if (MODE == 0) { const u64 m = qh_ballot(inb && " << (od.nullable ? okx + " && " : std::string("")) << g.val(od.root) << "); if (lane == 0) ((u64*)o.v[" << k
           << "])[j] = m; }\n";
    } else {
      const std::string T = ExprGen::ctype(nd.type);
      body << "    if (MODE == 0 && inb) ((" << T << "*)o.v[" << k << "])[row] = " << (od.nullable ? okx + " ? " : std::string("")) << g.val(od.root)
           << (od.nullable ? " : (" + T + ")0" : std::string("")) << ";\n";
    }
    if (od.nullable) body << "    if (MODE == 0) { const u64 m = qh_ballot(inb && " << okx << "); if (lane == 0) o.n[" << k << "][j] = m; }\n";
    out.outs.push_back(od);
  }
  std::ostringstream s;
  s << "struct P {\n";
  s << "  template <int MODE> __device__ static __forceinline__ void row(const KArgs& a, const ProjOut& o, const i64 i, const i64 row, const bool inb, const i64 j, "
       "const int lane, u32& err) {\n" << body.str() << "  }\n};\n";
  s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_project(KArgs a, ProjOut o, u32* status) { qh_project_body<P, 0>(a, o, status); }\n";
  if (out.has_utf8)
    s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_project_copy(KArgs a, ProjOut o, u32* status) { qh_project_body<P, 1>(a, o, status); }\n";
  out.source = s.str();
  out.kernel_name = "qk_project";
  out.bind = g.bind;
}

// ---------------------------------------------------------------- sort key images
void plan_sort_keys(const ExprSet& es, const std::vector<InputCol>& input, const int32_t* roots, int n, SortKeysPlan& out) {
  out = SortKeysPlan();
  if (n > 32) fail(QHIP_UNSUPPORTED, "more than 32 sort keys");
  ExprGen g(es, input);
  std::ostringstream body;
  int off = 0;
  for (int k = 0; k < n; ++k) {
    const ENode& nd = es.at(roots[k]);
    SortKeyDesc kd;
    kd.root = roots[k]; kd.type = nd.type; kd.nullable = nd.nullable; kd.word_off = off; kd.words = 1; kd.top_bits = 64; kd.column = -1;
    std::string code;
    g.emit(kd.root, code);
    body << code;
    const std::string v = g.val(kd.root), okx = g.ok(kd.root);
    auto store = [&](int w, const std::string& image) {
      body << "    img[" << off + w << "] = " << (kd.nullable ? okx + " ? " : std::string("")) << image << (kd.nullable ? " : 0ULL" : "") << ";\n";
    };
    const DType& t = nd.type;
    if (t.id == QHIP_UTF8) {
      if (nd.kind != QHIP_EXPR_COLUMN) fail(QHIP_UNSUPPORTED, "ORDER BY on a computed Utf8 expression is not accelerated");
      kd.words = 0; kd.top_bits = 0; kd.column = nd.column;
    } else if (t.id == QHIP_DECIMAL128) {
      kd.words = 2;
      store(0, "(u64)(u128)" + v);
      store(1, "((u64)((u128)" + v + " >> 64) ^ 0x8000000000000000ULL)");
    } else if (t.id == QHIP_BOOL) {
      kd.top_bits = 1;
      store(0, "(" + v + " ? 1ULL : 0ULL)");
    } else if (dtype_is_float(t)) {
      store(0, "qh_f64_ord((double)" + v + ")");
    } else if (intlike(t)) {
      const int b = dtype_width(t) * 8;
      kd.top_bits = b;
      if (signed_intlike(t)) {
        if (b == 64) store(0, "((u64)(i64)" + v + " ^ 0x8000000000000000ULL)");
        else store(0, "(((u64)(i64)" + v + " + " + std::to_string(1ULL << (b - 1)) + "ULL) & " + std::to_string((1ULL << b) - 1) + "ULL)");
      } else {
        store(0, "(u64)" + v);
      }
    } else if (t.id == QHIP_NULL) {
      kd.top_bits = 1;
      store(0, "0ULL");
    } else {
      fail(QHIP_UNSUPPORTED, "ORDER BY on " + dtype_name(t) + " is not supported");
    }
    if (kd.nullable) body << "    valid |= " << okx << " ? " << (1u << k) << "u : 0u;\n";
    else body << "    valid |= " << (1u << k) << "u;\n";
    off += kd.words;
    out.keys.push_back(kd);
  }
  out.NW = off;
  std::ostringstream s;
  s << "struct P {\n  static constexpr int NW = " << out.NW << ";\n  static constexpr int NK = " << n << ";\n";
  s << "  __device__ static __forceinline__ void images(const KArgs& a, const i64 i, u64* img, u32& valid, u32& err) {\n" << body.str() << "  }\n};\n";
  s << "extern \"C\" __global__ __launch_bounds__(QH_BLOCK) void qk_sort_keys(KArgs a, u64* img, u64* keyvalid, u64* diff, u32* status) { "
       "qh_sort_keys_body<P>(a, img, keyvalid, diff, status); }\n";
  out.source = s.str();
  out.kernel_name = "qk_sort_keys";
  out.bind = g.bind;
}

}  // namespace qhip
