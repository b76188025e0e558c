// agg_result.cpp — the hash aggregate's host-side result logic (agg_result.hpp). No HIP runtime call, no Ctx.
//
// Reference: physical/plan/aggregate/hash.rs:89-107 (GroupAccumulator::output); accumulators physical/expr/aggregate/*.rs.
#include "agg_result.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <map>

namespace qhip {

// ---------------------------------------------------------------- HostColumn
void HostColumn::init_fixed(const DType& t, int64_t n) {
  type = t; length = n; null_count = 0;
  const int w = dtype_width(t);
  if (w) values.assign((size_t)n * w, 0);
  else if (t.id == QHIP_BOOL) values.assign((size_t)((n + 7) / 8), 0);
  else if (t.id == QHIP_UTF8) offsets.assign((size_t)n + 1, 0);
}
void HostColumn::set_null(int64_t i) {
  if (validity.empty()) validity.assign((size_t)((length + 7) / 8), 0xff);
  validity[(size_t)(i >> 3)] &= (uint8_t)~(1u << (i & 7));
  ++null_count;
}

double ord_to_f64(uint64_t k) {
  uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
  double d; memcpy(&d, &b, 8); return d;
}

// MIN / MAX over these types compares as signed integers (F_MM_INT's is_signed, the host assembly's un-biasing)
static bool minmax_is_signed(const DType& t) {
  return dtype_is_signed(t) || t.id == QHIP_DATE32 || t.id == QHIP_DATE64 || (t.id >= QHIP_TIME32_S && t.id <= QHIP_TIMESTAMP_NS);
}

// ---------------------------------------------------------------- replica merge
uint32_t merge_replica_slots(const AggPlan& plan, std::vector<uint64_t>& slots, uint32_t G) {
  // same key words -> one slot; every cell is a commutative monoid (wrapping adds, max)
  std::map<std::vector<uint64_t>, uint32_t> seen;   // only consulted once there are many distinct keys
  uint32_t out = 0;
  for (uint32_t g = 0; g < G; ++g) {
    uint64_t* src = &slots[(size_t)g * plan.slot_words];
    uint32_t found = out;
    if (out <= 16) {
      for (uint32_t k = 0; k < out; ++k)
        if (!memcmp(&slots[(size_t)k * plan.slot_words + 1], src + 1, (size_t)plan.W * 8)) { found = k; break; }
      if (found == out && out == 16)   // growing past the linear-search regime: index what we have
        for (uint32_t k = 0; k < out; ++k) {
          const uint64_t* ks = &slots[(size_t)k * plan.slot_words + 1];
          seen.emplace(std::vector<uint64_t>(ks, ks + plan.W), k);
        }
    } else {
      auto it = seen.find(std::vector<uint64_t>(src + 1, src + 1 + plan.W));
      if (it != seen.end()) found = it->second;
    }
    if (found == out) {
      if (out >= 16) seen.emplace(std::vector<uint64_t>(src + 1, src + 1 + plan.W), out);
      if (out != g) memcpy(&slots[(size_t)out * plan.slot_words], src, (size_t)plan.slot_words * 8);
      ++out;
      continue;
    }
    uint64_t* dst = &slots[(size_t)found * plan.slot_words] + 1 + plan.W;
    const uint64_t* sc = src + 1 + plan.W;
    for (auto& cd : plan.cells) {
      switch (cd.kind) {
        case CELL_ROWS: case CELL_CNT: case CELL_SUM_U64: dst[cd.off] += sc[cd.off]; break;
        case CELL_SUM_I128: {
          const u128 a = ((u128)dst[cd.off + 1] << 64) | dst[cd.off], b2 = ((u128)sc[cd.off + 1] << 64) | sc[cd.off], r = a + b2;
          dst[cd.off] = (uint64_t)r; dst[cd.off + 1] = (uint64_t)(r >> 64);
          break;
        }
        case CELL_SUM_F64: { double x, y; memcpy(&x, &dst[cd.off], 8); memcpy(&y, &sc[cd.off], 8); x += y; memcpy(&dst[cd.off], &x, 8); break; }
        case CELL_MAXORD64: dst[cd.off] = std::max(dst[cd.off], sc[cd.off]); break;
        case CELL_MAXORD128: {
          const u128 a = ((u128)dst[cd.off + 1] << 64) | dst[cd.off], b2 = ((u128)sc[cd.off + 1] << 64) | sc[cd.off];
          if (b2 > a) { dst[cd.off] = sc[cd.off]; dst[cd.off + 1] = sc[cd.off + 1]; }
          break;
        }
      }
    }
  }
  slots.resize((size_t)out * plan.slot_words);
  return out;
}

// ---------------------------------------------------------------- slots -> columns (GroupAccumulator::output, hash.rs:89-107; accumulator evaluate())
static void assemble_key_column(const AggPlan& plan, const std::vector<uint64_t>& slots, uint32_t G, int k, HostColumn& hc) {
  const KeyDesc& kd = plan.keys[(size_t)k];
  hc.init_fixed(kd.type, G);
  for (uint32_t g = 0; g < G; ++g) {
    const uint64_t* slot = &slots[(size_t)g * plan.slot_words];
    const bool is_null = plan.null_mask_word && ((slot[1] >> k) & 1);
    const uint64_t w0 = slot[1 + kd.word_off];
    if (kd.type.id == QHIP_UTF8) {
      const uint64_t* kw = slot + 1 + kd.word_off;
      const int len = is_null ? 0 : (int)(kw[kd.words - 1] >> 56);
      for (int b = 0; b < len; ++b) hc.data.push_back((uint8_t)(kw[b >> 3] >> (8 * (b & 7))));
      hc.offsets[(size_t)g + 1] = (int32_t)hc.data.size();
    } else if (kd.type.id == QHIP_DECIMAL128) {
      hc.as<uint64_t>()[2 * (size_t)g] = w0;
      hc.as<uint64_t>()[2 * (size_t)g + 1] = slot[1 + kd.word_off + 1];
    } else {
      const int w = dtype_width(kd.type);
      memcpy(hc.values.data() + (size_t)g * w, &w0, (size_t)w);   // little-endian truncation of the sign-extended word
    }
    if (is_null) hc.set_null(g);
  }
}

// avg.rs:91-116 (DecimalAvgAccumulator::evaluate)
static i128 decimal_avg(const AggPlan& plan, const AggDesc& ad, const uint64_t* vc, uint64_t nonnull) {
  const DType& at = plan.args[(size_t)ad.arg].type;
  const i128 sum = (i128)(((u128)vc[1] << 64) | (u128)vc[0]);
  if (ad.ret.scale < at.scale) fail(QHIP_EXEC_ERROR, "Internal error: Arithmetic Overflow in DecimalAvgAccumulator");
  const i128 mul = pow10_i128(ad.ret.scale - at.scale);
  i128 value;
  if (__builtin_mul_overflow(sum, mul, &value)) fail(QHIP_EXEC_ERROR, "AVG(Decimal128): sum * 10^k overflows i128 (reference yields a mistyped NULL, avg.rs:105-116)");
  const i128 lim = pow10_i128(ad.ret.precision);
  if (value >= lim || value <= -lim)
    fail(QHIP_EXEC_ERROR, "AVG(Decimal128): scaled sum exceeds " + dtype_name(ad.ret) + " (reference yields a mistyped NULL, avg.rs:105-116)");
  return value / (i128)nonnull;   // truncating, like i128::div_wrapping
}

// PrimitiveAccumulator (aggregate/mod.rs:28-84): seeded with NATIVE::MAX / MIN, Some() as soon as accumulate ran once — i.e. for
// every existing group, and for NoGrouping whenever a batch arrived. vc = the group's MAXORD cell (MIN: the complement's maximum).
static void store_min_max(const DType& t, bool is_min, const uint64_t* vc, uint32_t g, HostColumn& hc) {
  if (t.id == QHIP_DECIMAL128) {
    u128 o = ((u128)vc[1] << 64) | (u128)vc[0];
    if (is_min) o = ~o;
    const u128 v = o ^ ((u128)1 << 127);
    hc.as<uint64_t>()[2 * (size_t)g] = (uint64_t)v;
    hc.as<uint64_t>()[2 * (size_t)g + 1] = (uint64_t)(v >> 64);
  } else if (dtype_is_float(t)) {
    uint64_t o = is_min ? ~vc[0] : vc[0];
    double v = (vc[0] == 0) ? (is_min ? DBL_MAX : -DBL_MAX) : ord_to_f64(o);
    if (t.id == QHIP_FLOAT32) {
      const float lim = FLT_MAX;
      float fv = (float)v;
      if (vc[0] == 0 || std::isnan(fv)) fv = is_min ? lim : -lim;
      if (is_min && fv > lim) fv = lim;
      if (!is_min && fv < -lim) fv = -lim;
      hc.as<float>()[g] = fv;
    } else {
      if (std::isnan(v)) v = is_min ? DBL_MAX : -DBL_MAX;
      if (is_min && v > DBL_MAX) v = DBL_MAX;
      if (!is_min && v < -DBL_MAX) v = -DBL_MAX;
      hc.as<double>()[g] = v;
    }
  } else {
    uint64_t o = is_min ? ~vc[0] : vc[0];
    const bool sgn = minmax_is_signed(t);
    uint64_t raw = sgn ? (o ^ 0x8000000000000000ULL) : o;
    const int w = dtype_width(t);
    // no non-null value seen (an all-zero cell): the seed of the column's OWN type (i32::MAX, not i64::MAX truncated)
    if (vc[0] == 0 && sgn && w < 8) raw = is_min ? ((1ULL << (8 * w - 1)) - 1) : (1ULL << (8 * w - 1));
    memcpy(hc.values.data() + (size_t)g * w, &raw, (size_t)w);
  }
}

std::vector<HostColumn> assemble_host_columns(const AggPlan& plan, const std::vector<uint64_t>& slots, uint32_t G, int n_groups, int n_aggs,
                                              bool zero_batches_in) {
  const int cell0 = 1 + plan.W;
  std::vector<HostColumn> cols((size_t)(n_groups + n_aggs));
  for (int k = 0; k < n_groups; ++k) assemble_key_column(plan, slots, G, k, cols[(size_t)k]);
  for (int k = 0; k < n_aggs; ++k) {
    const AggDesc& ad = plan.aggs[(size_t)k];
    HostColumn& hc = cols[(size_t)(n_groups + k)];
    hc.init_fixed(ad.ret, G);
    for (uint32_t g = 0; g < G; ++g) {
      const uint64_t* cell = &slots[(size_t)g * plan.slot_words + cell0];
      const uint64_t nonnull = cell[plan.cells[(size_t)ad.count_cell].off];
      const uint64_t* vc = ad.value_cell >= 0 ? cell + plan.cells[(size_t)ad.value_cell].off : nullptr;
      switch (ad.kind) {
        case QHIP_AGG_COUNT:   // count.rs:36-48
          hc.as<int64_t>()[g] = (int64_t)nonnull;
          break;
        case QHIP_AGG_SUM:     // sum.rs:71-103: None until a non-null value was seen
          if (!nonnull) { hc.set_null(g); break; }
          if (ad.ret.id == QHIP_DECIMAL128) { hc.as<uint64_t>()[2 * (size_t)g] = vc[0]; hc.as<uint64_t>()[2 * (size_t)g + 1] = vc[1]; }
          else hc.as<uint64_t>()[g] = vc[0];   // Int64 / UInt64 wrapping sum, Float64 bit pattern
          break;
        case QHIP_AGG_AVG: {
          if (!nonnull) { hc.set_null(g); break; }
          if (ad.ret.id == QHIP_FLOAT64) {   // avg.rs:63-78
            double s; memcpy(&s, vc, 8);
            hc.as<double>()[g] = s / (double)nonnull;
            break;
          }
          const i128 q = decimal_avg(plan, ad, vc, nonnull);
          hc.as<uint64_t>()[2 * (size_t)g] = (uint64_t)(u128)q;
          hc.as<uint64_t>()[2 * (size_t)g + 1] = (uint64_t)((u128)q >> 64);
          break;
        }
        case QHIP_AGG_MIN:
        case QHIP_AGG_MAX:
          if (plan.W == 0 && zero_batches_in) { hc.set_null(g); break; }
          store_min_max(ad.ret, ad.kind == QHIP_AGG_MIN, vc, g, hc);
          break;
      }
    }
  }
  return cols;
}

// ---------------------------------------------------------------- k_agg_finalize's column descriptors
std::vector<FinCol> describe_fin_cols(const AggPlan& plan, int n_groups, int n_aggs) {
  const int cell0 = 1 + plan.W;
  std::vector<FinCol> fc((size_t)(n_groups + n_aggs));
  for (int k = 0; k < n_groups + n_aggs; ++k) {
    FinCol& f = fc[(size_t)k];
    memset(&f, 0, sizeof f);
    f.cnt_word = -1; f.key_index = -1; f.src_word = 0;
    if (k < n_groups) {
      const KeyDesc& kd = plan.keys[(size_t)k];
      f.src_word = 1 + kd.word_off;
      f.key_index = (plan.null_mask_word && kd.nullable) ? k : -1;
      if (kd.type.id == QHIP_UTF8) { f.kind = F_KEY_UTF8_LEN; f.width = 4; f.pad = kd.words; }
      else if (kd.type.id == QHIP_DECIMAL128) { f.kind = F_KEY_DEC; f.width = 16; }
      else { f.kind = F_KEY_FIXED; f.width = dtype_width(kd.type); }
      continue;
    }
    const AggDesc& ad = plan.aggs[(size_t)(k - n_groups)];
    const int cntw = cell0 + plan.cells[(size_t)ad.count_cell].off;
    f.src_word = ad.value_cell >= 0 ? cell0 + plan.cells[(size_t)ad.value_cell].off : 0;
    f.width = dtype_width(ad.ret);
    switch (ad.kind) {
      case QHIP_AGG_COUNT: f.kind = F_COUNT; f.cnt_word = cntw; f.width = 8; break;
      case QHIP_AGG_SUM: f.kind = ad.ret.id == QHIP_DECIMAL128 ? F_SUM128 : F_SUM64; f.cnt_word = cntw; break;
      case QHIP_AGG_AVG:
        f.cnt_word = cntw;
        if (ad.ret.id == QHIP_FLOAT64) f.kind = F_AVG_F64;
        else {
          const DType& at = plan.args[(size_t)ad.arg].type;
          if (ad.ret.scale < at.scale) fail(QHIP_EXEC_ERROR, "Internal error: Arithmetic Overflow in DecimalAvgAccumulator");
          const i128 mul = pow10_i128(ad.ret.scale - at.scale), lim = pow10_i128(ad.ret.precision);
          f.kind = F_AVG_DEC;
          f.mul_lo = (uint64_t)(u128)mul; f.mul_hi = (uint64_t)((u128)mul >> 64);
          f.lim_lo = (uint64_t)(u128)lim; f.lim_hi = (uint64_t)((u128)lim >> 64);
        }
        break;
      default:
        f.is_min = ad.kind == QHIP_AGG_MIN;
        if (ad.ret.id == QHIP_DECIMAL128) f.kind = F_MM_DEC;
        else if (ad.ret.id == QHIP_FLOAT64) f.kind = F_MM_F64;
        else if (ad.ret.id == QHIP_FLOAT32) f.kind = F_MM_F32;
        else { f.kind = F_MM_INT; f.is_signed = minmax_is_signed(ad.ret); }
    }
  }
  return fc;
}

}  // namespace qhip
