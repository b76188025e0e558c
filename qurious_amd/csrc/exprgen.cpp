// exprgen.cpp — ExprGen: the statements that compute one expression node for the current row (declared in codegen.hpp).
// emit() dispatches on the node kind to one private member each. A member first emits the node's children (in a fixed
// order: column and literal slots are numbered in the order they are first met, and the slot numbers are part of the text)
// and then appends its own statements: `vK` the value of node K, `nK` its validity, `pK` / `lK` pointer and length of a string.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "codegen.hpp"
#include "device/qhip_status.h"

namespace qhip {

static bool is_cmp(int op) { return op >= QHIP_OP_EQ && op <= QHIP_OP_LTEQ; }
static const char* c_cmp(int op) {   // (qhip_operator order: EQ, NOTEQ, GT, GTEQ, LT, LTEQ)
  static const char* const s[] = {"==", "!=", ">", ">=", "<", "<="};
  return is_cmp(op) ? s[op - QHIP_OP_EQ] : "==";
}

std::string ExprGen::ctype(const DType& t) {
  switch (t.id) {
    case QHIP_BOOL: return "bool";
    case QHIP_INT8: return "signed char";
    case QHIP_INT16: return "short";
    case QHIP_INT32: case QHIP_DATE32: case QHIP_TIME32_S: case QHIP_TIME32_MS: return "int";
    case QHIP_INT64: case QHIP_DATE64: case QHIP_TIME64_US: case QHIP_TIME64_NS:
    case QHIP_TIMESTAMP_S: case QHIP_TIMESTAMP_MS: case QHIP_TIMESTAMP_US: case QHIP_TIMESTAMP_NS: return "i64";
    case QHIP_UINT8: return "u8";
    case QHIP_UINT16: return "u16";
    case QHIP_UINT32: return "u32";
    case QHIP_UINT64: return "u64";
    case QHIP_FLOAT32: return "float";
    case QHIP_FLOAT64: return "double";
    case QHIP_DECIMAL128: return "i128";
    default: return "int";
  }
}

std::string ExprGen::i128_const(i128 v) {
  char buf[96];
  snprintf(buf, sizeof buf, "qh_mk128(0x%llxULL, (i64)0x%llxULL)", (unsigned long long)(uint64_t)(u128)v,
           (unsigned long long)(uint64_t)((u128)v >> 64));
  return buf;
}

// (Time32 / Time64 are signed integers as far as key words, MIN / MAX images and sort keys go; the typing in expr.cpp keeps
// arithmetic and casts away from them)
// (... and so are the Timestamp types, which are not hash keys at all: check_key_type)
static bool timelike(const DType& t) { return t.id >= QHIP_TIME32_S && t.id <= QHIP_TIMESTAMP_NS; }
bool intlike(const DType& t) { return (t.id >= QHIP_INT8 && t.id <= QHIP_UINT64) || t.id == QHIP_DATE32 || t.id == QHIP_DATE64 || timelike(t); }
bool signed_intlike(const DType& t) { return (t.id >= QHIP_INT8 && t.id <= QHIP_INT64) || t.id == QHIP_DATE32 || t.id == QHIP_DATE64 || timelike(t); }
// the least / greatest value of an intlike type as a C literal, by its width in bytes (1, 2, 4, 8) and signedness
static std::string int_min(const DType& t) {
  static const char* const s[] = {"(-128)", "(-32768)", "(-2147483647-1)", "(-9223372036854775807LL-1)"};
  return signed_intlike(t) ? s[log2u((uint32_t)dtype_width(t))] : "0";
}
static std::string int_max(const DType& t) {
  static const char* const s[] = {"127", "32767", "2147483647", "9223372036854775807LL"}, *const u[] = {"255", "65535", "4294967295U", "18446744073709551615ULL"};
  return !intlike(t) ? "0" : (signed_intlike(t) ? s : u)[log2u((uint32_t)dtype_width(t))];
}
// unsigned type wide enough for wrapping arithmetic on t
static std::string wrap_type(const DType& t) { return dtype_width(t) == 8 ? "u64" : "u32"; }

ExprGen::ExprGen(const ExprSet& es, const std::vector<InputCol>& in) : es_(es), in_(in), done_(es.nodes.size(), false) {
  bind.stroff.push_back(0);
  // Column values and Utf8 offsets are read exactly once by every generated kernel: streaming (non-temporal) loads, which
  // on MI355X read ~10 % faster than plain ones (7.0 vs 6.3 TB/s, tools/stream_sweep.py) and keep the L2 for the tables
  // the kernels access at random. QHIP_NO_NT=1 switches them off (A/B measurements).
  nt_ = getenv("QHIP_NO_NT") == nullptr;
}

void ExprGen::use_tile_loads(const std::vector<KeyDesc>& keys) {
  set_indexing(" + tb", "o", "(tb + (i64)o)");
  set_raw_mode(true);
  for (auto& kd : keys)
    if (kd.type.id == QHIP_UTF8 && es_.at(kd.root).kind == QHIP_EXPR_COLUMN) mark_utf8_key(kd.root, kd.words);
}

// the statement that raises status bit(s) `bits`: under the gate, if one is set (codegen.hpp: set_err_gate)
std::string ExprGen::raise(unsigned bits) {
  raises_ = true;
  const std::string st = "err |= " + std::to_string(bits) + "u;";
  return gate_.empty() ? st : "{ if (" + gate_ + ") " + st + " }";
}

std::string ExprGen::ok(int k) const { return es_.at(k).nullable ? "n" + std::to_string(k) : "true"; }

int ExprGen::col_slot(int table_col) {
  for (size_t s = 0; s < bind.cols.size(); ++s) if (bind.cols[s] == table_col) return (int)s;
  if (bind.cols.size() >= 24) fail(QHIP_UNSUPPORTED, "expression references more than 24 distinct columns");
  bind.cols.push_back(table_col);
  bind.indirect.push_back(table_col >= 0 && table_col < (int)in_.size() && in_[(size_t)table_col].indirect ? 1 : 0);
  bind.narrow.push_back(table_col >= 0 && table_col < (int)in_.size() ? (char)in_[(size_t)table_col].narrow_bytes : (char)0);
  bind.rec.push_back(table_col >= 0 && table_col < (int)in_.size() ? (char)in_[(size_t)table_col].rec_stride : (char)0);
  return (int)bind.cols.size() - 1;
}

int ExprGen::lit_slot(const ENode& n) {
  if (bind.lit_lo.size() >= 24) fail(QHIP_UNSUPPORTED, "more than 24 literals in one kernel");
  uint64_t lo = n.lo; int64_t hi = n.hi;
  if (n.type.id == QHIP_FLOAT64 || n.type.id == QHIP_FLOAT32) { double f = n.f; memcpy(&lo, &f, 8); hi = 0; }
  if (n.type.id == QHIP_UTF8) {   // the first 8 bytes as a kernel scalar: `col = 'BUILDING'` is one masked word compare (qh_streq_lit)
    lo = 0; hi = 0;
    memcpy(&lo, n.s.data(), std::min<size_t>(8, n.s.size()));
  }
  bind.lit_lo.push_back(lo);
  bind.lit_hi.push_back(hi);
  if (n.type.id == QHIP_UTF8) bind.strlits += n.s;
  bind.stroff.push_back((int)bind.strlits.size());
  return (int)bind.lit_lo.size() - 1;
}

int ExprGen::str_slot(const std::string& bytes) {
  if (bind.lit_lo.size() >= 24) fail(QHIP_UNSUPPORTED, "more than 24 literals in one kernel");
  bind.lit_lo.push_back(0);
  bind.lit_hi.push_back(0);
  bind.strlits += bytes;
  bind.stroff.push_back((int)bind.strlits.size());
  return (int)bind.lit_lo.size() - 1;
}

void ExprGen::emit(int k, std::string& out) {
  if (done_[(size_t)k]) return;
  const ENode& n = es_.at(k);
  std::ostringstream o;
  switch (n.kind) {
    case QHIP_EXPR_COLUMN: emit_column(k, n, o); break;
    case QHIP_EXPR_LITERAL: emit_literal(k, n, o); break;
    case QHIP_EXPR_BINARY: emit_binary(k, n, out, o); break;
    case QHIP_EXPR_CAST: emit_cast(k, n, out, o); break;
    case QHIP_EXPR_IS_NULL:
    case QHIP_EXPR_IS_NOT_NULL:
      emit(n.left, out);
      o << "    const bool " << val(k) << " = " << (n.kind == QHIP_EXPR_IS_NULL ? "!" : "") << "(" << ok(n.left) << ");\n";
      break;
    case QHIP_EXPR_IF: emit_if(k, n, out, o); break;
    case QHIP_EXPR_LIKE: emit_like(k, n, out, o); break;
    case QHIP_EXPR_FUNCTION: emit_function(k, n, out, o); break;
    case QHIP_EXPR_NEGATIVE: emit_negative(k, n, out, o); break;
  }
  out += o.str();
  done_[(size_t)k] = true;
}

// `ld` receives the loads; in raw mode they go to load_code (fields of `Raw w`) and only aliases are emitted into `o`
void ExprGen::emit_column(int k, const ENode& n, std::ostringstream& o) {
  const std::string K = std::to_string(k), v = "v" + K, nn = "n" + K, S = std::to_string(col_slot(n.column));
  std::ostringstream ld;
  const std::string W = raw_ ? "w." : "";
  if (n.type.id == QHIP_UTF8) {
    emit_utf8_column(k, n, S, ld, o);
  } else if (n.type.id == QHIP_BOOL) {
    raw_field("bool", v);
    ld << "    " << (raw_ ? "" : "const bool ") << W << v << " = qh_bit((const u8*)a.c[" << S << "].v, " << row_ << ");\n";
    if (raw_) o << "    const bool " << v << " = w." << v << ";\n";
  } else if (n.type.id == QHIP_NULL) {
    o << "    const int " << v << " = 0;\n";
  } else {
    emit_value_column(k, n, S, ld, o);
  }
  if (n.nullable) {
    if (n.type.id == QHIP_NULL) o << "    const bool " << nn << " = false;\n";
    else {
      raw_field("bool", nn);
      ld << "    " << (raw_ ? "" : "const bool ") << W << nn << " = qh_bit(a.c[" << S << "].n, " << row_ << ");\n";
      if (raw_) o << "    const bool " << nn << " = w." << nn << ";\n";
    }
  }
  if (raw_) load_code += ld.str(); else o << ld.str();
}

void ExprGen::emit_utf8_column(int k, const ENode& n, const std::string& S, std::ostringstream& ld, std::ostringstream& o) {
  const std::string K = std::to_string(k), W = raw_ ? "w." : "";
  raw_field("int", "b" + K); raw_field("int", "l" + K);
  if (in_[(size_t)n.column].utf8_fixed1) {
    // every value is exactly one byte: offsets[i] == i, no offset loads, the data byte is addressed by row number
    ld << "    " << (raw_ ? "" : "const int ") << W << "b" << K << " = (int)(" << row_ << ");\n";
    ld << "    " << (raw_ ? "" : "const int ") << W << "l" << K << " = 1;\n";
  } else {
    const std::string o0 = "((const int*)a.c[" + S + "].v" + base_ + ")[" + idx_ + "]", o1 = "((const int*)a.c[" + S + "].v" + base_ + ")[" + idx_ + " + 1]";
    ld << "    " << (raw_ ? "" : "const int ") << W << "b" << K << " = " << (nt_ ? "__builtin_nontemporal_load(&" + o0 + ")" : o0) << ";\n";
    ld << "    " << (raw_ ? "" : "const int ") << W << "l" << K << " = " << (nt_ ? "__builtin_nontemporal_load(&" + o1 + ")" : o1) << " - " << W << "b" << K << ";\n";
  }
  if (!raw_) { ld << "    const u8* p" << K << " = a.c[" << S << "].d + b" << K << ";\n"; return; }
  auto it = utf8_key_words_.find(k);
  if (it != utf8_key_words_.end()) {
    raw_field("u64", "k" + K + "[" + std::to_string(it->second) + "]");
    // key bytes: 8 at a time — or just as many as the column's longest value has (Q1's flags are 1 byte: a 1-byte
    // load per row instead of 64 overlapping 8-byte windows per wavefront)
    const int maxlen = in_[(size_t)n.column].utf8_max_len;
    for (int w2 = 0; w2 < it->second; ++w2) {
      // (one-byte values: addressed by the 64-bit row, so that a lane's consecutive rows are provably adjacent bytes)
      const std::string at = in_[(size_t)n.column].utf8_fixed1 ? "(a.c[" + S + "].d + " + row_ + " + " + std::to_string(8 * w2) + ")"
                                                               : "(a.c[" + S + "].d + w.b" + K + " + " + std::to_string(8 * w2) + ")";
      const int left = maxlen >= 0 ? maxlen - 8 * w2 : 8;
      if (it->second == 1 && left <= 1) ld << "    w.k" << K << "[0] = (u64)" << (nt_ ? "__builtin_nontemporal_load((const u8*)" + at + ")" : "*(const u8*)" + at) << ";\n";
      else if (it->second == 1 && left <= 2) ld << "    w.k" << K << "[0] = (u64)*(const qh_u16_unaligned*)" << at << ";\n";
      else if (it->second == 1 && left <= 4) ld << "    w.k" << K << "[0] = (u64)*(const qh_u32_unaligned*)" << at << ";\n";
      else ld << "    w.k" << K << "[" << w2 << "] = *(const qh_u64_unaligned*)" << at << ";\n";
    }
  }
  o << "    const int l" << K << " = w.l" << K << "; const u8* p" << K << " = a.c[" << S << "].d + w.b" << K << ";\n";
}

// a fixed-width value
void ExprGen::emit_value_column(int k, const ENode& n, const std::string& S, std::ostringstream& ld, std::ostringstream& o) {
  const std::string v = val(k);
  const InputCol& ic = in_[(size_t)n.column];
  // a Decimal128 column with a narrow copy (InputCol::narrow_bytes): the kernel loads 4 / 8 bytes per value and widens
  // (an indirect column — read through an index vector — gathers from its SOURCE's narrow copy: ColRange::narrow_buf)
  const int nb = (n.type.id == QHIP_DECIMAL128 || (n.type.id == QHIP_INT64 && ic.narrow_bytes == 4)) ? ic.narrow_bytes : 0;
  const std::string T = nb == 4 ? "int" : nb == 8 ? "i64" : ctype(n.type);   // the type in memory
  raw_field(T, v);
  // streaming (non-temporal) loads when asked for: column values are read once; Decimal128 goes through a 4 x u32
  // vector (the builtin takes integer / float / vector types)
  // tile-relative indexing (uniform 64-bit tile base + 32-bit lane offset): the lane offset is turned into BYTES in 32
  // bits, so that the load is `global_load v, v_offset32, s[base]` — one VALU instruction for the address instead of a
  // 64-bit shift-add per column and row (a tile is far smaller than 4 GB / 16)
  const bool ind = ic.indirect;   // late materialisation: source[index[row]] (random access, no streaming hint)
  const int rec = ind ? ic.rec_stride : 0;   // a field of the source's record copy (KCol::v = records + field offset)
  const std::string addr = rec ? "(*(const " + T + "*)((const char*)a.c[" + S + "].v + (size_t)((const u32*)a.c[" + S + "].d)[" + row_ + "] * " + std::to_string(rec) + "u))"
                           : ind ? "((const " + T + "*)a.c[" + S + "].v)[((const u32*)a.c[" + S + "].d)[" + row_ + "]]"
                           : base_.empty() ? "((const " + T + "*)a.c[" + S + "].v)[" + idx_ + "]"
                                         : "(*(const " + T + "*)((const char*)((const " + T + "*)a.c[" + S + "].v" + base_ + ") + (size_t)((u32)(" + idx_ +
                                               ") * (u32)sizeof(" + T + "))))";
  std::string rhs = addr;
  if (!ind && nt_) rhs = n.type.id == QHIP_DECIMAL128 && nb == 0 ? "qh_nt_load_i128(&" + addr + ")" : "__builtin_nontemporal_load(&" + addr + ")";
  if (nb && !raw_) rhs = "(" + ctype(n.type) + ")(" + rhs + ")";   // (sign-extending)
  ld << "    " << (raw_ ? "" : "const " + ctype(n.type) + " ") << (raw_ ? "w." : "") << v << " = " << rhs << ";\n";
  if (raw_) o << "    const " << ctype(n.type) << " " << v << " = (" << ctype(n.type) << ")w." << v << ";\n";
}

void ExprGen::emit_literal(int k, const ENode& n, std::ostringstream& o) {
  const std::string K = std::to_string(k), v = "v" + K;
  if (n.lit_null) {
    if (n.type.id == QHIP_UTF8) o << "    const u8* p" << K << " = a.strlit; const int l" << K << " = 0;\n";
    else o << "    const " << ctype(n.type) << " " << v << " = 0;\n";
    o << "    const bool n" << K << " = false;\n";
    return;
  }
  const int s = lit_slot(n);
  const std::string S = std::to_string(s);
  if (n.type.id == QHIP_UTF8)
    o << "    const u8* p" << K << " = a.strlit + a.stroff[" << S << "]; const int l" << K << " = a.stroff[" << s + 1 << "] - a.stroff[" << S << "];"
      << " const u64 w" << K << " = a.lit_lo[" << S << "];\n";
  else if (n.type.id == QHIP_DECIMAL128)
    o << "    const i128 " << v << " = qh_mk128(a.lit_lo[" << S << "], a.lit_hi[" << S << "]);\n";
  else if (n.type.id == QHIP_FLOAT64)
    o << "    const double " << v << " = qh_f64(a.lit_lo[" << S << "]);\n";
  else if (n.type.id == QHIP_FLOAT32)
    o << "    const float " << v << " = (float)qh_f64(a.lit_lo[" << S << "]);\n";
  else if (n.type.id == QHIP_BOOL)
    o << "    const bool " << v << " = (a.lit_lo[" << S << "] & 1) != 0;\n";
  else
    o << "    const " << ctype(n.type) << " " << v << " = (" << ctype(n.type) << ")a.lit_lo[" << S << "];\n";
}

void ExprGen::emit_binary(int k, const ENode& n, std::string& out, std::ostringstream& o) {
  emit(n.left, out);
  emit(n.right, out);
  if (is_cmp(n.op)) return emit_compare(k, n, o);
  if (n.op == QHIP_OP_AND || n.op == QHIP_OP_OR) return emit_kleene(k, n, o);
  if (n.nullable) o << "    const bool n" << k << " = " << ok(n.left) << " && " << ok(n.right) << ";\n";
  if (es_.at(n.left).type.id == QHIP_DECIMAL128 || es_.at(n.right).type.id == QHIP_DECIMAL128) emit_decimal_arith(k, n, o);
  else if (dtype_is_float(n.type)) emit_float_arith(k, n, o);
  else emit_int_arith(k, n, o);
}

void ExprGen::emit_compare(int k, const ENode& n, std::ostringstream& o) {
  const ENode &l = es_.at(n.left), &r = es_.at(n.right);
  const std::string v = val(k), nn = "n" + std::to_string(k), lv = val(n.left), rv = val(n.right);
  std::string e;
  if (l.type.id == QHIP_UTF8) {
    // (in)equality with a literal: its first 8 bytes travel as a kernel scalar (lit_slot), so values of up to 8 bytes
    // compare as one masked word instead of a byte loop with an early exit
    const bool rlit = r.kind == QHIP_EXPR_LITERAL && !r.lit_null, llit = l.kind == QHIP_EXPR_LITERAL && !l.lit_null;
    std::string eqx = "qh_streq(" + ptr(n.left) + ", " + len(n.left) + ", " + ptr(n.right) + ", " + len(n.right) + ")";
    if (rlit && !llit) eqx = "qh_streq_lit(" + ptr(n.left) + ", " + len(n.left) + ", " + ptr(n.right) + ", " + len(n.right) + ", w" + std::to_string(n.right) + ")";
    else if (llit && !rlit) eqx = "qh_streq_lit(" + ptr(n.right) + ", " + len(n.right) + ", " + ptr(n.left) + ", " + len(n.left) + ", w" + std::to_string(n.left) + ")";
    if (n.op == QHIP_OP_EQ) e = eqx;
    else if (n.op == QHIP_OP_NOTEQ) e = "!" + eqx;
    else e = "(qh_strcmp(" + ptr(n.left) + ", " + len(n.left) + ", " + ptr(n.right) + ", " + len(n.right) + ") " + c_cmp(n.op) + " 0)";
  } else if (dtype_is_float(l.type)) {
    // arrow-rs compares floats in IEEE total order
    e = "(qh_f64_ord((double)" + lv + ") " + c_cmp(n.op) + " qh_f64_ord((double)" + rv + "))";
  } else if (l.type.id == QHIP_BOOL) {
    e = "((int)" + lv + " " + c_cmp(n.op) + " (int)" + rv + ")";
  } else {
    e = "(" + lv + " " + c_cmp(n.op) + " " + rv + ")";
  }
  if (n.nullable) o << "    const bool " << nn << " = " << ok(n.left) << " && " << ok(n.right) << ";\n";
  if (n.nullable && l.type.id == QHIP_UTF8) o << "    const bool " << v << " = " << nn << " ? " << e << " : false;\n";
  else o << "    const bool " << v << " = " << e << ";\n";
}

// Kleene AND / OR (binary.rs:44-46): false AND NULL = false
void ExprGen::emit_kleene(int k, const ENode& n, std::ostringstream& o) {
  const std::string v = val(k), nn = "n" + std::to_string(k), lv = val(n.left), rv = val(n.right), lo = ok(n.left), ro = ok(n.right);
  if (!n.nullable) {
    o << "    const bool " << v << " = " << lv << (n.op == QHIP_OP_AND ? " && " : " || ") << rv << ";\n";
  } else if (n.op == QHIP_OP_AND) {
    o << "    const bool " << nn << " = (" << lo << " && " << ro << ") || (" << lo << " && !" << lv << ") || (" << ro << " && !" << rv << ");\n";
    o << "    const bool " << v << " = (!" << lo << " || " << lv << ") && (!" << ro << " || " << rv << ");\n";
  } else {
    o << "    const bool " << nn << " = (" << lo << " && " << ro << ") || (" << lo << " && " << lv << ") || (" << ro << " && " << rv << ");\n";
    o << "    const bool " << v << " = (" << lo << " && " << lv << ") || (" << ro << " && " << rv << ");\n";
  }
}

void ExprGen::emit_decimal_arith(int k, const ENode& n, std::ostringstream& o) {
  const ENode &l = es_.at(n.left), &r = es_.at(n.right);
  const std::string v = val(k), lv = val(n.left), rv = val(n.right);
  if (n.op == QHIP_OP_DIV) {
    auto tof = [&](const ENode& x, const std::string& xv) {
      if (x.type.id == QHIP_DECIMAL128) {
        char b[64]; snprintf(b, sizeof b, "1e%d", x.type.scale);
        return "((double)" + xv + " / " + b + ")";
      }
      return "(double)" + xv;
    };
    o << "    const double " << v << " = " << tof(l, lv) << " / " << tof(r, rv) << ";\n";
  } else if (n.op == QHIP_OP_MUL) {
    // operand magnitudes known from the columns' statistics (ENode::maxabs): a 32 x 32 -> 64 or 64 x 64 -> 128
    // multiply written out, instead of the generic 128-bit product behind wave-uniform "do all lanes fit" tests
    const u128 b31 = (u128)1 << 31, b63 = (u128)1 << 63;
    if (l.maxabs < b31 && r.maxabs < b31)
      o << "    const i128 " << v << " = (i128)((i64)(int)(u32)(u128)" << lv << " * (i64)(int)(u32)(u128)" << rv << ");\n";
    else if (l.maxabs < b63 && r.maxabs < b63)
      o << "    const i128 " << v << " = qh_mul_i64_i128((i64)(u64)(u128)" << lv << ", (i64)(u64)(u128)" << rv << ");\n";
    else
      o << "    const i128 " << v << " = " << (raw_ ? "qh_mul_i128(" : "qh_mul_i128_plain(") << lv << ", " << rv << ");\n";
  } else {
    const int s = n.type.scale;
    const char* c = n.op == QHIP_OP_ADD ? " + " : " - ";
    if (n.maxabs < ((u128)1 << 63)) {
      // the result (hence both rescaled operands) fits 63 bits: the sum in 64-bit arithmetic, sign-extended
      auto k64 = [&](int e) { return std::to_string((unsigned long long)(u128)pow10_i128(e)) + "ULL"; };
      std::string a = "(u64)(u128)" + lv, b = "(u64)(u128)" + rv;
      if (s > l.type.scale) a = "(" + a + " * " + k64(s - l.type.scale) + ")";
      if (s > r.type.scale) b = "(" + b + " * " + k64(s - r.type.scale) + ")";
      o << "    const i128 " << v << " = (i128)(i64)(" << a << c << b << ");\n";
    } else {
      std::string a = "(u128)" + lv, b = "(u128)" + rv;
      if (s > l.type.scale) a = "(" + a + " * (u128)" + i128_const(pow10_i128(s - l.type.scale)) + ")";
      if (s > r.type.scale) b = "(" + b + " * (u128)" + i128_const(pow10_i128(s - r.type.scale)) + ")";
      o << "    const i128 " << v << " = (i128)(" << a << c << b << ");\n";
    }
  }
}

void ExprGen::emit_float_arith(int k, const ENode& n, std::ostringstream& o) {
  const std::string T = ctype(n.type), v = val(k), lv = val(n.left), rv = val(n.right);
  const char* c = n.op == QHIP_OP_ADD ? "+" : n.op == QHIP_OP_SUB ? "-" : n.op == QHIP_OP_MUL ? "*" : "/";
  if (n.op == QHIP_OP_MOD) o << "    const " << T << " " << v << " = (" << T << ")fmod((double)" << lv << ", (double)" << rv << ");\n";
  else o << "    const " << T << " " << v << " = " << lv << " " << c << " " << rv << ";\n";
}

void ExprGen::emit_int_arith(int k, const ENode& n, std::ostringstream& o) {
  const std::string T = ctype(n.type), U = wrap_type(n.type), v = val(k), lv = val(n.left), rv = val(n.right);
  if (n.op == QHIP_OP_ADD || n.op == QHIP_OP_SUB || n.op == QHIP_OP_MUL) {
    const char* c = n.op == QHIP_OP_ADD ? "+" : n.op == QHIP_OP_SUB ? "-" : "*";
    o << "    const " << T << " " << v << " = (" << T << ")((" << U << ")" << lv << " " << c << " (" << U << ")" << rv << ");\n";
    return;
  }
  // arrow `div`/`rem` are checked: DivideByZero, and MIN / -1 overflows (evaluated on valid rows only)
  o << "    " << T << " " << v << " = 0;\n";
  o << "    if (" << ok(k) << ") {\n";
  o << "      if (" << rv << " == 0) " << raise(1u << QS_DIV_ZERO) << "\n";
  if (signed_intlike(n.type)) {
    if (n.op == QHIP_OP_DIV)
      o << "      else if (" << lv << " == " << int_min(n.type) << " && " << rv << " == -1) " << raise(1u << QS_ARITH_OVERFLOW) << "\n";
    else
      o << "      else if (" << rv << " == -1) " << v << " = 0;\n";
  }
  o << "      else " << v << " = (" << T << ")(" << lv << (n.op == QHIP_OP_DIV ? " / " : " % ") << rv << ");\n";
  o << "    }\n";
}

void ExprGen::emit_cast(int k, const ENode& n, std::string& out, std::ostringstream& o) {
  emit(n.left, out);
  const std::string K = std::to_string(k), v = "v" + K, cv = val(n.left);
  const DType& from = es_.at(n.left).type;
  const DType& to = n.type;
  const std::string T = ctype(to);
  if (n.nullable) o << "    const bool n" << K << " = " << ok(n.left) << ";\n";
  auto flag = [&](const std::string& cond) {
    o << "    if (" << ok(k) << " && (" << cond << ")) " << raise(1u << QS_CAST_OVERFLOW) << "\n";
  };
  auto flag_precision = [&]() { const std::string lim = i128_const(pow10_i128(to.precision)); flag(v + " >= " + lim + " || " + v + " <= -" + lim); };
  // x * 10^k as a Decimal128 of the target precision: arrow-rs multiplies checked and then checks the precision, and both hold
  // exactly when |x| < 10^(precision - k) (x == 0 when precision <= k) — tested on x, so no wrapped product can pass
  auto flag_scaled = [&](const std::string& x, int k10) {
    if (to.precision <= k10) { flag(x + " != 0"); return; }
    const std::string lim = i128_const(pow10_i128(to.precision - k10));
    flag(x + " >= " + lim + " || " + x + " <= -" + lim);
  };
  // range checks in i128 so that every (from, to) pair is handled uniformly
  const std::string wide = std::string(from.id == QHIP_UINT64 ? "(i128)(u128)" : "(i128)") + cv;
  const std::string lo128 = signed_intlike(to) ? "(i128)" + int_min(to) : "(i128)0";
  if (from == to) {
    o << "    const " << T << " " << v << " = " << cv << ";\n";
  } else if (from.id == QHIP_BOOL) {
    o << "    const " << T << " " << v << " = " << cv << " ? 1 : 0;\n";
  } else if (intlike(from) && intlike(to)) {
    if (from.id == QHIP_DATE32 && to.id == QHIP_DATE64) o << "    const i64 " << v << " = (i64)" << cv << " * 86400000LL;\n";
    else if (from.id == QHIP_DATE64 && to.id == QHIP_DATE32) o << "    const int " << v << " = (int)(" << cv << " / 86400000LL);\n";
    else {
      flag(wide + " < " + lo128 + " || " + wide + " > (i128)" + int_max(to));
      o << "    const " << T << " " << v << " = (" << T << ")" << cv << ";\n";
    }
  } else if ((intlike(from) || dtype_is_float(from)) && dtype_is_float(to)) {
    o << "    const " << T << " " << v << " = (" << T << ")" << cv << ";\n";
  } else if (dtype_is_float(from) && intlike(to)) {
    const std::string tr = "trunc((double)" + cv + ")";
    const std::string lo = signed_intlike(to) ? "(double)" + int_min(to) : "0.0";
    // arrow-rs (num::cast): lo <= trunc(x) < 2^bits. The bound is written as the power of two itself: (double)INT64_MAX
    // rounds up to 2^63, which `<=` would let through
    static const char* const s2[] = {"128.0", "32768.0", "2147483648.0", "9223372036854775808.0"}, *const u2[] = {"256.0", "65536.0", "4294967296.0", "18446744073709551616.0"};
    const std::string hi = (signed_intlike(to) ? s2 : u2)[log2u((uint32_t)dtype_width(to))];
    flag("!(" + tr + " >= " + lo + " && " + tr + " < " + hi + ")");
    o << "    const " << T << " " << v << " = (" << T << ")" << tr << ";\n";
  } else if (intlike(from) && to.id == QHIP_DECIMAL128) {
    o << "    const i128 " << v << " = (i128)((u128)" << wide << " * (u128)" << i128_const(pow10_i128(to.scale)) << ");\n";
    flag_scaled(wide, to.scale);
  } else if (from.id == QHIP_DECIMAL128 && to.id == QHIP_DECIMAL128) {
    if (to.scale >= from.scale) {
      o << "    const i128 " << v << " = (i128)((u128)" << cv << " * (u128)" << i128_const(pow10_i128(to.scale - from.scale)) << ");\n";
      flag_scaled(cv, to.scale - from.scale);
    } else {
      const std::string d = i128_const(pow10_i128(from.scale - to.scale));
      o << "    i128 " << v << " = " << cv << " / " << d << "; { const i128 rm = " << cv << " % " << d << ", hf = " << d << " / 2;"
        << " if (rm >= hf) " << v << " += 1; else if (-rm >= hf) " << v << " -= 1; }\n";
      flag_precision();
    }
  } else if (from.id == QHIP_DECIMAL128 && dtype_is_float(to)) {
    char b[64]; snprintf(b, sizeof b, "1e%d", from.scale);
    o << "    const " << T << " " << v << " = (" << T << ")((double)" << cv << " / " << b << ");\n";
  } else if (from.id == QHIP_DECIMAL128 && intlike(to)) {
    o << "    const i128 w" << K << " = " << cv << " / " << i128_const(pow10_i128(from.scale)) << ";\n";
    flag("w" + K + " < " + lo128 + " || w" + K + " > (i128)" + int_max(to));
    o << "    const " << T << " " << v << " = (" << T << ")w" << K << ";\n";
  } else if (dtype_is_float(from) && to.id == QHIP_DECIMAL128) {
    char b[64]; snprintf(b, sizeof b, "1e%d", to.scale);
    o << "    const double f" << K << " = round((double)" << cv << " * " << b << ");\n";
    // the precision check is made on the converted integer: the double nearest to 10^p may lie below 10^p (p = 23, 24, 38) and
    // is then a legal value. Every |f| < 1.7e38 converts (2^127 > 1.7e38 > 10^38); NaN and the rest are flagged
    o << "    const bool i" << K << " = fabs(f" << K << ") < 1.7e38;\n";
    o << "    const i128 " << v << " = i" << K << " ? (i128)f" << K << " : (i128)0;\n";
    const std::string lim = i128_const(pow10_i128(to.precision));
    flag("!i" + K + " || " + v + " >= " + lim + " || " + v + " <= -" + lim);
  } else {
    fail(QHIP_UNSUPPORTED, "device cast " + dtype_name(from) + " -> " + dtype_name(to));
  }
}

// arrow zip(mask, truthy, falsy) (case.rs:44): a NULL or false mask selects the falsy side; both sides are evaluated
// for every row (like the reference's full-array evaluation, so their error flags are raised regardless of the mask)
void ExprGen::emit_if(int k, const ENode& n, std::string& out, std::ostringstream& o) {
  emit(n.left, out); emit(n.right, out); emit(n.third, out);
  const std::string K = std::to_string(k), sel = "s" + K;
  o << "    const bool " << sel << " = " << ok(n.left) << " && " << val(n.left) << ";\n";
  if (n.nullable) o << "    const bool n" << K << " = " << sel << " ? " << ok(n.right) << " : " << ok(n.third) << ";\n";
  if (n.type.id == QHIP_UTF8) {
    o << "    const u8* p" << K << " = " << sel << " ? " << ptr(n.right) << " : " << ptr(n.third) << ";\n";
    o << "    const int l" << K << " = " << sel << " ? " << len(n.right) << " : " << len(n.third) << ";\n";
  } else {
    o << "    const " << ctype(n.type) << " v" << K << " = " << sel << " ? " << val(n.right) << " : " << val(n.third) << ";\n";
  }
}

void ExprGen::emit_like(int k, const ENode& n, std::string& out, std::ostringstream& o) {
  emit(n.left, out);
  const std::string v = val(k), nn = "n" + std::to_string(k);
  const std::string head = (n.nullable ? nn + " && " : std::string("")) + (n.op ? "!" : "");
  if (n.right >= 0 && es_.at(n.right).kind == QHIP_EXPR_COLUMN) {
    // a pattern per row (like.rs:28-43 -> arrow `like` over two arrays)
    emit(n.right, out);
    if (n.nullable) o << "    const bool " << nn << " = " << ok(n.left) << " && " << ok(n.right) << ";\n";
    o << "    const bool " << v << " = " << head << "qh_like_raw(" << ptr(n.left) << ", " << len(n.left) << ", " << ptr(n.right) << ", " << len(n.right) << ");\n";
    return;
  }
  if (n.lit_null) { o << "    const bool " << v << " = false;\n    const bool " << nn << " = false;\n"; return; }
  const int s = str_slot(n.s);
  if (n.nullable) o << "    const bool " << nn << " = " << ok(n.left) << ";\n";
  o << "    const bool " << v << " = " << head << "qh_like(" << ptr(n.left) << ", "
    << len(n.left) << ", a.strlit + a.stroff[" << s << "], a.stroff[" << s + 1 << "] - a.stroff[" << s << "]);\n";
}

// EXTRACT(part FROM x): the part (and the argument's unit) are constants of the source, so qh_dt_extract
// (device/qhip_datetime.inc) folds to the one path it needs; a row outside chrono's range is NULL
void ExprGen::emit_function(int k, const ENode& n, std::string& out, std::ostringstream& o) {
  emit(n.right, out);
  const ENode& x = es_.at(n.right);
  const int unit = x.type.id == QHIP_DATE32 ? -1 : x.type.id == QHIP_TIMESTAMP_S ? 0 : x.type.id == QHIP_TIMESTAMP_US ? 6
                 : x.type.id == QHIP_TIMESTAMP_NS ? 9 : 3;
  o << "    i64 v" << k << "; const bool r" << k << " = qh_dt_extract(" << n.dt_part << ", " << unit << ", (i64)" << val(n.right) << ", v" << k << ");\n";
  if (n.nullable) o << "    const bool n" << k << " = " << ok(n.right) << " && r" << k << ";\n";
  else o << "    (void)r" << k << ";\n";
}

void ExprGen::emit_negative(int k, const ENode& n, std::string& out, std::ostringstream& o) {
  emit(n.left, out);
  if (n.nullable) o << "    const bool n" << k << " = " << ok(n.left) << ";\n";
  const std::string T = ctype(n.type), v = val(k);
  if (dtype_is_float(n.type)) o << "    const " << T << " " << v << " = -" << val(n.left) << ";\n";
  else if (n.type.id == QHIP_DECIMAL128) o << "    const i128 " << v << " = (i128)((u128)0 - (u128)" << val(n.left) << ");\n";
  else o << "    const " << T << " " << v << " = (" << T << ")((" << wrap_type(n.type) << ")0 - (" << wrap_type(n.type) << ")" << val(n.left) << ");\n";
}

}  // namespace qhip
