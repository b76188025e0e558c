// qhip_float.inc — every spelling of the strict float grammar, correctly rounded (the float_parse switch, qhip_ctx_set_float_parse;
// DESIGN §3.8): the field parsers behind the column kinds QH_CSV_K_FLOAT64_FULL and QH_CSV_K_FLOAT32 of the device CSV and JSON
// decoders. Included by qhip_csv.inc behind its level-1 Float64 parser (qh_csv_parse_float64, Clinger's exact range only), which
// stays as it is; one text for two compilers like the file around it: builtin integer types only, every function reads exactly
// the bytes [p, p + len) it is given.
//
// The grammar is the level-1 one, -?[0-9]+(\.[0-9]+)?([eE][-+]?[0-9]+)?, without its incidental limits: any number of digits,
// any number of exponent digits. A field is converted exactly as a correct parser converts it (the nearest value, ties to
// even), or it raises QH_CSV_R_FLOAT and the file takes the host path. What raises it:
//   - a spelling outside the grammar (a leading '+', ".5", "5.", inf, nan, hex floats, blanks);
//   - a nonzero decimal whose nearest value is infinity or zero (Arrow's CSV and JSON readers differ about them);
//   - more than 19 significant digits of which the first 19, m, do not settle the result: the decimal lies strictly between
//     m * 10^q and (m + 1) * 10^q, so when both convert to the same value that is its value, and when they do not the digits
//     behind the 19th decide. There is no big-integer arithmetic here to read them with.
//
// The conversion of (m, q), m < 2^64: the Eisel-Lemire algorithm (Lemire, "Number parsing at a gigabyte per second", Software:
// Practice and Experience 51, 2021): m is normalised, multiplied by the 128-bit truncated power of five of 10^q (qhip_pow5.inc)
// and the product's top bits are the significand. Mushtak and Lemire ("Fast number parsing without fallback", 2023) prove that
// the 128-bit product decides every case, round-to-even ties and subnormal results included, so there is no slow path.
#include "qhip_pow5.inc"

// the decimal a field spells: (-1)^neg * (m + f) * 10^q with 0 <= f < 1, f != 0 exactly when `more`
struct qh_float_dec {
  unsigned long long m;   // the first 19 significant digits (fewer when the field has fewer)
  long long q;
  bool neg, more;         // more: a nonzero digit was left out of m
};

// QH_CSV_OK, QH_CSV_NULL (an empty field) or QH_CSV_R_FLOAT. Leading zeros are not significant and zeros behind the 19th digit
// leave `more` clear, so neither uses up the 19 digits. The exponent saturates above 2^40: q is off by less than `len` from it,
// and no field is 2^39 bytes long, so a saturated exponent stays far outside every table whatever the digits add.
QH_CSV_HD inline int qh_float_scan(const unsigned char* p, unsigned long long len, qh_float_dec* out) {
  if (len == 0) return QH_CSV_NULL;
  unsigned long long i = 0;
  out->neg = p[0] == '-';
  if (out->neg) i = 1;
  unsigned long long m = 0;
  int nd = 0;            // significant digits inside m
  long long q = 0;
  bool more = false;
  const unsigned long long int_begin = i;
  for (; i < len; ++i) {
    const unsigned d = (unsigned)p[i] - (unsigned)'0';
    if (d > 9u) break;
    if (nd < 19) { m = m * 10ULL + d; nd += m != 0; }
    else { ++q; more |= d != 0; }
  }
  if (i == int_begin) return QH_CSV_R_FLOAT;
  if (i < len && p[i] == '.') {
    const unsigned long long frac_begin = ++i;
    for (; i < len; ++i) {
      const unsigned d = (unsigned)p[i] - (unsigned)'0';
      if (d > 9u) break;
      if (nd < 19) { m = m * 10ULL + d; nd += m != 0; --q; }
      else more |= d != 0;
    }
    if (i == frac_begin) return QH_CSV_R_FLOAT;
  }
  if (i < len && (p[i] == 'e' || p[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < len && (p[i] == '-' || p[i] == '+')) { eneg = p[i] == '-'; ++i; }
    const unsigned long long exp_begin = i;
    long long e = 0;
    for (; i < len; ++i) {
      const unsigned d = (unsigned)p[i] - (unsigned)'0';
      if (d > 9u) return QH_CSV_R_FLOAT;
      if (e < (1LL << 40)) e = e * 10 + (long long)d;
    }
    if (i == exp_begin) return QH_CSV_R_FLOAT;
    q += eneg ? -e : e;
  }
  if (i != len) return QH_CSV_R_FLOAT;
  out->m = m;
  out->q = q;
  out->more = more;
  return QH_CSV_OK;
}

// ---- Eisel-Lemire: the IEEE bits (without the sign) of the value nearest to w * 10^q, w != 0; F32: binary32, else binary64.
// Zero (all bits clear) and infinity (the exponent field full, the fraction clear) are results like any other: the callers
// turn them into the reason.
template <bool F32>
QH_CSV_HD inline unsigned long long qh_float_eisel_lemire(unsigned long long w, long long q) {
  typedef unsigned __int128 qh_u128;
  const int mant_bits = F32 ? 23 : 52;              // explicit bits of the significand
  const int min_exp = F32 ? -127 : -1023;
  const int inf_exp = F32 ? 0xFF : 0x7FF;
  const long long tie_q_lo = F32 ? -17 : -4;        // outside these powers w * 10^q is never halfway between two values
  const long long tie_q_hi = F32 ? 10 : 23;
  const unsigned long long inf_bits = (unsigned long long)inf_exp << mant_bits;
  // w < 2^64 < 1.9 * 10^19: below these powers the value is under half the smallest subnormal, above them over the largest finite
  if (q < (F32 ? -65 : QH_POW5_Q_MIN)) return 0ULL;
  if (q > (F32 ? 38 : QH_POW5_Q_MAX)) return inf_bits;
  const int lz = __builtin_clzll(w);
  w <<= lz;
  const unsigned long long* t = qh_pow5_128 + 2 * (q - QH_POW5_Q_MIN);
  // the top mant_bits + 3 bits of the product are wanted: when the bits below them in the first product are all ones, the
  // table's low word may carry into them
  qh_u128 first = (qh_u128)w * t[0];
  unsigned long long hi = (unsigned long long)(first >> 64), lo = (unsigned long long)first;
  const unsigned long long below = ~0ULL >> (mant_bits + 3);
  if ((hi & below) == below) {
    const unsigned long long second_hi = (unsigned long long)(((qh_u128)w * t[1]) >> 64);
    lo += second_hi;
    if (second_hi > lo) ++hi;
  }
  const int upper = (int)(hi >> 63);
  const int shift = upper + 64 - mant_bits - 3;
  unsigned long long mant = hi >> shift;
  // floor(log2(10^q)) + 63 = ((217706 * q) >> 16) + 63 for every q of the table (217706 / 65536 = 3.3219...)
  int power2 = (int)((217706LL * q) >> 16) + 63 + upper - lz - min_exp;
  if (power2 <= 0) {                                 // a subnormal result, or zero
    if (-power2 + 1 >= 64) return 0ULL;
    mant >>= -power2 + 1;
    mant += mant & 1ULL;                             // round up; a tie cannot occur down here (q is far below tie_q_lo)
    mant >>= 1;
    // (a carry into bit mant_bits is the smallest normal value: the bit lands in the exponent field by itself)
    return mant;
  }
  // exactly halfway, rounding to even: the product is exact (lo <= 1 holds what truncation left) and the bits shifted out are zero
  if (lo <= 1ULL && q >= tie_q_lo && q <= tie_q_hi && (mant & 3ULL) == 1ULL && (mant << shift) == hi) mant &= ~1ULL;
  mant += mant & 1ULL;
  mant >>= 1;
  if (mant >= (2ULL << mant_bits)) { mant = 1ULL << mant_bits; ++power2; }
  mant &= ~(1ULL << mant_bits);
  if (power2 >= inf_exp) return inf_bits;
  return mant | ((unsigned long long)power2 << mant_bits);
}

// the bits of a scanned decimal, or QH_CSV_R_FLOAT (the header's second and third case)
template <bool F32>
QH_CSV_HD inline int qh_float_convert(const qh_float_dec& d, unsigned long long* bits) {
  const unsigned long long sign = d.neg ? 1ULL << (F32 ? 31 : 63) : 0ULL;
  if (d.m == 0 && !d.more) { *bits = sign; return QH_CSV_OK; }   // a decimal that is zero, whatever its exponent: +-0.0
  const unsigned long long inf_bits = F32 ? 0xFFULL << 23 : 0x7FFULL << 52;
  const unsigned long long v = qh_float_eisel_lemire<F32>(d.m, d.q);
  // (m has 19 digits when `more` is set: m + 1 <= 10^19 < 2^64)
  if (d.more && qh_float_eisel_lemire<F32>(d.m + 1ULL, d.q) != v) return QH_CSV_R_FLOAT;
  if (v == 0ULL || v == inf_bits) return QH_CSV_R_FLOAT;
  *bits = v | sign;
  return QH_CSV_OK;
}

// ---- one field -> the IEEE bits. Float64: Clinger's one-operation path first, for the inputs qh_csv_parse_float64 covers:
// the same operation on the same operands, hence the same bits. Float32: the same algorithm with binary32's parameters on the
// decimal itself, one rounding. (Rounding the Float64 to Float32 would be two: 1.000000059604644776 is 1.00000011920928955 as a
// Float32 and 1.0 by way of the double.)
// `json`: the field is a JSON number token. Arrow's JSON reader lets its tokenizer (RapidJSON) look at every number before the
// converter sees it, and the tokenizer refuses a positive exponent that, less the fraction digits, exceeds 308 ("Number too
// big") — for a nonzero value that means infinity, which is refused here anyway, but it refuses 0e309 too, which the CSV reader
// takes for the zero it is. That error message belongs to the host.
template <bool F32>
QH_CSV_HD inline int qh_float_parse(const unsigned char* p, unsigned long long len, bool json, unsigned long long* bits) {
  qh_float_dec d;
  const int st = qh_float_scan(p, len, &d);
  if (st != QH_CSV_OK) return st;
  if (json && d.m == 0 && d.q > 308) return QH_CSV_R_FLOAT;
  if (!F32 && !d.more && d.m <= (1ULL << 53) && d.q >= -22 && d.q <= 22) {
    const double dm = (double)d.m;
    double v = d.q >= 0 ? dm * qh_csv_pow10((int)d.q) : dm / qh_csv_pow10((int)-d.q);
    if (d.neg) v = -v;                                  // (-0.0 keeps its sign)
    __builtin_memcpy(bits, &v, 8);
    return QH_CSV_OK;
  }
  return qh_float_convert<F32>(d, bits);
}

QH_CSV_HD inline int qh_parse_float64_full(const unsigned char* p, unsigned long long len, double* out) {
  unsigned long long bits = 0;
  const int st = qh_float_parse<false>(p, len, false, &bits);
  if (st == QH_CSV_OK) __builtin_memcpy(out, &bits, 8);
  return st;
}
QH_CSV_HD inline int qh_parse_float32_full(const unsigned char* p, unsigned long long len, float* out) {
  unsigned long long bits = 0;
  const int st = qh_float_parse<true>(p, len, false, &bits);
  const unsigned b32 = (unsigned)bits;
  if (st == QH_CSV_OK) __builtin_memcpy(out, &b32, 4);
  return st;
}
