// qhip_csv.inc — per-byte and per-field code of the device CSV decoder (csv.cpp qhip_table_from_csv, kernels_csv.hip):
// the record splitter's byte classification and the field parsers of the strict canonical grammar (DESIGN §3.8). A field is
// either decoded EXACTLY as Arrow C++'s CSV reader with an explicit schema decodes it, or it raises a "needs host" reason and
// the whole call answers QHIP_UNSUPPORTED: the device path never imitates a lenient spelling or an error message.
//
// One text for two compilers: included by kernels_csv.hip for hipcc and, as plain host C++, by tests/cpp/csv_tests.cpp, so the
// functions the kernels call are the functions the CPU tests check. Self-contained: builtin integer types only, no #include but
// qhip_float.inc beside it (the float_parse switch: every Float64 spelling, Float32).
// Every function reads exactly the bytes [p, p + len) it is given (generic pointers: LDS or global memory on the device).
#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define QH_CSV_HD __host__ __device__
#else
#define QH_CSV_HD
#endif

#define QH_CSV_MAX_COLS 64

// outcome of a field: a value, NULL (an empty field of a non-Utf8 column), or the reason the file needs the host path
#define QH_CSV_OK 0
#define QH_CSV_NULL 1
#define QH_CSV_R_QUOTE 2         // the quote byte occurs somewhere in the data
#define QH_CSV_R_LONE_CR 3       // a '\r' that is not followed by '\n'
#define QH_CSV_R_EMPTY_LINE 4    // an empty line (the host path skips them; here they are outside the grammar)
#define QH_CSV_R_FIELD_COUNT 5   // a record with fewer or more fields than the schema
#define QH_CSV_R_INT 6
#define QH_CSV_R_DATE 7
#define QH_CSV_R_DECIMAL 8
#define QH_CSV_R_FLOAT 9
#define QH_CSV_R_UTF8 10         // invalid UTF-8
#define QH_CSV_R_UTF8_LONG 11    // one Utf8 field of more than 2^31 - 1 bytes
// (grammar level 2 only, qhip_ctx_set_csv_grammar)
#define QH_CSV_R_QUOTING 12      // a field that holds the quote byte and is not a canonical quoted field
#define QH_CSV_R_BOOL 13
#define QH_CSV_R_TIMESTAMP 14
#define QH_CSV_R_COUNT 15

QH_CSV_HD inline const char* qh_csv_reason_text(unsigned r) {
  switch (r) {
    case QH_CSV_R_QUOTE: return "a quote character";
    case QH_CSV_R_LONE_CR: return "a carriage return that is not followed by a line feed";
    case QH_CSV_R_EMPTY_LINE: return "an empty line";
    case QH_CSV_R_FIELD_COUNT: return "a record whose field count differs from the schema's";
    case QH_CSV_R_INT: return "an integer outside -?[0-9]+ or outside its type's range";
    case QH_CSV_R_DATE: return "a date that is not a valid YYYY-MM-DD";
    case QH_CSV_R_DECIMAL: return "a decimal outside -?[0-9]*(.[0-9]*)? or outside its precision and scale";
    case QH_CSV_R_FLOAT: return "a float outside the exactly convertible spellings";
    case QH_CSV_R_UTF8: return "invalid UTF-8";
    case QH_CSV_R_UTF8_LONG: return "a string field of 2 GiB or more";
    case QH_CSV_R_QUOTING: return "quoting outside the canonical form";
    case QH_CSV_R_BOOL: return "a boolean that is not true or false";
    case QH_CSV_R_TIMESTAMP: return "a timestamp outside YYYY-MM-DD[ T]hh:mm:ss[.fraction] or outside its unit's range";
    default: return "an unknown reason";
  }
}

// ---- the record splitter's view of a byte
#define QH_CSV_B_LF 1u
#define QH_CSV_B_CR 2u
#define QH_CSV_B_QUOTE 4u
QH_CSV_HD inline unsigned qh_csv_byte_class(unsigned char b, int quote) {
  return (b == '\n' ? QH_CSV_B_LF : 0u) | (b == '\r' ? QH_CSV_B_CR : 0u) | ((int)b == quote ? QH_CSV_B_QUOTE : 0u);
}

// ---- column descriptors: what the decode kernel is driven by (a kernel argument, like qh_wk_col)
#define QH_CSV_K_INT 0
#define QH_CSV_K_DATE32 1
#define QH_CSV_K_DECIMAL128 2
#define QH_CSV_K_FLOAT64 3
#define QH_CSV_K_UTF8 4
#define QH_CSV_K_BOOL 5          // grammar level 2: no `values` store per row, the kernel packs 64 rows into one ballot word
#define QH_CSV_K_TIMESTAMP 6     // grammar level 2: a = fraction digits of the unit (0 s, 3 ms, 6 us, 9 ns)
#define QH_CSV_K_FLOAT64_FULL 7  // float_parse level 2 (qhip_ctx_set_float_parse): every spelling of the grammar, qhip_float.inc
#define QH_CSV_K_FLOAT32 8       // float_parse level 2: 4-byte values
struct qh_csv_col {
  void* values;                  // row-indexed values of `width` bytes; Utf8: the u32 LENGTH of every row (scanned into offsets later)
  unsigned long long* valid;     // one ballot word per 64 rows (written by the kernel, not by the functions below)
  unsigned long long* strpos;    // Utf8: where the field starts in the file (64-bit: files are larger than 4 GB)
  unsigned field;                // index of the field inside a record
  unsigned char kind, width;     // QH_CSV_K_*; bytes per value (Int: 1, 2, 4, 8)
  unsigned char a, b;            // Int: a = signed; Decimal128: a = precision, b = scale; Timestamp: a = fraction digits
};

// ---- integers: -?[0-9]+ inside the type's range (leading zeros are fine, "-0" is 0, no '-' at all for unsigned types)
QH_CSV_HD inline int qh_csv_parse_int(const unsigned char* p, unsigned long long len, int width, int is_signed, unsigned long long* out) {
  if (len == 0) return QH_CSV_NULL;
  unsigned long long i = 0;
  const bool neg = p[0] == '-';
  if (neg) { if (!is_signed) return QH_CSV_R_INT; i = 1; }
  if (i == len) return QH_CSV_R_INT;
  unsigned long long v = 0;
  for (; i < len; ++i) {
    const unsigned d = (unsigned)p[i] - (unsigned)'0';
    if (d > 9u) return QH_CSV_R_INT;
    if (v > (~0ULL - d) / 10ULL) return QH_CSV_R_INT;
    v = v * 10ULL + d;
  }
  unsigned long long max;
  if (is_signed) max = (1ULL << (8 * width - 1)) - (neg ? 0ULL : 1ULL);
  else max = width == 8 ? ~0ULL : (1ULL << (8 * width)) - 1ULL;
  if (v > max) return QH_CSV_R_INT;
  *out = neg ? 0ULL - v : v;
  return QH_CSV_OK;
}

// ---- Date32: exactly YYYY-MM-DD, a valid civil date of the years 0001 to 9999 -> days since 1970-01-01
QH_CSV_HD inline int qh_csv_parse_date32(const unsigned char* p, unsigned long long len, int* out) {
  if (len == 0) return QH_CSV_NULL;
  if (len != 10 || p[4] != '-' || p[7] != '-') return QH_CSV_R_DATE;
  unsigned dg[10];
  for (int i = 0; i < 10; ++i) {
    if (i == 4 || i == 7) { dg[i] = 0; continue; }
    dg[i] = (unsigned)p[i] - (unsigned)'0';
    if (dg[i] > 9u) return QH_CSV_R_DATE;
  }
  const int y = (int)(dg[0] * 1000u + dg[1] * 100u + dg[2] * 10u + dg[3]);
  const int m = (int)(dg[5] * 10u + dg[6]);
  const int d = (int)(dg[8] * 10u + dg[9]);
  if (y < 1 || m < 1 || m > 12 || d < 1) return QH_CSV_R_DATE;
  const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
  const int dim = m == 2 ? (leap ? 29 : 28) : ((m == 4 || m == 6 || m == 9 || m == 11) ? 30 : 31);
  if (d > dim) return QH_CSV_R_DATE;
  // days from civil (proleptic Gregorian; y >= 1, so every division is of a non-negative number)
  const int yy = m <= 2 ? y - 1 : y;
  const int era = yy / 400;
  const int yoe = yy - era * 400;
  const int doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
  const int doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  *out = era * 146097 + doe - 719468;
  return QH_CSV_OK;
}

// ---- Decimal128(p, s >= 0): -?[0-9]*(\.[0-9]*)? with at least one digit, at most s fractional digits, |value| < 10^p.
// The unscaled value as two's complement in out[0] (low) / out[1] (high). Multiplications, additions and comparisons of
// unsigned __int128 only (no division: the device has none).
QH_CSV_HD inline int qh_csv_parse_decimal128(const unsigned char* p, unsigned long long len, int precision, int scale, unsigned long long* out) {
  typedef unsigned __int128 qh_u128;
  if (len == 0) return QH_CSV_NULL;
  qh_u128 lim38 = 1;                                  // 10^38 < 2^127: nothing below may pass it
  for (int i = 0; i < 38; ++i) lim38 *= 10u;
  unsigned long long i = 0;
  const bool neg = p[0] == '-';
  if (neg) i = 1;
  qh_u128 v = 0;
  unsigned long long ndigits = 0;
  int frac = -1;                                      // -1: no '.' yet; else the fractional digits read so far
  for (; i < len; ++i) {
    const unsigned char c = p[i];
    if (c == '.') { if (frac >= 0) return QH_CSV_R_DECIMAL; frac = 0; continue; }
    const unsigned d = (unsigned)c - (unsigned)'0';
    if (d > 9u) return QH_CSV_R_DECIMAL;
    if (frac >= 0 && ++frac > scale) return QH_CSV_R_DECIMAL;   // would lose digits
    v = v * 10u + d;
    if (v >= lim38) return QH_CSV_R_DECIMAL;
    ++ndigits;
  }
  if (ndigits == 0) return QH_CSV_R_DECIMAL;
  for (int k = frac < 0 ? 0 : frac; k < scale; ++k) {
    v *= 10u;
    if (v >= lim38) return QH_CSV_R_DECIMAL;
  }
  qh_u128 limp = 1;
  for (int k = 0; k < precision; ++k) limp *= 10u;
  if (v >= limp) return QH_CSV_R_DECIMAL;
  if (neg) v = (qh_u128)0 - v;
  out[0] = (unsigned long long)v;
  out[1] = (unsigned long long)(v >> 64);
  return QH_CSV_OK;
}

// ---- Float64: -?[0-9]+(\.[0-9]+)?([eE][-+]?[0-9]+)? in Clinger's exact range only. The digits without the point form an
// integer m <= 2^53, the effective power of ten e has |e| <= 22: m and 10^|e| are exact doubles, and m * 10^e or
// m / 10^|e| is ONE correctly rounded IEEE operation — the same bits as any correct parser. Everything else needs the host.
QH_CSV_HD inline double qh_csv_pow10(int e) {          // 10^e, 0 <= e <= 22, exact
  unsigned long long a = 1;
  const int e1 = e > 19 ? 19 : e;
  for (int k = 0; k < e1; ++k) a *= 10ULL;
  double r = (double)a;                                 // 10^19 = 2^19 * 5^19, 5^19 < 2^53: exact
  if (e > 19) {
    unsigned long long b = 1;
    for (int k = 19; k < e; ++k) b *= 10ULL;
    r = r * (double)b;                                  // the product (<= 10^22 = 2^22 * 5^22, 5^22 < 2^53) is representable: exact
  }
  return r;
}
QH_CSV_HD inline int qh_csv_parse_float64(const unsigned char* p, unsigned long long len, double* out) {
  if (len == 0) return QH_CSV_NULL;
  unsigned long long i = 0;
  const bool neg = p[0] == '-';
  if (neg) i = 1;
  unsigned long long m = 0;
  unsigned long long nint = 0, nfrac = 0;
  for (; i < len; ++i) {
    const unsigned d = (unsigned)p[i] - (unsigned)'0';
    if (d > 9u) break;
    m = m * 10ULL + d;
    if (m > (1ULL << 53)) return QH_CSV_R_FLOAT;
    ++nint;
  }
  if (nint == 0) return QH_CSV_R_FLOAT;
  if (i < len && p[i] == '.') {
    ++i;
    for (; i < len; ++i) {
      const unsigned d = (unsigned)p[i] - (unsigned)'0';
      if (d > 9u) break;
      m = m * 10ULL + d;
      if (m > (1ULL << 53)) return QH_CSV_R_FLOAT;
      ++nfrac;
    }
    if (nfrac == 0) return QH_CSV_R_FLOAT;
  }
  if (nfrac > 64) return QH_CSV_R_FLOAT;
  long long e = 0;
  if (i < len && (p[i] == 'e' || p[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < len && (p[i] == '-' || p[i] == '+')) { eneg = p[i] == '-'; ++i; }
    unsigned long long nexp = 0;
    for (; i < len; ++i) {
      const unsigned d = (unsigned)p[i] - (unsigned)'0';
      if (d > 9u) return QH_CSV_R_FLOAT;
      e = e * 10 + (long long)d;
      if (e > 100000) return QH_CSV_R_FLOAT;
      ++nexp;
    }
    if (nexp == 0) return QH_CSV_R_FLOAT;
    if (eneg) e = -e;
  }
  if (i != len) return QH_CSV_R_FLOAT;
  e -= (long long)nfrac;
  if (e > 22 || e < -22) return QH_CSV_R_FLOAT;
  const double dm = (double)m;                          // m <= 2^53: exact
  double v = e >= 0 ? dm * qh_csv_pow10((int)e) : dm / qh_csv_pow10((int)-e);
  *out = neg ? -v : v;                                  // (-0.0 keeps its sign)
  return QH_CSV_OK;
}

// ---- float_parse level 2: qh_parse_float64_full, qh_parse_float32_full
#include "qhip_float.inc"

// ---- Utf8: the bytes as they are (a NUL byte is data); well-formed UTF-8 only (no overlong forms, no surrogates, <= U+10FFFF)
QH_CSV_HD inline int qh_csv_check_utf8(const unsigned char* p, unsigned long long len) {
  unsigned long long i = 0;
  while (i < len) {
    const unsigned c = p[i];
    if (c < 0x80u) { ++i; continue; }
    unsigned n, lo = 0x80u, hi = 0xBFu;
    if (c >= 0xC2u && c <= 0xDFu) n = 1;
    else if (c == 0xE0u) { n = 2; lo = 0xA0u; }
    else if (c == 0xEDu) { n = 2; hi = 0x9Fu; }
    else if (c >= 0xE1u && c <= 0xEFu) n = 2;
    else if (c == 0xF0u) { n = 3; lo = 0x90u; }
    else if (c >= 0xF1u && c <= 0xF3u) n = 3;
    else if (c == 0xF4u) { n = 3; hi = 0x8Fu; }
    else return QH_CSV_R_UTF8;
    if (len - i <= n) return QH_CSV_R_UTF8;
    const unsigned c1 = p[i + 1];
    if (c1 < lo || c1 > hi) return QH_CSV_R_UTF8;
    for (unsigned k = 2; k <= n; ++k)
      if ((p[i + k] & 0xC0u) != 0x80u) return QH_CSV_R_UTF8;
    i += n + 1;
  }
  return QH_CSV_OK;
}

// ---- one field of one row -> the column's buffers. `filepos`: where the field starts in the file.
QH_CSV_HD inline int qh_csv_parse_store(const qh_csv_col& c, const unsigned char* p, unsigned long long len, unsigned long long row,
                                        unsigned long long filepos) {
  switch (c.kind) {
    case QH_CSV_K_INT: {
      unsigned long long v = 0;
      const int st = qh_csv_parse_int(p, len, c.width, c.a, &v);
      if (st != QH_CSV_OK) v = 0;
      switch (c.width) {
        case 1: ((unsigned char*)c.values)[row] = (unsigned char)v; break;
        case 2: ((unsigned short*)c.values)[row] = (unsigned short)v; break;
        case 4: ((unsigned*)c.values)[row] = (unsigned)v; break;
        default: ((unsigned long long*)c.values)[row] = v; break;
      }
      return st;
    }
    case QH_CSV_K_DATE32: {
      int v = 0;
      const int st = qh_csv_parse_date32(p, len, &v);
      ((int*)c.values)[row] = st == QH_CSV_OK ? v : 0;
      return st;
    }
    case QH_CSV_K_DECIMAL128: {
      unsigned long long v[2] = {0, 0};
      const int st = qh_csv_parse_decimal128(p, len, c.a, c.b, v);
      unsigned long long* o = (unsigned long long*)c.values + 2 * row;
      o[0] = st == QH_CSV_OK ? v[0] : 0;
      o[1] = st == QH_CSV_OK ? v[1] : 0;
      return st;
    }
    case QH_CSV_K_FLOAT64: {
      double v = 0.0;
      const int st = qh_csv_parse_float64(p, len, &v);
      ((double*)c.values)[row] = st == QH_CSV_OK ? v : 0.0;
      return st;
    }
    case QH_CSV_K_FLOAT64_FULL: {
      double v = 0.0;
      const int st = qh_parse_float64_full(p, len, &v);
      ((double*)c.values)[row] = st == QH_CSV_OK ? v : 0.0;
      return st;
    }
    case QH_CSV_K_FLOAT32: {
      float v = 0.0f;
      const int st = qh_parse_float32_full(p, len, &v);
      ((float*)c.values)[row] = st == QH_CSV_OK ? v : 0.0f;
      return st;
    }
    default: {   // QH_CSV_K_UTF8: an empty field is the empty string, never NULL
      const bool too_long = len > 0x7fffffffULL;
      ((unsigned*)c.values)[row] = too_long ? 0u : (unsigned)len;
      c.strpos[row] = filepos;
      if (too_long) return QH_CSV_R_UTF8_LONG;
      return qh_csv_check_utf8(p, len);
    }
  }
}

// ---- one record: bytes [p, p + len) without its line end, at `filepos` in the file. Splits at `delim`, decodes the fields the
// descriptors name (cols: ascending by .field; a field may be named more than once) and skips the others unparsed: garbage in
// an unprojected field is not an error, only the NUMBER of fields is checked for every record. Returns QH_CSV_OK or the
// record's first needs-host reason; bit k of *valid_mask: descriptor k got a value (clear: NULL, or not reached).
QH_CSV_HD inline int qh_csv_decode_record(const qh_csv_col* cols, int ncols, unsigned nfields, unsigned char delim, const unsigned char* p,
                                          unsigned long long len, unsigned long long row, unsigned long long filepos,
                                          unsigned long long* valid_mask) {
  unsigned long long vm = 0;
  int reason = QH_CSV_OK;
  unsigned f = 0;
  int k = 0;
  unsigned long long a = 0;
  for (;;) {
    unsigned long long b = a;
    while (b < len && p[b] != delim) ++b;
    while (k < ncols && cols[k].field == f) {
      const int st = qh_csv_parse_store(cols[k], p + a, b - a, row, filepos + a);
      if (st == QH_CSV_OK) vm |= 1ULL << k;
      else if (st != QH_CSV_NULL && reason == QH_CSV_OK) reason = st;
      ++k;
    }
    ++f;
    if (b >= len) break;
    a = b + 1;
    if (f > nfields) break;   // already too long: the rest of the record need not be walked
  }
  *valid_mask = vm;
  if (f != nfields) return QH_CSV_R_FIELD_COUNT;
  return reason;
}

// ================================================================ grammar level 2 (qhip_ctx_set_csv_grammar; DESIGN §3.8)
// Quoted fields, Boolean and Timestamp columns. Everything above is level 1 and stays as it is: the level-1 kernel calls
// qh_csv_decode_record, the level-2 kernel calls qh_csv_decode_record_q below.

// ---- Boolean: exactly "true" or "false"
QH_CSV_HD inline int qh_csv_parse_bool(const unsigned char* p, unsigned long long len, int* out) {
  if (len == 0) return QH_CSV_NULL;
  if (len == 4 && p[0] == 't' && p[1] == 'r' && p[2] == 'u' && p[3] == 'e') { *out = 1; return QH_CSV_OK; }
  if (len == 5 && p[0] == 'f' && p[1] == 'a' && p[2] == 'l' && p[3] == 's' && p[4] == 'e') { *out = 0; return QH_CSV_OK; }
  return QH_CSV_R_BOOL;
}

// ---- Timestamp without a zone: YYYY-MM-DD, one ' ' or 'T', hh:mm:ss, then optionally '.' and 1..digits digits (digits: 0 for
// seconds, 3, 6, 9), padded on the right -> units since 1970-01-01T00:00:00. Nanoseconds must fit 64 bits.
QH_CSV_HD inline int qh_csv_parse_timestamp(const unsigned char* p, unsigned long long len, int digits, long long* out) {
  if (len == 0) return QH_CSV_NULL;
  if (len < 19 || len > 20ULL + (unsigned)digits || len == 20) return QH_CSV_R_TIMESTAMP;
  if ((p[10] != ' ' && p[10] != 'T') || p[13] != ':' || p[16] != ':') return QH_CSV_R_TIMESTAMP;
  int days = 0;
  if (qh_csv_parse_date32(p, 10, &days) != QH_CSV_OK) return QH_CSV_R_TIMESTAMP;
  unsigned t[3];
  for (int k = 0; k < 3; ++k) {
    const unsigned hi = (unsigned)p[11 + 3 * k] - (unsigned)'0', lo = (unsigned)p[12 + 3 * k] - (unsigned)'0';
    if (hi > 9u || lo > 9u) return QH_CSV_R_TIMESTAMP;
    t[k] = hi * 10u + lo;
  }
  if (t[0] > 23u || t[1] > 59u || t[2] > 59u) return QH_CSV_R_TIMESTAMP;
  unsigned long long frac = 0;
  if (len > 19) {
    if (p[19] != '.') return QH_CSV_R_TIMESTAMP;
    for (unsigned long long i = 20; i < len; ++i) {
      const unsigned d = (unsigned)p[i] - (unsigned)'0';
      if (d > 9u) return QH_CSV_R_TIMESTAMP;
      frac = frac * 10ULL + d;
    }
    for (unsigned long long i = len; i < 20ULL + (unsigned)digits; ++i) frac *= 10ULL;
  }
  const long long secs = (long long)days * 86400LL + (long long)(t[0] * 3600u + t[1] * 60u + t[2]);
  unsigned long long mul = 1;
  for (int k = 0; k < digits; ++k) mul *= 10ULL;
  if (digits == 9) {
    // 1677-09-21T00:12:44 to 2262-04-11T23:47:16.854775807. Arrow C++ refuses every instant whose whole seconds alone do not
    // fit as nanoseconds, so the 0.854775808 s below -9223372036 s that int64 could hold belong to the host and its error
    if (secs > 9223372036LL || (secs == 9223372036LL && frac > 854775807ULL)) return QH_CSV_R_TIMESTAMP;
    if (secs < -9223372036LL) return QH_CSV_R_TIMESTAMP;
  }
  *out = (long long)((unsigned long long)secs * mul + frac);   // (unsigned arithmetic: a negative count of seconds wraps as two's complement does)
  return QH_CSV_OK;
}

// ---- Utf8 at level 2: bits 63 and 62 of strpos[row]. Positions in a file stay far below 2^62.
#define QH_CSV_POS_PAIRS (1ULL << 63)   // the field holds doubled quotes: the copy drops the second of every pair
#define QH_CSV_POS_LONG (1ULL << 62)    // ... and its raw inner span is longer than 64 bytes: the whole wavefront copies it
#define QH_CSV_POS_MASK ((1ULL << 62) - 1ULL)

// the reason a column's kind gives when its field cannot be a value of it
QH_CSV_HD inline int qh_csv_kind_reason(int kind) {
  switch (kind) {
    case QH_CSV_K_INT: return QH_CSV_R_INT;
    case QH_CSV_K_DATE32: return QH_CSV_R_DATE;
    case QH_CSV_K_DECIMAL128: return QH_CSV_R_DECIMAL;
    case QH_CSV_K_FLOAT64: case QH_CSV_K_FLOAT64_FULL: case QH_CSV_K_FLOAT32: return QH_CSV_R_FLOAT;
    case QH_CSV_K_BOOL: return QH_CSV_R_BOOL;
    case QH_CSV_K_TIMESTAMP: return QH_CSV_R_TIMESTAMP;
    default: return QH_CSV_R_UTF8;
  }
}

// ---- one field of one row at level 2. [p, p + len): the field without its quotes, `pairs` doubled quotes still inside;
// `filepos`: where p[0] is in the file. *truth: a Boolean's value (the kernel packs it; nothing is stored here).
QH_CSV_HD inline int qh_csv_parse_store_q(const qh_csv_col& c, const unsigned char* p, unsigned long long len, unsigned long long pairs,
                                          unsigned long long row, unsigned long long filepos, int* truth) {
  switch (c.kind) {
    case QH_CSV_K_UTF8: {
      const unsigned long long ulen = len - pairs;   // the unescaped length: what the offsets and byte totals are made of
      const bool too_long = ulen > 0x7fffffffULL;
      ((unsigned*)c.values)[row] = too_long ? 0u : (unsigned)ulen;
      c.strpos[row] = filepos | (pairs ? QH_CSV_POS_PAIRS | (len > 64 ? QH_CSV_POS_LONG : 0ULL) : 0ULL);
      if (too_long) return QH_CSV_R_UTF8_LONG;
      return qh_csv_check_utf8(p, len);   // (the quote is an ASCII byte: dropping one of two leaves validity as it is)
    }
    case QH_CSV_K_BOOL: {
      int v = 0;
      const int st = pairs ? QH_CSV_R_BOOL : qh_csv_parse_bool(p, len, &v);
      *truth = st == QH_CSV_OK ? v : 0;
      return st;
    }
    case QH_CSV_K_TIMESTAMP: {
      long long v = 0;
      const int st = pairs ? QH_CSV_R_TIMESTAMP : qh_csv_parse_timestamp(p, len, c.a, &v);
      ((long long*)c.values)[row] = st == QH_CSV_OK ? v : 0;
      return st;
    }
    default:
      // a quote inside a number: no spelling of the strict grammar; the parser sees the raw bytes, so it is not asked
      if (pairs) { qh_csv_parse_store(c, p, 0, row, filepos); return qh_csv_kind_reason(c.kind); }
      return qh_csv_parse_store(c, p, len, row, filepos);
  }
}

// ---- one record at level 2: as qh_csv_decode_record, with fields that may stand in quotes. A field is canonical when it
// holds no quote byte, or begins and ends with one and every quote in between is half of a doubled pair; anything else is
// QH_CSV_R_QUOTING, in projected and unprojected fields alike (where the next field begins depends on it), and ends the walk.
// One state bit (`open`): a delimiter inside quotes is data. A record that the splitter cut at a line end inside a quoted
// field ends with the bit still set: an unterminated quote, QH_CSV_R_QUOTING. quote < 0: no byte is a quote.
// bit k of *true_mask: descriptor k is a Boolean column and the row's value is true.
QH_CSV_HD inline int qh_csv_decode_record_q(const qh_csv_col* cols, int ncols, unsigned nfields, unsigned char delim, int quote, const unsigned char* p,
                                            unsigned long long len, unsigned long long row, unsigned long long filepos,
                                            unsigned long long* valid_mask, unsigned long long* true_mask) {
  unsigned long long vm = 0, tm = 0;
  int reason = QH_CSV_OK;
  unsigned f = 0;
  int k = 0;
  unsigned long long a = 0;
  *valid_mask = 0;
  *true_mask = 0;
  for (;;) {
    unsigned long long b = a, va = a, vb, pairs = 0;
    if (a < len && (int)p[a] == quote) {
      bool open = true;
      b = a + 1;
      while (b < len) {
        if ((int)p[b] == quote) {
          if (b + 1 < len && (int)p[b + 1] == quote) { ++pairs; b += 2; continue; }
          open = false;
          break;
        }
        ++b;
      }
      if (open) return QH_CSV_R_QUOTING;                       // no closing quote
      va = a + 1; vb = b;
      ++b;
      if (b < len && p[b] != delim) return QH_CSV_R_QUOTING;   // bytes behind the closing quote
    } else {
      bool seen = false;
      while (b < len && p[b] != delim) { seen |= (int)p[b] == quote; ++b; }
      if (seen) return QH_CSV_R_QUOTING;                       // a quote inside a field that does not begin with one
      vb = b;
    }
    while (k < ncols && cols[k].field == f) {
      int truth = 0;
      const int st = qh_csv_parse_store_q(cols[k], p + va, vb - va, pairs, row, filepos + va, &truth);
      if (st == QH_CSV_OK) { vm |= 1ULL << k; if (truth) tm |= 1ULL << k; }
      else if (st != QH_CSV_NULL && reason == QH_CSV_OK) reason = st;
      ++k;
    }
    ++f;
    if (b >= len) break;
    a = b + 1;
    if (f > nfields) break;
  }
  *valid_mask = vm;
  *true_mask = tm;
  if (f != nfields) return QH_CSV_R_FIELD_COUNT;
  return reason;
}

// ---- the undoubling copy's lane logic (k_csv_copy_utf8 at level 2). The wavefront takes a field's raw inner bytes 64 at a
// time; `quotes` is the ballot of "my byte is the quote". Quotes come in runs: inside a run the bytes at odd distance from
// its beginning are the second halves of pairs and are dropped. A run may cross the 64-byte steps: `carry` is how many
// quotes (mod 2) of the run that reaches into this step stand in earlier steps (0 when the previous step's last byte was
// no quote, and at the field's beginning).
QH_CSV_HD inline bool qh_csv_undouble_drops(unsigned long long quotes, unsigned carry, int lane) {
  if (!((quotes >> lane) & 1ULL)) return false;
  const unsigned long long below = ~quotes & ((1ULL << lane) - 1ULL);   // the bytes below mine that are no quotes
  unsigned dist;                                                          // my distance from the run's beginning
  if (below == 0) dist = (unsigned)lane + carry;
  else dist = (unsigned)lane - (unsigned)(64 - __builtin_clzll(below));
  return (dist & 1u) != 0;
}
// the carry for the next step
QH_CSV_HD inline unsigned qh_csv_undouble_carry(unsigned long long quotes, unsigned carry) {
  if (!(quotes >> 63)) return 0u;
  if (~quotes == 0ULL) return carry;                 // 64 quotes: an even number more
  return (unsigned)__builtin_clzll(~quotes) & 1u;    // the run at the top began inside this step
}
// where a lane that keeps its byte writes it, counted from the field's first output byte: `emitted` bytes left the earlier
// steps, `dropped` is the ballot of qh_csv_undouble_drops over this step
QH_CSV_HD inline unsigned long long qh_csv_undouble_out(unsigned long long emitted, unsigned long long dropped, int lane) {
  return emitted + (unsigned long long)__builtin_popcountll(~dropped & ((1ULL << lane) - 1ULL));
}
