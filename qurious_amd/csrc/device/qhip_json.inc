// qhip_json.inc — per-record code of the device decoder for newline-delimited JSON (json.cpp qhip_table_from_json,
// kernels_json.hip): the walk over one object and the lane logic of the copy that removes backslash escapes (DESIGN §3.10). A file
// is either decoded EXACTLY as Arrow C++'s JSON reader with an explicit schema decodes it, or the walk raises a "needs host" reason
// and the whole call answers QHIP_UNSUPPORTED: the device path never imitates a lenient reading or an error message.
//
// One text for two compilers, as qhip_csv.inc, whose strict value parsers it uses as they are: included by kernels_json.hip for
// hipcc and, as plain host C++, by tests/cpp/json_tests.cpp. Every function reads exactly the bytes [p, p + len) it is given.
#include "qhip_csv.inc"

#define QH_JSON_MAX_FIELDS 64
// the key names travel inside the kernel argument, next to the descriptors: together they stay below 4 KB
#define QH_JSON_MAX_NAME_BYTES 1984

// outcome of a record: QH_CSV_OK, or the reason the file needs the host path. The splitter's reasons (k_csv_scan with no quote
// byte) keep their CSV numbers; so do the value reasons that mean the same thing.
#define QH_JSON_R_LONE_CR QH_CSV_R_LONE_CR          // 3
#define QH_JSON_R_EMPTY_LINE QH_CSV_R_EMPTY_LINE    // 4
#define QH_JSON_R_SYNTAX 5         // not exactly one object on the line: a cut record, a blank line, a trailing comma, bytes behind '}'
#define QH_JSON_R_INT QH_CSV_R_INT                  // 6
#define QH_JSON_R_DATE QH_CSV_R_DATE                // 7
#define QH_JSON_R_DECIMAL QH_CSV_R_DECIMAL          // 8
#define QH_JSON_R_FLOAT QH_CSV_R_FLOAT              // 9
#define QH_JSON_R_UTF8 QH_CSV_R_UTF8                // 10
#define QH_JSON_R_UTF8_LONG QH_CSV_R_UTF8_LONG      // 11
#define QH_JSON_R_KEY_ESCAPE 12    // a key that holds a backslash
// (13, CSV's Boolean reason, is not raised here: a literal is true, false, null or a syntax error)
#define QH_JSON_R_TIMESTAMP QH_CSV_R_TIMESTAMP      // 14
#define QH_JSON_R_KEY_UNKNOWN 15   // a key that is not in the schema
#define QH_JSON_R_KEY_TWICE 16     // a key that occurs twice in a record
#define QH_JSON_R_NESTED 17        // a value that begins with '{' or '['
#define QH_JSON_R_UESCAPE 18       // a \uXXXX escape: the next grammar level
#define QH_JSON_R_ESCAPE 19        // any other byte behind a backslash than " \ / b f n r t
#define QH_JSON_R_CONTROL 20       // a raw byte below 0x20 inside a string
#define QH_JSON_R_KIND 21          // a string where the column's type wants a number, and so on

QH_CSV_HD inline const char* qh_json_reason_text(unsigned r) {
  switch (r) {
    case QH_JSON_R_LONE_CR: return "a carriage return that is not followed by a line feed";
    case QH_JSON_R_EMPTY_LINE: return "an empty line";
    case QH_JSON_R_SYNTAX: return "a line that is not exactly one complete object";
    case QH_JSON_R_INT: return "an integer outside -?(0|[1-9][0-9]*) or outside its type's range";
    case QH_JSON_R_DATE: return "a date that is not an integer number of days";
    case QH_JSON_R_DECIMAL: return "a decimal with an exponent or outside its precision and scale";
    case QH_JSON_R_FLOAT: return "a float outside the exactly convertible spellings";
    case QH_JSON_R_UTF8: return "invalid UTF-8";
    case QH_JSON_R_UTF8_LONG: return "a string value of 2 GiB or more";
    case QH_JSON_R_KEY_ESCAPE: return "a key with a backslash escape";
    case QH_JSON_R_TIMESTAMP: return "a timestamp outside YYYY-MM-DD[ T]hh:mm:ss[.fraction] or outside its unit's range";
    case QH_JSON_R_KEY_UNKNOWN: return "a key that the schema does not hold";
    case QH_JSON_R_KEY_TWICE: return "a key that occurs twice";
    case QH_JSON_R_NESTED: return "a nested object or array";
    case QH_JSON_R_UESCAPE: return "a \\u escape";
    case QH_JSON_R_ESCAPE: return "an unknown backslash escape";
    case QH_JSON_R_CONTROL: return "a control character inside a string";
    case QH_JSON_R_KIND: return "a value of another JSON kind than its column's type";
    default: return "an unknown reason";
  }
}

// ---- descriptors: what the decode kernel is driven by, one kernel argument. Every schema field has a `field` entry (its value
// is validated whether it is projected or not); the projected ones name their output column, whose buffers are in `out`.
struct qh_json_out {
  void* values;                  // as qh_csv_col: row-indexed values; Utf8: the u32 unescaped LENGTH of every row; Boolean: ballot words
  unsigned long long* valid;     // one ballot word per 64 rows (written by the kernel)
  unsigned long long* strpos;    // Utf8: where the first inner byte stands in the file, and QH_JSON_POS_*
};
struct qh_json_field {
  unsigned short name_off, name_len;   // the key inside `names`
  unsigned char kind;                  // QH_CSV_K_*
  signed char col;                     // index into `out`, -1: not projected
  unsigned char a, b;                  // Int: a = signed, b = bytes; Decimal128: a = precision, b = scale; Timestamp: a = fraction digits
};
struct qh_json_desc {
  qh_json_out out[QH_JSON_MAX_FIELDS];
  qh_json_field field[QH_JSON_MAX_FIELDS];
  unsigned char names[QH_JSON_MAX_NAME_BYTES];
};

// ---- Utf8: bits 63 and 62 of strpos[row], as at CSV grammar level 2
#define QH_JSON_POS_ESC (1ULL << 63)    // the value holds backslash escapes: the copy removes them
#define QH_JSON_POS_LONG (1ULL << 62)   // ... and its raw inner span is longer than 64 bytes: the whole wavefront copies it
#define QH_JSON_POS_MASK ((1ULL << 62) - 1ULL)

QH_CSV_HD inline bool qh_json_is_blank(unsigned char c) { return c == ' ' || c == '\t'; }

// the byte an escape stands for; 0: none of " \ / b f n r t
QH_CSV_HD inline unsigned char qh_json_unescape_byte(unsigned char e) {
  switch (e) {
    case '"': case '\\': case '/': return e;
    case 'b': return 8;
    case 'f': return 12;
    case 'n': return 10;
    case 'r': return 13;
    case 't': return 9;
    default: return 0;
  }
}

// -?0[0-9]: a number token with a leading zero (JSON has none; the CSV parsers accept them)
QH_CSV_HD inline bool qh_json_leading_zero(const unsigned char* p, unsigned long long len) {
  const unsigned long long i = (len > 0 && p[0] == '-') ? 1 : 0;
  return len - i >= 2 && p[i] == '0' && (unsigned)p[i + 1] - (unsigned)'0' <= 9u;
}

QH_CSV_HD inline bool qh_json_key_is(const qh_json_desc& d, unsigned f, const unsigned char* key, unsigned long long klen) {
  if (d.field[f].name_len != klen) return false;
  const unsigned char* name = d.names + d.field[f].name_off;
  for (unsigned long long i = 0; i < klen; ++i)
    if (name[i] != key[i]) return false;
  return true;
}

QH_CSV_HD inline void qh_json_store_int(void* values, unsigned long long row, int width, unsigned long long v) {
  switch (width) {
    case 1: ((unsigned char*)values)[row] = (unsigned char)v; break;
    case 2: ((unsigned short*)values)[row] = (unsigned short)v; break;
    case 4: ((unsigned*)values)[row] = (unsigned)v; break;
    default: ((unsigned long long*)values)[row] = v; break;
  }
}

// a NULL row (the literal null, or a key the record does not hold): zeros, as the CSV decoder leaves them
QH_CSV_HD inline void qh_json_store_null(const qh_json_field& fd, const qh_json_out& o, unsigned long long row) {
  switch (fd.kind) {
    case QH_CSV_K_INT: qh_json_store_int(o.values, row, fd.b, 0ULL); break;
    case QH_CSV_K_DATE32: ((int*)o.values)[row] = 0; break;
    case QH_CSV_K_DECIMAL128: ((unsigned long long*)o.values)[2 * row] = 0; ((unsigned long long*)o.values)[2 * row + 1] = 0; break;
    case QH_CSV_K_FLOAT64: case QH_CSV_K_FLOAT64_FULL: case QH_CSV_K_TIMESTAMP: ((unsigned long long*)o.values)[row] = 0; break;
    case QH_CSV_K_FLOAT32: ((unsigned*)o.values)[row] = 0u; break;
    case QH_CSV_K_UTF8: ((unsigned*)o.values)[row] = 0u; o.strpos[row] = 0ULL; break;
    default: break;   // Boolean: the kernel packs the words
  }
}

// ---- one record: bytes [p, p + len) without its line end, at `filepos` in the file. The grammar:
//   blanks '{' blanks [ pair ( blanks ',' blanks pair )* ] blanks '}' blanks        blanks: ' ' and '\t'
//   pair: '"' key '"' blanks ':' blanks value      key: no backslash, no byte below 0x20; one of the schema's names, once
//   value: null | true | false | a number token | '"' string '"'; a string ends at the first '"' behind an even number of backslashes
// EVERY value is validated by its field's type, projected or not (the host converts every column and refuses the file on a
// bad one); only the stores are left out for a field without an output column. Returns QH_CSV_OK or the record's first
// needs-host reason. bit c of *valid_mask: output column c got a value; of *true_mask: ... a Boolean one, and it is true.
QH_CSV_HD inline int qh_json_decode_record(const qh_json_desc& d, unsigned nfields, const unsigned char* p, unsigned long long len,
                                           unsigned long long row, unsigned long long filepos, unsigned long long* valid_mask,
                                           unsigned long long* true_mask) {
  unsigned long long vm = 0, tm = 0, seen = 0;
  *valid_mask = 0;
  *true_mask = 0;
  unsigned long long i = 0;
  unsigned next = 0;   // the field behind the last matched one: records usually keep one key order
  while (i < len && qh_json_is_blank(p[i])) ++i;
  if (i >= len || p[i] != '{') return QH_JSON_R_SYNTAX;
  ++i;
  while (i < len && qh_json_is_blank(p[i])) ++i;
  if (i < len && p[i] == '}') {
    ++i;
  } else {
    for (;;) {
      // ---- the key
      if (i >= len || p[i] != '"') return QH_JSON_R_SYNTAX;
      const unsigned long long ka = ++i;
      while (i < len && p[i] != '"') {
        if (p[i] == '\\') return QH_JSON_R_KEY_ESCAPE;
        if (p[i] < 0x20u) return QH_JSON_R_CONTROL;
        ++i;
      }
      if (i >= len) return QH_JSON_R_SYNTAX;
      const unsigned long long klen = i - ka;
      ++i;
      unsigned f = nfields;
      if (next < nfields && qh_json_key_is(d, next, p + ka, klen)) f = next;
      else
        for (unsigned g = 0; g < nfields; ++g)
          if (qh_json_key_is(d, g, p + ka, klen)) { f = g; break; }
      if (f >= nfields) return QH_JSON_R_KEY_UNKNOWN;
      if ((seen >> f) & 1ULL) return QH_JSON_R_KEY_TWICE;
      seen |= 1ULL << f;
      next = f + 1;
      while (i < len && qh_json_is_blank(p[i])) ++i;
      if (i >= len || p[i] != ':') return QH_JSON_R_SYNTAX;
      ++i;
      while (i < len && qh_json_is_blank(p[i])) ++i;
      if (i >= len) return QH_JSON_R_SYNTAX;
      // ---- the value
      const qh_json_field fd = d.field[f];
      const int col = fd.col;
      const unsigned char c0 = p[i];
      if (c0 == '"') {
        const unsigned long long a = ++i;
        unsigned long long nesc = 0;
        int bad = QH_CSV_OK;
        while (i < len) {
          const unsigned char c = p[i];
          if (c == '"') break;
          if (c == '\\') {
            if (i + 1 >= len) return QH_JSON_R_SYNTAX;   // the record is cut behind the backslash
            const unsigned char e = p[i + 1];
            if (bad == QH_CSV_OK && qh_json_unescape_byte(e) == 0) bad = e == 'u' ? QH_JSON_R_UESCAPE : QH_JSON_R_ESCAPE;
            ++nesc;
            i += 2;
            continue;
          }
          if (c < 0x20u && bad == QH_CSV_OK) bad = QH_JSON_R_CONTROL;
          ++i;
        }
        if (i >= len) return QH_JSON_R_SYNTAX;           // no closing quote: a raw line end inside a string cuts the record
        const unsigned long long b = i;
        ++i;
        if (fd.kind == QH_CSV_K_UTF8) {
          if (bad != QH_CSV_OK) return bad;
          const unsigned long long ulen = b - a - nesc;   // the unescaped length: what the offsets and byte totals are made of
          if (ulen > 0x7fffffffULL) return QH_JSON_R_UTF8_LONG;
          // (an escape and the byte it stands for are ASCII: removing the introducers leaves validity as it is)
          if (qh_csv_check_utf8(p + a, b - a) != QH_CSV_OK) return QH_JSON_R_UTF8;
          if (col >= 0) {
            ((unsigned*)d.out[col].values)[row] = (unsigned)ulen;
            d.out[col].strpos[row] = (filepos + a) | (nesc ? QH_JSON_POS_ESC | (b - a > 64 ? QH_JSON_POS_LONG : 0ULL) : 0ULL);
            vm |= 1ULL << col;
          }
        } else if (fd.kind == QH_CSV_K_TIMESTAMP) {
          // (a backslash is no byte of the grammar: a string with an escape fails in the parser)
          long long v = 0;
          if (b == a || qh_csv_parse_timestamp(p + a, b - a, fd.a, &v) != QH_CSV_OK) return QH_JSON_R_TIMESTAMP;
          if (col >= 0) { ((long long*)d.out[col].values)[row] = v; vm |= 1ULL << col; }
        } else if (fd.kind == QH_CSV_K_DECIMAL128) {
          unsigned long long v[2] = {0, 0};
          if (b == a || qh_csv_parse_decimal128(p + a, b - a, fd.a, fd.b, v) != QH_CSV_OK) return QH_JSON_R_DECIMAL;
          if (col >= 0) {
            unsigned long long* o = (unsigned long long*)d.out[col].values + 2 * row;
            o[0] = v[0]; o[1] = v[1];
            vm |= 1ULL << col;
          }
        } else {
          return QH_JSON_R_KIND;
        }
      } else if (c0 == '{' || c0 == '[') {
        return QH_JSON_R_NESTED;
      } else {
        const unsigned long long a = i;
        while (i < len && p[i] != ',' && p[i] != '}' && !qh_json_is_blank(p[i])) ++i;
        const unsigned long long tl = i - a;
        const unsigned char* t = p + a;
        if (c0 == 'n' || c0 == 't' || c0 == 'f') {
          int truth = 0;
          if (tl == 4 && t[0] == 'n' && t[1] == 'u' && t[2] == 'l' && t[3] == 'l') {
            // NULL for a column of any type
          } else if (qh_csv_parse_bool(t, tl, &truth) == QH_CSV_OK) {
            if (fd.kind != QH_CSV_K_BOOL) return QH_JSON_R_KIND;
            if (col >= 0) { vm |= 1ULL << col; if (truth) tm |= 1ULL << col; }
          } else {
            return QH_JSON_R_SYNTAX;
          }
        } else if (c0 == '-' || (unsigned)c0 - (unsigned)'0' <= 9u) {
          if (fd.kind == QH_CSV_K_INT) {
            unsigned long long v = 0;
            if (qh_json_leading_zero(t, tl) || qh_csv_parse_int(t, tl, fd.b, fd.a, &v) != QH_CSV_OK) return QH_JSON_R_INT;
            if (col >= 0) { qh_json_store_int(d.out[col].values, row, fd.b, v); vm |= 1ULL << col; }
          } else if (fd.kind == QH_CSV_K_DATE32) {
            unsigned long long v = 0;
            if (qh_json_leading_zero(t, tl) || qh_csv_parse_int(t, tl, 4, 1, &v) != QH_CSV_OK) return QH_JSON_R_DATE;
            if (col >= 0) { ((unsigned*)d.out[col].values)[row] = (unsigned)v; vm |= 1ULL << col; }
          } else if (fd.kind == QH_CSV_K_FLOAT64) {
            double v = 0.0;
            if (qh_json_leading_zero(t, tl) || qh_csv_parse_float64(t, tl, &v) != QH_CSV_OK) return QH_JSON_R_FLOAT;
            if (col >= 0) { ((double*)d.out[col].values)[row] = v; vm |= 1ULL << col; }
          } else if (fd.kind == QH_CSV_K_FLOAT64_FULL) {
            unsigned long long v = 0;
            if (qh_json_leading_zero(t, tl) || qh_float_parse<false>(t, tl, true, &v) != QH_CSV_OK) return QH_JSON_R_FLOAT;
            if (col >= 0) { ((unsigned long long*)d.out[col].values)[row] = v; vm |= 1ULL << col; }
          } else if (fd.kind == QH_CSV_K_FLOAT32) {
            unsigned long long v = 0;
            if (qh_json_leading_zero(t, tl) || qh_float_parse<true>(t, tl, true, &v) != QH_CSV_OK) return QH_JSON_R_FLOAT;
            if (col >= 0) { ((unsigned*)d.out[col].values)[row] = (unsigned)v; vm |= 1ULL << col; }
          } else if (fd.kind == QH_CSV_K_DECIMAL128) {
            // a JSON number without exponent: a digit on both sides of the point (the CSV grammar also takes ".5" and "5.")
            unsigned long long v[2] = {0, 0};
            const unsigned char first = t[c0 == '-' && tl > 1 ? 1 : 0];
            if ((unsigned)first - (unsigned)'0' > 9u || t[tl - 1] == '.' || qh_json_leading_zero(t, tl) ||
                qh_csv_parse_decimal128(t, tl, fd.a, fd.b, v) != QH_CSV_OK)
              return QH_JSON_R_DECIMAL;
            if (col >= 0) {
              unsigned long long* o = (unsigned long long*)d.out[col].values + 2 * row;
              o[0] = v[0]; o[1] = v[1];
              vm |= 1ULL << col;
            }
          } else {
            return QH_JSON_R_KIND;
          }
        } else {
          return QH_JSON_R_SYNTAX;
        }
      }
      while (i < len && qh_json_is_blank(p[i])) ++i;
      if (i >= len) return QH_JSON_R_SYNTAX;
      if (p[i] == '}') { ++i; break; }
      if (p[i] != ',') return QH_JSON_R_SYNTAX;
      ++i;
      while (i < len && qh_json_is_blank(p[i])) ++i;
    }
  }
  while (i < len && qh_json_is_blank(p[i])) ++i;
  if (i != len) return QH_JSON_R_SYNTAX;   // bytes behind the object (a second object on the line included)
  for (unsigned f = 0; f < nfields; ++f) {
    const int col = d.field[f].col;
    if (col >= 0 && !((vm >> col) & 1ULL)) qh_json_store_null(d.field[f], d.out[col], row);
  }
  *valid_mask = vm;
  *true_mask = tm;
  return QH_CSV_OK;
}

// ---- the unescaping copy's lane logic (k_json_copy_utf8). The wavefront takes a value's raw inner bytes 64 at a time;
// `slashes` is the ballot of "my byte is a backslash". Backslashes come in runs: inside a run the bytes at EVEN distance from
// its beginning introduce an escape and are dropped, those at odd distance are the escaped backslash itself; the byte behind a
// run of odd length is an escaped byte and is translated. This is the parity machinery of qh_csv_undouble_*, used as it is:
// `carry` is the run's length (mod 2) that stands in earlier steps, qh_csv_undouble_carry makes the next step's, and
// qh_csv_undouble_out tells where a kept byte goes.
QH_CSV_HD inline bool qh_json_unescape_drops(unsigned long long slashes, unsigned carry, int lane) {
  return ((slashes >> lane) & 1ULL) && !qh_csv_undouble_drops(slashes, carry, lane);
}
// is lane's byte the one behind an introducer? `dropped`: the ballot of qh_json_unescape_drops over this step
QH_CSV_HD inline bool qh_json_unescape_escaped(unsigned long long dropped, unsigned carry, int lane) {
  return lane ? ((dropped >> (lane - 1)) & 1ULL) != 0 : carry != 0;
}
