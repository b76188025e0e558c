// float_parse_tests.cpp — the float parsers of float_parse level 2 on the host (qurious_amd/csrc/device/qhip_float.inc through
// qhip_csv.inc and qhip_json.inc as plain C++): the very functions kernels_csv.hip and kernels_json.hip call, against glibc's
// strtod / strtof in the same process, bit for bit. tests/test_float_parse_cpu.py drives it and holds the expectations that come
// from Python and pyarrow.
//
//   float_parse_tests table                   the 651 table entries, "high low" in hex, one per line
//   float_parse_tests parse f64|f32 <file>    one field per line -> its bits in hex, N (an empty field) or R<reason>
//   float_parse_tests diff64 <n> <seed>       %.17g of n random finite Float64 bit patterns: none refused, all equal to strtod
//   float_parse_tests diff32 <n> <seed>       %.9g of n random finite Float32 bit patterns: equal to strtof; refused only when that is 0 or inf
//   float_parse_tests digits <n> <seed>       n random digit strings (1 .. 40 digits, a point and an exponent at random), as Float64
//                                             and as Float32: equal to strtod / strtof, or refused for a reason strtod confirms
//   float_parse_tests clinger <n> <seed>      n random inputs that qh_csv_parse_float64 accepts: the same bits from qh_parse_float64_full
//   float_parse_tests csv <file> <types> <grammar 1|2> <projection | ->       the record walks of the CSV decoder (header, ',' and '"')
//   float_parse_tests json <file> <names> <types> <projection | ->            ... and of the JSON decoder
//     types: f64 (QH_CSV_K_FLOAT64_FULL), f32 (QH_CSV_K_FLOAT32), f64c (QH_CSV_K_FLOAT64, level 1), i64
//     dump: "ROWS n", then a row per line, tab-separated: hex bits, a decimal integer, N; or "NEEDS_HOST reason record"
//
// A refusal is confirmed by what strtod says about the same text (`digits`): the nearest value is zero or infinite; or the text
// has more than 19 significant digits and its 19-digit truncation m and m + 1, spelled out and given to strtod with the same
// power of ten, give different values (or both zero / both infinite). Anything else is a failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device/qhip_json.inc"

static const size_t kSlack = 64;

static uint64_t g_rng;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static uint64_t bits64(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
static uint32_t bits32(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }

// the parsers on an exactly sized copy: the sanitizers see a read outside [p, p + len)
static int parse64(const std::string& s, uint64_t* bits) {
  unsigned char* p = (unsigned char*)malloc(s.size() ? s.size() : 1);
  memcpy(p, s.data(), s.size());
  double v = 0;
  const int st = qh_parse_float64_full(p, s.size(), &v);
  free(p);
  *bits = bits64(v);
  return st;
}
static int parse32(const std::string& s, uint32_t* bits) {
  unsigned char* p = (unsigned char*)malloc(s.size() ? s.size() : 1);
  memcpy(p, s.data(), s.size());
  float v = 0;
  const int st = qh_parse_float32_full(p, s.size(), &v);
  free(p);
  *bits = bits32(v);
  return st;
}

static int run_table() {
  for (int q = QH_POW5_Q_MIN; q <= QH_POW5_Q_MAX; ++q)
    printf("%016llx %016llx\n", qh_pow5_128[2 * (q - QH_POW5_Q_MIN)], qh_pow5_128[2 * (q - QH_POW5_Q_MIN) + 1]);
  return 0;
}

static int run_parse(bool f32, const char* path) {
  FILE* in = fopen(path, "rb");
  if (!in) { perror(path); return 2; }
  std::string all;
  char chunk[65536];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, in)) > 0) all.append(chunk, got);
  fclose(in);
  size_t a = 0;
  while (a < all.size()) {
    size_t b = all.find('\n', a);
    if (b == std::string::npos) b = all.size();
    const std::string field = all.substr(a, b - a);
    uint64_t b64 = 0;
    uint32_t b32 = 0;
    const int st = f32 ? parse32(field, &b32) : parse64(field, &b64);
    if (st == QH_CSV_NULL) printf("N\n");
    else if (st != QH_CSV_OK) printf("R%d\n", st);
    else if (f32) printf("%08x\n", b32);
    else printf("%016llx\n", (unsigned long long)b64);
    a = b + 1;
  }
  return 0;
}

static int run_diff64(long n) {
  char text[64];
  for (long k = 0; k < n; ++k) {
    uint64_t b = rnd();
    if (((b >> 52) & 0x7FF) == 0x7FF) b &= ~(1ULL << 62);   // finite
    if (k % 16 == 0) b &= ~(0x7FFULL << 52);                // one in 16 a subnormal (or zero)
    double v;
    memcpy(&v, &b, 8);
    snprintf(text, sizeof text, "%.17g", v);
    uint64_t got = 0;
    const int st = parse64(text, &got);
    if (st != QH_CSV_OK) { printf("REFUSED %s reason %d\n", text, st); return 1; }
    if (got != b || got != bits64(strtod(text, nullptr))) { printf("MISMATCH %s got %016llx want %016llx\n", text, (unsigned long long)got, (unsigned long long)b); return 1; }
  }
  printf("DIFF64 OK %ld\n", n);
  return 0;
}

static int run_diff32(long n) {
  char text[64];
  long refused = 0;
  for (long k = 0; k < n; ++k) {
    uint32_t b = (uint32_t)rnd();
    if (((b >> 23) & 0xFF) == 0xFF) b &= ~(1u << 30);
    if (k % 16 == 0) b &= ~(0xFFu << 23);
    float v;
    memcpy(&v, &b, 4);
    snprintf(text, sizeof text, "%.9g", (double)v);
    const float want = strtof(text, nullptr);
    uint32_t got = 0;
    const int st = parse32(text, &got);
    if (st != QH_CSV_OK) {
      // a zero's spelling is a zero decimal and is never refused: only a nonzero decimal that rounds to 0 or inf may be
      if (st == QH_CSV_R_FLOAT && (want == 0.0f || std::isinf(want)) && v != 0.0f) { ++refused; continue; }
      printf("REFUSED %s reason %d\n", text, st);
      return 1;
    }
    if (got != bits32(want) || got != b) { printf("MISMATCH %s got %08x want %08x\n", text, got, bits32(want)); return 1; }
  }
  printf("DIFF32 OK %ld refused %ld\n", n, refused);
  return 0;
}

// ---- random digit strings. The generator also knows what it wrote: the significant digits and the power of ten of the last one.
struct Digits {
  std::string text;
  std::string sig;     // the digits from the first nonzero one on (empty: the decimal is zero)
  long long q;         // the decimal is sig * 10^q
};
static Digits random_digits() {
  Digits d;
  const int nd = 1 + (int)below(40);
  std::string digs;
  // short runs of zeros at either end now and then, so that leading and trailing zeros meet the 19-digit budget
  const int lead = below(4) == 0 ? (int)below((uint64_t)nd) : 0;
  const int trail = below(4) == 0 ? (int)below((uint64_t)(nd - lead) + 1) : 0;
  for (int k = 0; k < nd; ++k) digs.push_back(k < lead || k >= nd - trail ? '0' : (char)('0' + below(10)));
  const bool neg = below(2) == 0;
  const int point = below(3) == 0 ? nd : 1 + (int)below((uint64_t)nd);   // digits in front of the point (nd: no point)
  long long e = 0;
  const bool has_e = below(4) != 0;
  // the magnitude of the value: mostly inside Float64's or Float32's range, sometimes at or beyond either end
  const int mode = (int)below(8);
  if (has_e) {
    const long long centre = mode == 0 ? 308 : mode == 1 ? -324 : mode == 2 ? 38 : mode == 3 ? -45 : mode == 4 ? 0 : (long long)below(700) - 350;
    e = centre - (point - 1) + (long long)below(7) - 3;
    if (mode == 4) e = (long long)below(45) - 22;
  }
  if (neg) d.text.push_back('-');
  d.text.append(digs, 0, (size_t)point);
  if (point < nd) { d.text.push_back('.'); d.text.append(digs, (size_t)point, std::string::npos); }
  if (has_e) {
    d.text.push_back(below(2) ? 'e' : 'E');
    if (e < 0) d.text.push_back('-'); else if (below(2)) d.text.push_back('+');
    if (below(8) == 0) d.text.append((size_t)below(25), '0');   // leading zeros of the exponent
    d.text += std::to_string(e < 0 ? -e : e);
  }
  size_t first = digs.find_first_not_of('0');
  d.sig = first == std::string::npos ? "" : digs.substr(first);
  d.q = e - (nd - point);
  return d;
}

// is the refusal of d one of the documented classes? F: double with strtod, float with strtof
template <typename F, F (*CONV)(const char*, char**)>
static const char* refusal_class(const Digits& d) {
  if (d.sig.empty()) return nullptr;   // a zero decimal is never refused
  size_t last = d.sig.find_last_not_of('0');
  const F whole = CONV(d.text.c_str(), nullptr);
  if (last + 1 <= 19) return (whole == 0 || std::isinf(whole)) ? "range" : nullptr;
  // more than 19 significant digits: the bounds, spelled out
  std::string lo = d.sig.substr(0, 19), hi = lo;
  int k = 18;
  while (k >= 0 && hi[(size_t)k] == '9') hi[(size_t)k--] = '0';
  if (k >= 0) ++hi[(size_t)k]; else hi = "1" + hi;
  const std::string tail = "e" + std::to_string(d.q + (long long)d.sig.size() - 19);
  const F a = CONV((lo + tail).c_str(), nullptr), b = CONV((hi + tail).c_str(), nullptr);
  if (bits64((double)a) != bits64((double)b)) return "long";
  return (a == 0 || std::isinf(a)) ? "range" : nullptr;
}

static int run_digits(long n) {
  long accepted = 0, range = 0, longs = 0;
  for (long k = 0; k < n; ++k) {
    const Digits d = random_digits();
    for (int f32 = 0; f32 < 2; ++f32) {
      int st;
      bool same;
      if (f32) { uint32_t got = 0; st = parse32(d.text, &got); same = got == bits32(strtof(d.text.c_str(), nullptr)); }
      else { uint64_t got = 0; st = parse64(d.text, &got); same = got == bits64(strtod(d.text.c_str(), nullptr)); }
      if (st == QH_CSV_OK) {
        if (!same) { printf("MISMATCH %s as %s\n", d.text.c_str(), f32 ? "f32" : "f64"); return 1; }
        ++accepted;
        continue;
      }
      const char* cls = st != QH_CSV_R_FLOAT ? nullptr : f32 ? refusal_class<float, strtof>(d) : refusal_class<double, strtod>(d);
      if (!cls) { printf("REFUSED %s as %s reason %d: in none of the classes\n", d.text.c_str(), f32 ? "f32" : "f64", st); return 1; }
      if (cls[0] == 'r') ++range; else ++longs;
    }
  }
  printf("DIGITS OK %ld accepted %ld range %ld long %ld\n", n, accepted, range, longs);
  return 0;
}

static int run_clinger(long n) {
  long done = 0;
  while (done < n) {
    const int nd = 1 + (int)below(17);
    std::string digs;
    for (int k = 0; k < nd; ++k) digs.push_back((char)('0' + below(10)));
    const int point = below(3) == 0 ? nd : 1 + (int)below((uint64_t)nd);
    std::string text = below(2) ? "-" : "";
    text.append(digs, 0, (size_t)point);
    if (point < nd) { text.push_back('.'); text.append(digs, (size_t)point, std::string::npos); }
    if (below(2)) {
      const long long e = (long long)below(45) - 22 + (nd - point);
      text += below(2) ? "e" : "E";
      text += e < 0 ? "-" : below(2) ? "+" : "";
      text += std::to_string(e < 0 ? -e : e);
    }
    double old = 0;
    if (qh_csv_parse_float64((const unsigned char*)text.data(), text.size(), &old) != QH_CSV_OK) continue;
    uint64_t got = 0;
    if (parse64(text, &got) != QH_CSV_OK || got != bits64(old)) { printf("MISMATCH %s old %016llx new %016llx\n", text.c_str(), (unsigned long long)bits64(old), (unsigned long long)got); return 1; }
    ++done;
  }
  printf("CLINGER OK %ld\n", done);
  return 0;
}

// ---- the record walks
struct Spec { int kind; int width; };
static bool parse_type(const std::string& s, Spec& o) {
  if (s == "f64") { o = Spec{QH_CSV_K_FLOAT64_FULL, 8}; return true; }
  if (s == "f64c") { o = Spec{QH_CSV_K_FLOAT64, 8}; return true; }
  if (s == "f32") { o = Spec{QH_CSV_K_FLOAT32, 4}; return true; }
  if (s == "i64") { o = Spec{QH_CSV_K_INT, 8}; return true; }
  return false;
}
static std::vector<std::string> split(const std::string& s, char d) {
  std::vector<std::string> out;
  size_t a = 0;
  for (;;) {
    const size_t b = s.find(d, a);
    out.push_back(s.substr(a, b == std::string::npos ? b : b - a));
    if (b == std::string::npos) break;
    a = b + 1;
  }
  return out;
}
static void print_cell(const Spec& sp, const void* values, size_t r) {
  if (sp.width == 4) printf("%08x", ((const unsigned*)values)[r]);
  else if (sp.kind == QH_CSV_K_INT) printf("%lld", ((const long long*)values)[r]);
  else printf("%016llx", ((const unsigned long long*)values)[r]);
}

static int run_file(bool json, int argc, char** argv) {
  // csv: file types grammar projection          json: file names types projection
  const char* path = argv[0];
  std::vector<std::string> names;
  if (json) names = split(argv[1], ',');
  std::vector<Spec> fields;
  for (const std::string& s : split(argv[json ? 2 : 1], ',')) {
    Spec sp;
    if (!parse_type(s, sp)) { fprintf(stderr, "bad type %s\n", s.c_str()); return 2; }
    fields.push_back(sp);
  }
  const int grammar = json ? 0 : atoi(argv[2]);
  std::vector<int> proj;
  if (strcmp(argv[3], "-") == 0) for (size_t k = 0; k < fields.size(); ++k) proj.push_back((int)k);
  else for (const std::string& s : split(argv[3], ',')) proj.push_back(atoi(s.c_str()));
  (void)argc;

  FILE* in = fopen(path, "rb");
  if (!in) { perror(path); return 2; }
  fseek(in, 0, SEEK_END);
  const size_t n = (size_t)ftell(in);
  fseek(in, 0, SEEK_SET);
  unsigned char* buf = (unsigned char*)malloc(n + kSlack);
  if (n && fread(buf, 1, n, in) != n) { perror("read"); return 2; }
  fclose(in);
  memset(buf + n, 0xAB, kSlack);
  size_t d0 = 0;
  if (!json) {   // the header
    const unsigned char* nl = (const unsigned char*)memchr(buf, '\n', n);
    d0 = nl ? (size_t)(nl - buf) + 1 : n;
  }
  std::vector<unsigned long long> starts;
  starts.push_back(d0);
  for (size_t i = d0; i < n; ++i) if (buf[i] == '\n') starts.push_back(i + 1);
  if (n > d0 && buf[n - 1] != '\n') starts.push_back(n + 1);
  const size_t R = starts.size() - 1;

  // descriptors ascending by field (the CSV walk wants them so); at[k]: where output column k stands among them
  std::vector<int> order(proj.size());
  for (size_t k = 0; k < proj.size(); ++k) order[k] = (int)k;
  if (!json)
    for (size_t i = 1; i < order.size(); ++i)
      for (size_t j = i; j > 0 && proj[(size_t)order[j]] < proj[(size_t)order[j - 1]]; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
  std::vector<size_t> at(proj.size());
  for (size_t j = 0; j < order.size(); ++j) at[(size_t)order[j]] = j;
  std::vector<void*> values(order.size());
  std::vector<std::vector<unsigned char>> valid(order.size(), std::vector<unsigned char>(R, 0));
  for (size_t j = 0; j < order.size(); ++j) values[j] = malloc(R * (size_t)fields[(size_t)proj[(size_t)order[j]]].width + kSlack);
  std::vector<qh_csv_col> cdesc(order.size());
  qh_json_desc* jdesc = (qh_json_desc*)calloc(1, sizeof(qh_json_desc));
  if (json) {
    size_t name_bytes = 0;
    for (size_t f = 0; f < fields.size(); ++f) {
      qh_json_field& d = jdesc->field[f];
      d.name_off = (unsigned short)name_bytes; d.name_len = (unsigned short)names[f].size();
      memcpy(jdesc->names + name_bytes, names[f].data(), names[f].size());
      name_bytes += names[f].size();
      d.kind = (unsigned char)fields[f].kind; d.col = -1; d.a = 1; d.b = (unsigned char)fields[f].width;
    }
    for (size_t k = 0; k < proj.size(); ++k) { jdesc->field[proj[k]].col = (signed char)k; jdesc->out[k].values = values[k]; }
  } else {
    for (size_t j = 0; j < order.size(); ++j) {
      const Spec& sp = fields[(size_t)proj[(size_t)order[j]]];
      qh_csv_col& d = cdesc[j];
      memset(&d, 0, sizeof d);
      d.values = values[j];
      d.field = (unsigned)proj[(size_t)order[j]];
      d.kind = (unsigned char)sp.kind; d.width = (unsigned char)sp.width; d.a = 1;
    }
  }
  int rc = 0;
  for (size_t r = 0; r < R && rc == 0; ++r) {
    const size_t s = (size_t)starts[r];
    size_t len = (size_t)starts[r + 1] - 1 - s;
    if (len > 0 && buf[s + len - 1] == '\r') --len;
    unsigned long long vm = 0, tm = 0;
    int reason;
    if (json) reason = qh_json_decode_record(*jdesc, (unsigned)fields.size(), buf + s, len, r, s, &vm, &tm);
    else if (grammar == 1) reason = qh_csv_decode_record(cdesc.data(), (int)cdesc.size(), (unsigned)fields.size(), ',', buf + s, len, r, s, &vm);
    else reason = qh_csv_decode_record_q(cdesc.data(), (int)cdesc.size(), (unsigned)fields.size(), ',', '"', buf + s, len, r, s, &vm, &tm);
    if (reason != QH_CSV_OK) { printf("NEEDS_HOST %d %zu\n", reason, r + 1); rc = 1; }
    for (size_t j = 0; j < order.size(); ++j) valid[j][r] = (unsigned char)((vm >> j) & 1);
  }
  if (rc == 0) {
    printf("ROWS %zu\n", R);
    for (size_t r = 0; r < R; ++r) {
      for (size_t k = 0; k < proj.size(); ++k) {
        const size_t j = at[k];
        if (k) fputc('\t', stdout);
        if (!valid[j][r]) { fputc('N', stdout); continue; }
        print_cell(fields[(size_t)proj[k]], values[j], r);
      }
      fputc('\n', stdout);
    }
  }
  for (void* v : values) free(v);
  free(jdesc);
  free(buf);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "table" && argc == 2) return run_table();
  if (mode == "parse" && argc == 4) return run_parse(strcmp(argv[2], "f32") == 0, argv[3]);
  if ((mode == "diff64" || mode == "diff32" || mode == "digits" || mode == "clinger") && argc == 4) {
    const long n = atol(argv[2]);
    g_rng = strtoull(argv[3], nullptr, 10);
    return mode == "diff64" ? run_diff64(n) : mode == "diff32" ? run_diff32(n) : mode == "digits" ? run_digits(n) : run_clinger(n);
  }
  if ((mode == "csv" || mode == "json") && argc == 6) return run_file(mode == "json", argc - 2, argv + 2);
  fprintf(stderr, "usage: float_parse_tests table | parse f64|f32 file | diff64|diff32|digits|clinger n seed | csv file types grammar projection | json file names types projection\n");
  return 2;
}
