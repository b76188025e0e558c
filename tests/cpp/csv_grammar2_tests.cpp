// csv_grammar2_tests.cpp — grammar level 2 of the device CSV decoder on the host (qurious_amd/csrc/device/qhip_csv.inc as plain
// C++): the quote-aware record walk, the Boolean and Timestamp parsers and the undoubling copy's lane logic, the very functions
// kernels_csv.hip calls. tests/test_csv_grammar2_cpu.py compares the dump with pyarrow on the same bytes.
//
//   csv_grammar2_tests decode <file> <types> <has_header 0|1> <delimiter byte> <quote byte | -1> <projection | ->  > dump
//     types: csv_tests' (i8 .. u64 f64 date utf8 dec:P:S) and bool, ts0 ts3 ts6 ts9 (Timestamp with that many fraction digits)
//   csv_grammar2_tests undouble      runs of 1..130 quotes at every offset 0..129: the wavefront's copy against a byte-serial one
//
// Dump: as csv_tests'; a Boolean as 0 / 1, a Timestamp as its int64. A Utf8 value goes through the copy the kernel makes: rows
// without doubled quotes byte by byte, marked rows of up to 64 raw bytes by the serial walk of one lane, longer ones by the
// wavefront's 64-byte steps with a simulated ballot. The file and every buffer carry exactly the 64 bytes of slack a device
// allocation has, so the sanitizers see any access beyond it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device/qhip_csv.inc"

static const size_t kSlack = 64;

struct Spec { int kind; int width; int a; int b; };

static bool parse_type(const std::string& s, Spec& o) {
  o = Spec{QH_CSV_K_INT, 0, 0, 0};
  if (s == "f64") { o.kind = QH_CSV_K_FLOAT64; o.width = 8; return true; }
  if (s == "date") { o.kind = QH_CSV_K_DATE32; o.width = 4; return true; }
  if (s == "utf8") { o.kind = QH_CSV_K_UTF8; o.width = 4; return true; }
  if (s == "bool") { o.kind = QH_CSV_K_BOOL; o.width = 1; return true; }   // (the program keeps one byte per row; the kernel a ballot word)
  if (s.rfind("ts", 0) == 0 && s.size() == 3) { o.kind = QH_CSV_K_TIMESTAMP; o.width = 8; o.a = s[2] - '0'; return o.a == 0 || o.a == 3 || o.a == 6 || o.a == 9; }
  if (s.rfind("dec:", 0) == 0) { o.kind = QH_CSV_K_DECIMAL128; o.width = 16; return sscanf(s.c_str(), "dec:%d:%d", &o.a, &o.b) == 2; }
  if ((s[0] == 'i' || s[0] == 'u') && s.size() >= 2) {
    const int bits = atoi(s.c_str() + 1);
    if (bits != 8 && bits != 16 && bits != 32 && bits != 64) return false;
    o.width = bits / 8; o.a = s[0] == 'i';
    return true;
  }
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

static void print_i128(FILE* f, unsigned long long lo, unsigned long long hi) {
  unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
  const bool neg = (hi >> 63) != 0;
  if (neg) v = (unsigned __int128)0 - v;
  char buf[48];
  int n = 0;
  do { buf[n++] = (char)('0' + (int)(v % 10)); v /= 10; } while (v);
  if (neg) fputc('-', f);
  while (n) fputc(buf[--n], f);
}

// ---- the copy of one marked row, as k_csv_copy_utf8_q makes it
// one lane, a raw span of up to 64 bytes
static void lane_copy(const unsigned char* src, unsigned n, unsigned char* dst, int quote) {
  size_t q = 0;
  for (unsigned b = 0; b < n; ++b) {
    const unsigned char c = src[q];
    dst[b] = c;
    q += (int)c == quote ? 2 : 1;
  }
}
// the wavefront: 64 raw bytes per step, the ballots simulated lane by lane
static void wave_copy(const unsigned char* src, unsigned n, unsigned char* dst, int quote) {
  unsigned long long emitted = 0;
  unsigned carry = 0;
  for (size_t raw = 0; emitted < n; raw += 64) {
    unsigned long long quotes = 0, dropped = 0;
    for (int l = 0; l < 64; ++l) quotes |= (unsigned long long)((int)src[raw + (size_t)l] == quote) << l;
    for (int l = 0; l < 64; ++l) dropped |= (unsigned long long)qh_csv_undouble_drops(quotes, carry, l) << l;
    for (int l = 0; l < 64; ++l) {
      if ((dropped >> l) & 1ULL) continue;
      const unsigned long long o = qh_csv_undouble_out(emitted, dropped, l);
      if (o < n) dst[o] = src[raw + (size_t)l];
    }
    emitted += (unsigned long long)__builtin_popcountll(~dropped);
    carry = qh_csv_undouble_carry(quotes, carry);
  }
}

static int run_undouble() {
  const int quote = '"';
  size_t checked = 0;
  for (int run = 1; run <= 130; ++run) {
    for (int at = 0; at <= 129; ++at) {
      // 'a' x at, the run, then text with a pair of its own so that the parity behind the run matters
      std::string raw(at, 'a');
      raw.append((size_t)run, '"');
      raw += "bc\"\"d";
      raw.append(70, 'e');
      unsigned char* src = (unsigned char*)malloc(raw.size() + kSlack);
      memcpy(src, raw.data(), raw.size());
      memset(src + raw.size(), '"', kSlack);   // (what lies behind the field is arbitrary: quotes are the worst case)
      std::string want;                         // the byte-serial undouble
      for (size_t i = 0; i < raw.size(); ++i) { want.push_back(raw[i]); if (raw[i] == '"' && i + 1 < raw.size() && raw[i + 1] == '"') ++i; }
      // an odd run's last quote pairs with nothing inside `raw`; behind it comes 'b'
      unsigned char* dst = (unsigned char*)malloc(want.size() + kSlack);
      memset(dst, 0xCD, want.size() + kSlack);
      wave_copy(src, (unsigned)want.size(), dst, quote);
      bool ok = memcmp(dst, want.data(), want.size()) == 0;
      for (size_t i = 0; i < kSlack; ++i) ok = ok && dst[want.size() + i] == 0xCD;
      if (ok && raw.size() <= 64) {
        memset(dst, 0xCD, want.size());
        lane_copy(src, (unsigned)want.size(), dst, quote);
        ok = memcmp(dst, want.data(), want.size()) == 0;
      }
      free(src); free(dst);
      if (!ok) { printf("MISMATCH run %d at %d\n", run, at); return 1; }
      ++checked;
    }
  }
  printf("UNDOUBLE OK %zu\n", checked);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "undouble") == 0) return run_undouble();
  if (argc != 8 || strcmp(argv[1], "decode") != 0) { fprintf(stderr, "usage: csv_grammar2_tests decode file types has_header delimiter quote projection | undouble\n"); return 2; }
  ++argv;
  std::vector<Spec> fields;
  for (const std::string& s : split(argv[2], ',')) {
    Spec sp;
    if (!parse_type(s, sp)) { fprintf(stderr, "bad type %s\n", s.c_str()); return 2; }
    fields.push_back(sp);
  }
  const int has_header = atoi(argv[3]), delim = atoi(argv[4]), quote = atoi(argv[5]);
  std::vector<int> proj;
  if (strcmp(argv[6], "-") == 0) for (size_t k = 0; k < fields.size(); ++k) proj.push_back((int)k);
  else for (const std::string& s : split(argv[6], ',')) proj.push_back(atoi(s.c_str()));

  FILE* in = fopen(argv[1], "rb");
  if (!in) { perror(argv[1]); return 2; }
  fseek(in, 0, SEEK_END);
  const size_t n = (size_t)ftell(in);
  fseek(in, 0, SEEK_SET);
  unsigned char* buf = (unsigned char*)malloc(n + kSlack);
  if (n && fread(buf, 1, n, in) != n) { perror("read"); return 2; }
  fclose(in);
  memset(buf + n, 0xAB, kSlack);

  if (n == 0) { printf("NEEDS_HOST empty 0\n"); free(buf); return 0; }
  size_t d0 = 0;
  if (has_header) {
    const unsigned char* nl = (const unsigned char*)memchr(buf, '\n', n);
    d0 = nl ? (size_t)(nl - buf) + 1 : n;
  }
  // ---- the splitter at level 2: no byte is a quote for it (k_csv_scan is launched with quote = -1), every '\n' ends a record
  std::vector<unsigned long long> starts;
  starts.push_back(d0);
  for (size_t i = d0; i < n; ++i) {
    const unsigned cls = qh_csv_byte_class(buf[i], -1);
    unsigned reason = 0;
    if ((cls & QH_CSV_B_CR) && !(i + 1 < n && buf[i + 1] == '\n')) reason = QH_CSV_R_LONE_CR;
    else if (cls & QH_CSV_B_LF) {
      const size_t s = (size_t)starts.back();
      if (i == s || (i == s + 1 && buf[s] == '\r')) reason = QH_CSV_R_EMPTY_LINE;
      starts.push_back(i + 1);
    }
    if (reason) { printf("NEEDS_HOST %u %zu\n", reason, starts.size() - (reason == QH_CSV_R_EMPTY_LINE ? 1 : 0)); free(buf); return 0; }
  }
  if (n > d0 && buf[n - 1] != '\n') starts.push_back(n + 1);
  const size_t R = starts.size() - 1;

  std::vector<int> order(proj.size());
  for (size_t k = 0; k < proj.size(); ++k) order[k] = (int)k;
  for (size_t i = 1; i < order.size(); ++i)
    for (size_t j = i; j > 0 && proj[(size_t)order[j]] < proj[(size_t)order[j - 1]]; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
  std::vector<qh_csv_col> desc(order.size());
  std::vector<std::vector<unsigned char>> valid(order.size(), std::vector<unsigned char>(R, 0));
  for (size_t j = 0; j < order.size(); ++j) {
    const Spec& sp = fields[(size_t)proj[(size_t)order[j]]];
    qh_csv_col& d = desc[j];
    memset(&d, 0, sizeof d);
    d.values = malloc(R * (size_t)sp.width + kSlack);
    d.strpos = sp.kind == QH_CSV_K_UTF8 ? (unsigned long long*)malloc(R * 8 + kSlack) : nullptr;
    d.field = (unsigned)proj[(size_t)order[j]];
    d.kind = (unsigned char)sp.kind; d.width = (unsigned char)sp.width; d.a = (unsigned char)sp.a; d.b = (unsigned char)sp.b;
  }
  auto release = [&] { for (auto& d : desc) { free(d.values); free(d.strpos); } free(buf); };
  for (size_t r = 0; r < R; ++r) {
    const size_t s = (size_t)starts[r];
    size_t len = (size_t)starts[r + 1] - 1 - s;
    if (len > 0 && buf[s + len - 1] == '\r') --len;
    unsigned long long vm = 0, tm = 0;
    const int reason = qh_csv_decode_record_q(desc.data(), (int)desc.size(), (unsigned)fields.size(), (unsigned char)delim, quote, buf + s, len, r, s, &vm, &tm);
    if (reason != QH_CSV_OK) { printf("NEEDS_HOST %d %zu\n", reason, r + 1); release(); return 0; }
    for (size_t j = 0; j < desc.size(); ++j) {
      valid[j][r] = (unsigned char)((vm >> j) & 1);
      if (desc[j].kind == QH_CSV_K_BOOL) ((unsigned char*)desc[j].values)[r] = (unsigned char)((tm >> j) & 1);
    }
  }
  std::vector<size_t> at(proj.size());
  for (size_t j = 0; j < order.size(); ++j) at[(size_t)order[j]] = j;
  printf("ROWS %zu\n", R);
  for (size_t r = 0; r < R; ++r) {
    for (size_t k = 0; k < proj.size(); ++k) {
      const size_t j = at[k];
      const qh_csv_col& d = desc[j];
      if (k) fputc('\t', stdout);
      if (!valid[j][r]) { fputc('N', stdout); continue; }
      switch (d.kind) {
        case QH_CSV_K_INT:
          if (d.a) {
            long long v = d.width == 1 ? ((signed char*)d.values)[r] : d.width == 2 ? ((short*)d.values)[r] : d.width == 4 ? ((int*)d.values)[r] : ((long long*)d.values)[r];
            printf("%lld", v);
          } else {
            unsigned long long v = d.width == 1 ? ((unsigned char*)d.values)[r] : d.width == 2 ? ((unsigned short*)d.values)[r] : d.width == 4 ? ((unsigned*)d.values)[r] : ((unsigned long long*)d.values)[r];
            printf("%llu", v);
          }
          break;
        case QH_CSV_K_DATE32: printf("%d", ((int*)d.values)[r]); break;
        case QH_CSV_K_DECIMAL128: print_i128(stdout, ((unsigned long long*)d.values)[2 * r], ((unsigned long long*)d.values)[2 * r + 1]); break;
        case QH_CSV_K_FLOAT64: printf("%016llx", ((unsigned long long*)d.values)[r]); break;
        case QH_CSV_K_BOOL: printf("%d", (int)((unsigned char*)d.values)[r]); break;
        case QH_CSV_K_TIMESTAMP: printf("%lld", ((long long*)d.values)[r]); break;
        default: {
          fputc('s', stdout);
          const unsigned len = ((unsigned*)d.values)[r];
          const unsigned long long pos = d.strpos[r] & QH_CSV_POS_MASK;
          unsigned char* out = (unsigned char*)malloc(len + kSlack);
          if (!(d.strpos[r] & QH_CSV_POS_PAIRS)) { if (len) memcpy(out, buf + pos, len); }
          else if (!(d.strpos[r] & QH_CSV_POS_LONG)) lane_copy(buf + pos, len, out, quote);
          else wave_copy(buf + pos, len, out, quote);
          for (unsigned b = 0; b < len; ++b) printf("%02x", out[b]);
          free(out);
        }
      }
    }
    fputc('\n', stdout);
  }
  release();
  return 0;
}
