// csv_tests.cpp — the device CSV decoder's per-field code on the host (qurious_amd/csrc/device/qhip_csv.inc as plain C++): the
// very functions kernels_csv.hip calls, driven by a byte-wise mirror of the record splitter. Decodes a file into a text dump
// that tests/test_csv_cpu.py compares with pyarrow on the same bytes; a file outside the grammar prints one NEEDS_HOST line.
//
//   csv_tests <file> <types> <has_header 0|1> <delimiter byte> <quote byte | -1> <projection | ->  > dump
//   types: comma-separated i8 i16 i32 i64 u8 u16 u32 u64 f64 date utf8 dec:P:S, one per field of a record
//
// Dump: one line per row, columns separated by '\t': integers / dates (days) / decimals (unscaled) in decimal, Float64 as the
// 16 hex digits of its bits, Utf8 as 's' + hex of its bytes, NULL as 'N'. The file and every output buffer are allocated with
// exactly the 64 bytes of slack a device allocation has, so the sanitizers see any read or write beyond it.
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

int main(int argc, char** argv) {
  if (argc != 7) { fprintf(stderr, "usage: csv_tests file types has_header delimiter quote projection\n"); return 2; }
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
  if (n >= 3 && buf[0] == 0xEF && buf[1] == 0xBB && buf[2] == 0xBF) { printf("NEEDS_HOST bom 0\n"); free(buf); return 0; }
  size_t d0 = 0;
  if (has_header) {
    const unsigned char* nl = (const unsigned char*)memchr(buf, '\n', n);
    d0 = nl ? (size_t)(nl - buf) + 1 : n;
  }
  // ---- the splitter, byte by byte (the kernels do the same over 16-byte vectors): record starts + structural reasons
  std::vector<unsigned long long> starts;
  starts.push_back(d0);
  for (size_t i = d0; i < n; ++i) {
    const unsigned cls = qh_csv_byte_class(buf[i], quote);
    unsigned reason = 0;
    if (cls & QH_CSV_B_QUOTE) reason = QH_CSV_R_QUOTE;
    else if ((cls & QH_CSV_B_CR) && !(i + 1 < n && (qh_csv_byte_class(buf[i + 1], quote) & QH_CSV_B_LF))) reason = QH_CSV_R_LONE_CR;
    else if (cls & QH_CSV_B_LF) {
      const size_t s = (size_t)starts.back();
      if (i == s || (i == s + 1 && buf[s] == '\r')) reason = QH_CSV_R_EMPTY_LINE;
      starts.push_back(i + 1);
    }
    if (reason) { printf("NEEDS_HOST %u %zu\n", reason, starts.size() - (reason == QH_CSV_R_EMPTY_LINE ? 1 : 0)); free(buf); return 0; }
  }
  if (n > d0 && buf[n - 1] != '\n') starts.push_back(n + 1);
  const size_t R = starts.size() - 1;

  // ---- descriptors (ascending by field) and output buffers, each with exactly the slack
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
  for (size_t r = 0; r < R; ++r) {
    const size_t s = (size_t)starts[r];
    size_t len = (size_t)starts[r + 1] - 1 - s;
    if (len > 0 && buf[s + len - 1] == '\r') --len;
    unsigned long long vm = 0;
    const int reason = qh_csv_decode_record(desc.data(), (int)desc.size(), (unsigned)fields.size(), (unsigned char)delim, buf + s, len, r, s, &vm);
    if (reason != QH_CSV_OK) {
      printf("NEEDS_HOST %d %zu\n", reason, r + 1);
      for (auto& d : desc) { free(d.values); free(d.strpos); }
      free(buf);
      return 0;
    }
    for (size_t j = 0; j < desc.size(); ++j) valid[j][r] = (unsigned char)((vm >> j) & 1);
  }
  // ---- dump in projection order
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
        default: {
          fputc('s', stdout);
          const unsigned len = ((unsigned*)d.values)[r];
          for (unsigned b = 0; b < len; ++b) printf("%02x", buf[d.strpos[r] + b]);
        }
      }
    }
    fputc('\n', stdout);
  }
  for (auto& d : desc) { free(d.values); free(d.strpos); }
  free(buf);
  return 0;
}
