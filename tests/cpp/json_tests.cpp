// json_tests.cpp — the device JSON decoder on the host (qurious_amd/csrc/device/qhip_json.inc as plain C++): the record walk and
// the unescaping copy's lane logic, the very functions kernels_json.hip calls. tests/test_json_cpu.py compares the dump with
// pyarrow.json.read_json(explicit_schema=...) on the same bytes.
//
//   json_tests decode <file> <names> <types> <projection | ->  > dump
//     names: the schema's keys, comma separated; types: i8 .. u64 f64 date utf8 bool dec:P:S ts0 ts3 ts6 ts9
//   json_tests unescape      runs of 1..130 backslashes at every offset 0..129: the wavefront's copy against a byte-serial one
//
// Dump: "ROWS n" and one line per row, cells separated by tabs (N = NULL, a Float64 as its bits, a Utf8 value as hex behind an
// 's'), or "NEEDS_HOST <reason> <1-based record>". A Utf8 value goes through the copy the kernel makes: rows without escapes byte
// by byte, marked rows of up to 64 raw bytes by the serial walk of one lane, longer ones by the wavefront's 64-byte steps with a
// simulated ballot. The file and every buffer carry exactly the 64 bytes of slack a device allocation has, so the sanitizers
// see any access beyond it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device/qhip_json.inc"

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
    o.width = bits / 8; o.a = s[0] == 'i'; o.b = o.width;
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

// ---- the copy of one marked row, as k_json_copy_utf8 makes it
// one lane, a raw span of up to 64 bytes
static void lane_copy(const unsigned char* src, unsigned n, unsigned char* dst) {
  size_t q = 0;
  for (unsigned b = 0; b < n; ++b) {
    unsigned char c = src[q++];
    if (c == '\\') c = qh_json_unescape_byte(src[q++]);
    dst[b] = c;
  }
}
// the wavefront: 64 raw bytes per step, the ballots simulated lane by lane
static void wave_copy(const unsigned char* src, unsigned n, unsigned char* dst) {
  unsigned long long emitted = 0;
  unsigned carry = 0;
  for (size_t raw = 0; emitted < n; raw += 64) {
    unsigned long long slashes = 0, dropped = 0;
    for (int l = 0; l < 64; ++l) slashes |= (unsigned long long)(src[raw + (size_t)l] == '\\') << l;
    for (int l = 0; l < 64; ++l) dropped |= (unsigned long long)qh_json_unescape_drops(slashes, carry, l) << l;
    for (int l = 0; l < 64; ++l) {
      if ((dropped >> l) & 1ULL) continue;
      const unsigned long long o = qh_csv_undouble_out(emitted, dropped, l);
      const unsigned char c = src[raw + (size_t)l];
      if (o < n) dst[o] = qh_json_unescape_escaped(dropped, carry, l) ? qh_json_unescape_byte(c) : c;
    }
    emitted += (unsigned long long)__builtin_popcountll(~dropped);
    carry = qh_csv_undouble_carry(slashes, carry);
  }
}

static int run_unescape() {
  size_t checked = 0;
  for (int run = 1; run <= 130; ++run) {
    for (int at = 0; at <= 129; ++at) {
      // 'a' x at, the run, an 'n' (a line feed behind a run of odd length, itself behind an even one), then text with escapes
      // of its own so that the parity behind the run matters
      std::string raw(at, 'a');
      raw.append((size_t)run, '\\');
      raw += "nbc\\\"d\\\\\\te\\/";
      raw.append(70, 'f');
      raw += "\\r";
      unsigned char* src = (unsigned char*)malloc(raw.size() + kSlack);
      memcpy(src, raw.data(), raw.size());
      memset(src + raw.size(), '\\', kSlack);   // (what lies behind the value is arbitrary: backslashes are the worst case)
      std::string want;                          // the byte-serial unescape
      for (size_t i = 0; i < raw.size(); ++i) {
        if (raw[i] == '\\') want.push_back((char)qh_json_unescape_byte((unsigned char)raw[++i]));
        else want.push_back(raw[i]);
      }
      unsigned char* dst = (unsigned char*)malloc(want.size() + kSlack);
      memset(dst, 0xCD, want.size() + kSlack);
      wave_copy(src, (unsigned)want.size(), dst);
      bool ok = memcmp(dst, want.data(), want.size()) == 0;
      for (size_t i = 0; i < kSlack; ++i) ok = ok && dst[want.size() + i] == 0xCD;
      if (ok && raw.size() <= 64) {
        memset(dst, 0xCD, want.size());
        lane_copy(src, (unsigned)want.size(), dst);
        ok = memcmp(dst, want.data(), want.size()) == 0;
      }
      free(src); free(dst);
      if (!ok) { printf("MISMATCH run %d at %d\n", run, at); return 1; }
      ++checked;
    }
  }
  printf("UNESCAPE OK %zu\n", checked);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "unescape") == 0) return run_unescape();
  if (argc != 6 || strcmp(argv[1], "decode") != 0) { fprintf(stderr, "usage: json_tests decode file names types projection | unescape\n"); return 2; }
  const std::vector<std::string> names = split(argv[3], ',');
  std::vector<Spec> fields;
  for (const std::string& s : split(argv[4], ',')) {
    Spec sp;
    if (!parse_type(s, sp)) { fprintf(stderr, "bad type %s\n", s.c_str()); return 2; }
    fields.push_back(sp);
  }
  if (names.size() != fields.size() || fields.size() > QH_JSON_MAX_FIELDS) { fprintf(stderr, "names and types differ\n"); return 2; }
  std::vector<int> proj;
  if (strcmp(argv[5], "-") == 0) for (size_t k = 0; k < fields.size(); ++k) proj.push_back((int)k);
  else for (const std::string& s : split(argv[5], ',')) proj.push_back(atoi(s.c_str()));

  FILE* in = fopen(argv[2], "rb");
  if (!in) { perror(argv[2]); return 2; }
  fseek(in, 0, SEEK_END);
  const size_t n = (size_t)ftell(in);
  fseek(in, 0, SEEK_SET);
  unsigned char* buf = (unsigned char*)malloc(n + kSlack);
  if (n && fread(buf, 1, n, in) != n) { perror("read"); return 2; }
  fclose(in);
  memset(buf + n, 0xAB, kSlack);

  if (n == 0) { printf("NEEDS_HOST empty 0\n"); free(buf); return 0; }
  if (n >= 3 && buf[0] == 0xEF && buf[1] == 0xBB && buf[2] == 0xBF) { printf("NEEDS_HOST bom 0\n"); free(buf); return 0; }
  // ---- the splitter (k_csv_scan with quote = -1): every '\n' ends a record
  std::vector<unsigned long long> starts;
  starts.push_back(0);
  for (size_t i = 0; i < n; ++i) {
    const unsigned cls = qh_csv_byte_class(buf[i], -1);
    unsigned reason = 0;
    if ((cls & QH_CSV_B_CR) && !(i + 1 < n && buf[i + 1] == '\n')) reason = QH_JSON_R_LONE_CR;
    else if (cls & QH_CSV_B_LF) {
      const size_t s = (size_t)starts.back();
      if (i == s || (i == s + 1 && buf[s] == '\r')) reason = QH_JSON_R_EMPTY_LINE;
      starts.push_back(i + 1);
    }
    if (reason) { printf("NEEDS_HOST %u %zu\n", reason, starts.size() - (reason == QH_JSON_R_EMPTY_LINE ? 1 : 0)); free(buf); return 0; }
  }
  if (buf[n - 1] != '\n') starts.push_back(n + 1);
  const size_t R = starts.size() - 1;

  // (the descriptor is as large as a kernel argument: on the heap, with the slack behind it)
  qh_json_desc* desc = (qh_json_desc*)calloc(1, sizeof(qh_json_desc) + kSlack);
  size_t name_bytes = 0;
  for (size_t f = 0; f < fields.size(); ++f) {
    if (name_bytes + names[f].size() > QH_JSON_MAX_NAME_BYTES) { fprintf(stderr, "names too long\n"); return 2; }
    qh_json_field& d = desc->field[f];
    d.name_off = (unsigned short)name_bytes; d.name_len = (unsigned short)names[f].size();
    memcpy(desc->names + name_bytes, names[f].data(), names[f].size());
    name_bytes += names[f].size();
    d.kind = (unsigned char)fields[f].kind; d.col = -1; d.a = (unsigned char)fields[f].a; d.b = (unsigned char)fields[f].b;
  }
  std::vector<std::vector<unsigned char>> valid(proj.size(), std::vector<unsigned char>(R, 0));
  for (size_t k = 0; k < proj.size(); ++k) {
    const Spec& sp = fields[(size_t)proj[k]];
    desc->field[proj[k]].col = (signed char)k;
    desc->out[k].values = malloc(R * (size_t)sp.width + kSlack);
    desc->out[k].strpos = sp.kind == QH_CSV_K_UTF8 ? (unsigned long long*)malloc(R * 8 + kSlack) : nullptr;
  }
  auto release = [&] { for (size_t k = 0; k < proj.size(); ++k) { free(desc->out[k].values); free(desc->out[k].strpos); } free(desc); free(buf); };
  for (size_t r = 0; r < R; ++r) {
    const size_t s = (size_t)starts[r];
    size_t len = (size_t)starts[r + 1] - 1 - s;
    if (len > 0 && buf[s + len - 1] == '\r') --len;
    unsigned long long vm = 0, tm = 0;
    const int reason = qh_json_decode_record(*desc, (unsigned)fields.size(), buf + s, len, r, s, &vm, &tm);
    if (reason != QH_CSV_OK) { printf("NEEDS_HOST %d %zu\n", reason, r + 1); release(); return 0; }
    for (size_t k = 0; k < proj.size(); ++k) {
      valid[k][r] = (unsigned char)((vm >> k) & 1);
      if (fields[(size_t)proj[k]].kind == QH_CSV_K_BOOL) ((unsigned char*)desc->out[k].values)[r] = (unsigned char)((tm >> k) & 1);
    }
  }
  printf("ROWS %zu\n", R);
  for (size_t r = 0; r < R; ++r) {
    for (size_t k = 0; k < proj.size(); ++k) {
      const Spec& sp = fields[(size_t)proj[k]];
      const qh_json_out& d = desc->out[k];
      if (k) fputc('\t', stdout);
      if (!valid[k][r]) { fputc('N', stdout); continue; }
      switch (sp.kind) {
        case QH_CSV_K_INT:
          if (sp.a) {
            long long v = sp.width == 1 ? ((signed char*)d.values)[r] : sp.width == 2 ? ((short*)d.values)[r] : sp.width == 4 ? ((int*)d.values)[r] : ((long long*)d.values)[r];
            printf("%lld", v);
          } else {
            unsigned long long v = sp.width == 1 ? ((unsigned char*)d.values)[r] : sp.width == 2 ? ((unsigned short*)d.values)[r] : sp.width == 4 ? ((unsigned*)d.values)[r] : ((unsigned long long*)d.values)[r];
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
          const unsigned long long pos = d.strpos[r] & QH_JSON_POS_MASK;
          unsigned char* out = (unsigned char*)malloc(len + kSlack);
          if (!(d.strpos[r] & QH_JSON_POS_ESC)) { if (len) memcpy(out, buf + pos, len); }
          else if (!(d.strpos[r] & QH_JSON_POS_LONG)) lane_copy(buf + pos, len, out);
          else wave_copy(buf + pos, len, out);
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
