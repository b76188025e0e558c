// widekey_tests.cpp — the per-row code of the wide-key encoding stage (csrc/device/qhip_widekey.inc) compiled for the host: the
// insert loop runs single-threaded over small ragged tables whose buffers carry the 64 bytes of slack every device allocation
// has, and the group codes are checked against a std::map of the keys. Stand-alone: no HIP, no library of the project.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "device/qhip_widekey.inc"

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    ++g_checks;                                                                \
    if (!(cond)) { ++g_failed; printf("FAILED %s:%d: %s — ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
  } while (0)

struct PlainSlot {   // the host's slot accesses: one thread
  static unsigned long long load(const unsigned long long* p) { return *p; }
  static unsigned long long cas(unsigned long long* p, unsigned long long desired) {
    const unsigned long long old = *p;
    if (old == 0) *p = desired;
    return old;
  }
};

constexpr size_t kSlack = 64;   // DevBuf::alloc: every allocation is 64 bytes longer than asked for
struct Buf {                     // (heap blocks of the exact size: the address sanitizer sees a read past the slack)
  std::vector<uint8_t> b;
  explicit Buf(size_t n = 0) : b(n + kSlack, 0xA5) {}   // (the slack holds garbage: no result may depend on it)
  uint8_t* p() { return b.data(); }
};

// a column as the test describes it: per row NULL or the value's bytes
struct Column {
  unsigned width;   // 0 = Utf8
  bool nullable;
  std::vector<bool> valid;
  std::vector<std::string> bytes;   // value bytes (fixed width: exactly `width` of them, NULL rows: garbage)
  Buf values, data, validity;
  qh_wk_col desc;
  void finish() {
    const size_t n = bytes.size();
    if (width == 0) {
      size_t total = 0;
      for (auto& s : bytes) total += s.size();
      values = Buf((n + 1) * 4);
      data = Buf(total);
      int32_t off = 0;
      for (size_t r = 0; r < n; ++r) {
        memcpy(values.p() + 4 * r, &off, 4);
        if (!bytes[r].empty()) memcpy(data.p() + off, bytes[r].data(), bytes[r].size());
        off += (int32_t)bytes[r].size();
      }
      memcpy(values.p() + 4 * n, &off, 4);
    } else {
      values = Buf(n * width);
      for (size_t r = 0; r < n; ++r) memcpy(values.p() + r * width, bytes[r].data(), width);
    }
    validity = Buf((n + 7) / 8);
    memset(validity.p(), 0, (n + 7) / 8);
    for (size_t r = 0; r < n; ++r) if (valid[r]) validity.p()[r >> 3] |= (uint8_t)(1u << (r & 7));
    desc.v = values.p();
    desc.d = width == 0 ? data.p() : nullptr;
    desc.n = nullable ? validity.p() : nullptr;
    desc.width = width;
    desc.pad = 0;
  }
};

static std::string key_of(const std::vector<Column>& cols, size_t r) {
  std::string k;
  for (auto& c : cols) {
    if (c.nullable && !c.valid[r]) { k += "N"; continue; }
    const uint32_t len = (uint32_t)c.bytes[r].size();
    k += "V";
    k.append((const char*)&len, 4);
    k += c.bytes[r];
  }
  return k;
}

static void run_table(const char* what, std::vector<Column>& cols, size_t n, int hash_bits) {
  std::vector<qh_wk_col> desc;
  for (auto& c : cols) { c.finish(); desc.push_back(c.desc); }
  unsigned nslots = 1024;
  while (nslots < 2 * n) nslots *= 2;
  std::vector<unsigned long long> table(nslots, 0);
  const unsigned long long mask = hash_bits ? (1ULL << hash_bits) - 1 : ~0ULL;
  std::vector<unsigned> code(n);
  for (size_t r = 0; r < n; ++r) code[r] = qh_wk_insert<PlainSlot>(desc.data(), (int)desc.size(), table.data(), nslots - 1, mask, (unsigned)r);
  std::map<std::string, unsigned> want;   // key -> the code its first row got
  std::set<unsigned> distinct;
  for (size_t r = 0; r < n; ++r) {
    CHECK(code[r] < n, "%s: row %zu has code %u of %zu rows", what, r, code[r], n);
    if (code[r] >= n) return;
    const std::string k = key_of(cols, r);
    CHECK(key_of(cols, code[r]) == k, "%s: row %zu is represented by row %u of another key", what, r, code[r]);
    CHECK(code[code[r]] == code[r], "%s: the representative %u of row %zu is not its own", what, code[r], r);
    auto it = want.find(k);
    if (it == want.end()) want.emplace(k, code[r]);
    else CHECK(it->second == code[r], "%s: row %zu has code %u, an earlier row of its key %u", what, r, code[r], it->second);
    distinct.insert(code[r]);
  }
  CHECK(distinct.size() == want.size(), "%s: %zu codes for %zu keys", what, distinct.size(), want.size());
  size_t used = 0;
  for (auto s : table) used += s != 0;
  CHECK(used == want.size(), "%s: %zu slots set for %zu keys", what, used, want.size());
}

template <class T> static std::string raw(T v) { return std::string((const char*)&v, sizeof v); }

// the Q10 shape in small: Int64, short Utf8, Decimal128, Utf8 up to 117 bytes, Int32, UInt8 — every column nullable or not by turns
static void mixed_table(size_t n, unsigned groups, int hash_bits, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::vector<Column> cols(6);
  const unsigned widths[6] = {8, 0, 16, 0, 4, 1};
  for (int c = 0; c < 6; ++c) { cols[c].width = widths[c]; cols[c].nullable = (c + seed) % 2 == 0; }
  for (size_t r = 0; r < n; ++r) {
    const uint64_t g = groups ? rng() % groups : r;   // (groups == 0: every row its own key)
    std::mt19937_64 kr(g * 7919 + 1);
    for (int c = 0; c < 6; ++c) {
      Column& col = cols[c];
      const bool valid = !col.nullable || kr() % 5 != 0;
      col.valid.push_back(valid);
      std::string v;
      if (col.width == 0) {
        const size_t len = c == 1 ? kr() % 19 : kr() % 118;
        for (size_t b = 0; b < len; ++b) v.push_back((char)('a' + kr() % 3));
        if (!groups) v += std::to_string(r);
      } else if (col.width == 16) {
        v = raw<uint64_t>(kr() % 4) + raw<int64_t>((int64_t)(kr() % 3) - 1);
      } else if (col.width == 8) {
        v = raw<int64_t>((int64_t)(kr() % 1000) - 500);
      } else if (col.width == 4) {
        v = raw<int32_t>((int32_t)(kr() % 7) - 3);
      } else {
        v = raw<uint8_t>((uint8_t)(kr() % 3));
      }
      if (!valid) {   // a NULL's value bytes are whatever the buffer holds: they must not matter
        if (col.width == 0) v = rng() % 2 ? std::string(rng() % 9, 'z') : std::string();
        else for (auto& ch : v) ch = (char)rng();
      }
      col.bytes.push_back(v);
    }
  }
  char what[96];
  snprintf(what, sizeof what, "mixed n=%zu groups=%u bits=%d seed=%u", n, groups, hash_bits, seed);
  run_table(what, cols, n, hash_bits);
}

// one Utf8 key of 56..300 bytes whose values differ only in the last byte, at every 8-byte boundary, and in length only
static void late_differences() {
  std::string base;
  for (int k = 0; k < 300; ++k) base.push_back((char)('A' + k % 23));
  std::vector<std::string> vals{"", base};
  for (size_t len : {56u, 57u, 63u, 64u, 65u, 71u, 72u, 73u, 117u, 128u, 255u, 256u, 299u}) {
    vals.push_back(base.substr(0, len));                                                  // differs in length only
    { std::string s = base.substr(0, len); s.back() ^= 1; vals.push_back(s); }            // ... in the last byte
    for (size_t at = 8; at < len; at += 8) {                                              // ... around every word boundary
      std::string s = base.substr(0, len); s[at] ^= 2; vals.push_back(s);
      std::string t = base.substr(0, len); t[at - 1] ^= 4; vals.push_back(t);
    }
  }
  std::vector<Column> cols(1);
  cols[0].width = 0; cols[0].nullable = true;
  std::mt19937_64 rng(5);
  const size_t n = vals.size() * 3 + 7;
  for (size_t r = 0; r < n; ++r) {
    const bool valid = rng() % 11 != 0;
    cols[0].valid.push_back(valid);
    cols[0].bytes.push_back(valid ? vals[rng() % vals.size()] : (rng() % 2 ? std::string("junk") : std::string()));
  }
  run_table("late differences", cols, n, 0);
  run_table("late differences, 3 hash bits", cols, n, 3);
}

// (NULL, 5) and (5, NULL) stay two groups; NULL equals NULL within a column
static void null_positions() {
  std::vector<Column> cols(2);
  const int64_t a[] = {0, 5, 5, 0, 5, 0, 7};
  const int64_t b[] = {5, 0, 5, 5, 0, 0, 0};
  const bool va[] = {false, true, true, false, true, false, false};
  const bool vb[] = {true, false, true, true, false, false, false};
  for (int c = 0; c < 2; ++c) { cols[c].width = 8; cols[c].nullable = true; }
  for (int r = 0; r < 7; ++r) {
    cols[0].valid.push_back(va[r]); cols[0].bytes.push_back(raw<int64_t>(a[r]));
    cols[1].valid.push_back(vb[r]); cols[1].bytes.push_back(raw<int64_t>(b[r]));
  }
  std::vector<qh_wk_col> desc;
  for (auto& c : cols) { c.finish(); desc.push_back(c.desc); }
  std::vector<unsigned long long> table(1024, 0);
  unsigned code[7];
  for (unsigned r = 0; r < 7; ++r) code[r] = qh_wk_insert<PlainSlot>(desc.data(), 2, table.data(), 1023, ~0ULL, r);
  const unsigned want[7] = {0, 1, 2, 0, 1, 5, 5};
  for (int r = 0; r < 7; ++r) CHECK(code[r] == want[r], "null positions: row %d has code %u, expected %u", r, code[r], want[r]);
}

int main() {
  for (size_t n : {0u, 1u, 63u, 64u, 65u, 257u, 1000u}) {
    mixed_table(n, 1, 0, 1);     // one group for all rows
    mixed_table(n, 0, 0, 2);     // every row its own group
    mixed_table(n, 40, 0, 3);
    mixed_table(n, 40, 3, 4);    // 8 hash values: long probe chains, equal tags on different keys
  }
  mixed_table(5000, 300, 3, 5);
  mixed_table(5000, 300, 0, 6);
  late_differences();
  null_positions();
  printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
