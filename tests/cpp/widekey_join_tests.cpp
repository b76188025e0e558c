// widekey_join_tests.cpp — the per-row code of the wide JOIN key stage (csrc/device/qhip_widekey.inc: qh_wk_any_null,
// qh_wk_equal2, the build row and the lookup row) compiled for the host: the build loop, then the lookup loop, run
// single-threaded with plain slot accesses over small ragged tables whose buffers carry exactly the 64 bytes of slack every
// device allocation has. Build codes and probe codes are checked against a std::map of the keys without NULLs.
// Stand-alone: no HIP, no library of the project.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
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
  unsigned width = 8;   // 0 = Utf8
  bool nullable = false;
  std::vector<bool> valid;
  std::vector<std::string> bytes;   // value bytes (fixed width: exactly `width` of them, NULL rows: garbage)
  Buf values, data, validity;
  qh_wk_col desc;
  void add(bool is_valid, const std::string& v) { valid.push_back(is_valid); bytes.push_back(v); }
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
typedef std::vector<Column> Side;

static bool has_null(const Side& cols, size_t r) {
  for (auto& c : cols) if (c.nullable && !c.valid[r]) return true;
  return false;
}
static std::string key_of(const Side& cols, size_t r) {   // (of a row without NULLs)
  std::string k;
  for (auto& c : cols) {
    const uint32_t len = (uint32_t)c.bytes[r].size();
    k.append((const char*)&len, 4);
    k += c.bytes[r];
  }
  return k;
}

// build loop, then lookup loop; returns the probe codes (for the cases that know what they expect)
static std::vector<int> run_join(const char* what, Side& build, size_t B, Side& probe, size_t P, int hash_bits) {
  std::vector<qh_wk_col> bd, pd;
  for (auto& c : build) { c.finish(); bd.push_back(c.desc); }
  for (auto& c : probe) { c.finish(); pd.push_back(c.desc); }
  const int ncols = (int)bd.size();
  unsigned nslots = 1024;
  while (nslots < 2 * B) nslots *= 2;
  std::vector<unsigned long long> table(nslots, 0);
  const unsigned long long mask = hash_bits ? (1ULL << hash_bits) - 1 : ~0ULL;
  std::vector<unsigned> bcode(B);
  for (size_t r = 0; r < B; ++r) {
    CHECK(qh_wk_any_null(bd.data(), ncols, (unsigned)r) == has_null(build, r), "%s: build row %zu: any_null", what, r);
    bcode[r] = qh_wk_join_build_row<PlainSlot>(bd.data(), ncols, table.data(), nslots - 1, mask, (unsigned)r);
  }
  std::map<std::string, unsigned> want;   // key without NULLs -> the code its first build row got
  for (size_t r = 0; r < B; ++r) {
    CHECK(bcode[r] < B, "%s: build row %zu has code %u of %zu rows", what, r, bcode[r], B);
    if (bcode[r] >= B) return {};
    if (has_null(build, r)) {
      CHECK(bcode[r] == r, "%s: build row %zu with a NULL key column has code %u, not its own number", what, r, bcode[r]);
      continue;
    }
    const std::string k = key_of(build, r);
    CHECK(!has_null(build, bcode[r]), "%s: build row %zu is represented by row %u, which has a NULL key column", what, r, bcode[r]);
    CHECK(key_of(build, bcode[r]) == k, "%s: build row %zu is represented by row %u of another key", what, r, bcode[r]);
    CHECK(bcode[bcode[r]] == bcode[r], "%s: the representative %u of build row %zu is not its own", what, bcode[r], r);
    auto it = want.find(k);
    if (it == want.end()) want.emplace(k, bcode[r]);
    else CHECK(it->second == bcode[r], "%s: build row %zu has code %u, an earlier row of its key %u", what, r, bcode[r], it->second);
  }
  size_t used = 0;
  for (auto s : table) used += s != 0;
  CHECK(used == want.size(), "%s: %zu slots set for %zu keys without NULLs", what, used, want.size());
  const std::vector<unsigned long long> before = table;
  std::vector<int> pcode(P);
  for (size_t r = 0; r < P; ++r) {
    pcode[r] = qh_wk_join_lookup_row<PlainSlot>(pd.data(), bd.data(), ncols, table.data(), nslots - 1, mask, (unsigned)r);
    int expect = -1;
    if (!has_null(probe, r)) {
      auto it = want.find(key_of(probe, r));
      if (it != want.end()) expect = (int)it->second;
    }
    CHECK(pcode[r] == expect, "%s: probe row %zu has code %d, expected %d", what, r, pcode[r], expect);
  }
  CHECK(table == before, "%s: the lookups changed the table", what);
  return pcode;
}

template <class T> static std::string raw(T v) { return std::string((const char*)&v, sizeof v); }

// every fixed width (1 / 2 / 4 / 8 / 16) and two Utf8 columns (short, up to 117 bytes), nullable or not by turns; the probe
// side draws from more keys than the build side has, so some of its keys are absent
static void fill_mixed(Side& cols, size_t n, unsigned keys, unsigned seed, unsigned null_shift, bool own_keys) {
  std::mt19937_64 rng(seed);
  const unsigned widths[7] = {8, 0, 16, 0, 4, 1, 2};
  cols.assign(7, Column());
  for (int c = 0; c < 7; ++c) { cols[c].width = widths[c]; cols[c].nullable = (c + null_shift) % 2 == 0; }
  for (size_t r = 0; r < n; ++r) {
    const uint64_t g = own_keys ? r : rng() % keys;
    std::mt19937_64 kr(g * 7919 + 1);
    for (int c = 0; c < 7; ++c) {
      Column& col = cols[c];
      std::string v;
      if (col.width == 0) {
        const size_t len = c == 1 ? kr() % 19 : kr() % 118;
        for (size_t b = 0; b < len; ++b) v.push_back((char)('a' + kr() % 3));
        if (own_keys) v += std::to_string(r);
      } else if (col.width == 16) {
        v = raw<uint64_t>(kr() % 4) + raw<int64_t>((int64_t)(kr() % 3) - 1);
      } else if (col.width == 8) {
        v = raw<int64_t>((int64_t)(kr() % 1000) - 500);
      } else if (col.width == 4) {
        v = raw<int32_t>((int32_t)(kr() % 7) - 3);
      } else if (col.width == 2) {
        v = raw<uint16_t>((uint16_t)(kr() % 5));
      } else {
        v = raw<uint8_t>((uint8_t)(kr() % 3));
      }
      // NULLs are the row's own, not the key's: the same key shows with and without them on either side
      const bool valid = !col.nullable || rng() % 9 != 0;
      if (!valid) {   // a NULL's value bytes are whatever the buffer holds: they must not matter
        if (col.width == 0) v = rng() % 2 ? std::string(rng() % 9, 'z') : std::string();
        else for (auto& ch : v) ch = (char)rng();
      }
      col.add(valid, v);
    }
  }
}
static void mixed_join(size_t B, size_t P, unsigned keys, int hash_bits, unsigned seed, bool own_keys = false) {
  Side build, probe;
  fill_mixed(build, B, keys, seed, 0, own_keys);          // NULLs in columns 0, 2, 4, 6 of the build side
  fill_mixed(probe, P, keys + keys / 2 + 1, seed + 100, 1, own_keys);   // ... in columns 1, 3, 5 of the probe side
  char what[112];
  snprintf(what, sizeof what, "mixed B=%zu P=%zu keys=%u bits=%d seed=%u own=%d", B, P, keys, hash_bits, seed, (int)own_keys);
  run_join(what, build, B, probe, P, hash_bits);
}

// one Utf8 key of up to 300 bytes: empty strings, values that differ only in the last byte, around every 8-byte boundary and in
// length only; the probe side also holds strict prefixes of build values and values one byte longer, which the build side lacks
static void late_differences() {
  std::string base;
  for (int k = 0; k < 300; ++k) base.push_back((char)('A' + k % 23));
  std::vector<std::string> vals{"", base}, absent;
  for (size_t len : {1u, 7u, 8u, 9u, 15u, 16u, 17u, 56u, 57u, 63u, 64u, 65u, 71u, 72u, 73u, 117u, 128u, 255u, 256u, 299u}) {
    vals.push_back(base.substr(0, len));                                                  // differs in length only
    { std::string s = base.substr(0, len); s.back() ^= 1; vals.push_back(s); }            // ... in the last byte
    for (size_t at = 8; at < len; at += 8) {                                              // ... around every word boundary
      std::string s = base.substr(0, len); s[at] ^= 2; vals.push_back(s);
      std::string t = base.substr(0, len); t[at - 1] ^= 4; vals.push_back(t);
    }
    { std::string s = base.substr(0, len); s.back() ^= 8; absent.push_back(s); }          // absent: another last byte
    { std::string s = base.substr(0, len); s.back() ^= 1; absent.push_back(s.substr(0, len - 1) + "~"); }
    absent.push_back(base.substr(0, len) + "!");                                          // absent: a build value is its strict prefix
  }
  absent.push_back(base.substr(0, 2));     // absent: strict prefixes of build values
  absent.push_back(base.substr(0, 60));
  absent.push_back(base.substr(0, 298));
  Side build(1), probe(1);
  build[0].width = probe[0].width = 0;
  build[0].nullable = probe[0].nullable = true;
  std::mt19937_64 rng(5);
  const size_t B = vals.size() * 2 + 7, P = (vals.size() + absent.size()) * 3 + 5;
  for (size_t r = 0; r < B; ++r) {
    const bool valid = rng() % 11 != 0;
    build[0].add(valid, valid ? vals[rng() % vals.size()] : (rng() % 2 ? std::string("junk") : std::string()));
  }
  for (size_t r = 0; r < P; ++r) {
    const bool valid = rng() % 11 != 0;
    const size_t pick = rng() % (vals.size() + absent.size());
    probe[0].add(valid, valid ? (pick < vals.size() ? vals[pick] : absent[pick - vals.size()]) : std::string("junk"));
  }
  run_join("late differences", build, B, probe, P, 0);
  run_join("late differences, 3 hash bits", build, B, probe, P, 3);
}

// a probe value that is a strict prefix of the one build value, and the other way round, at the exact end of the data buffer
static void prefixes() {
  for (size_t len : {1u, 8u, 9u, 16u, 60u, 64u, 117u}) {
    std::string v;
    for (size_t k = 0; k < len; ++k) v.push_back((char)('a' + k % 7));
    Side build(1), probe(1);
    build[0].width = probe[0].width = 0;
    build[0].add(true, v);
    probe[0].add(true, v.substr(0, len - 1));
    probe[0].add(true, v + "x");
    probe[0].add(true, v);   // (the last value of its buffer: the masked tail reads into the slack)
    const std::vector<int> got = run_join("prefixes", build, 1, probe, 3, 0);
    CHECK(got.size() == 3 && got[0] == -1 && got[1] == -1 && got[2] == 0, "prefixes of %zu bytes", len);
  }
}

// in a join NULL equals nothing: (NULL, 5) vs (5, NULL) vs (NULL, 5) again
static void null_positions() {
  const int64_t ba[] = {0, 5, 5, 0, 5, 0, 5}, bb[] = {5, 0, 5, 5, 0, 0, 5};
  const bool bva[] = {false, true, true, false, true, false, true}, bvb[] = {true, false, true, true, false, false, true};
  const int64_t pa[] = {0, 5, 5, 0, 5, 7}, pb[] = {5, 0, 5, 0, 7, 5};
  const bool pva[] = {false, true, true, false, true, true}, pvb[] = {true, false, true, false, true, true};
  Side build(2), probe(2);
  for (int c = 0; c < 2; ++c) { build[c].nullable = probe[c].nullable = true; }
  for (int r = 0; r < 7; ++r) { build[0].add(bva[r], raw<int64_t>(ba[r])); build[1].add(bvb[r], raw<int64_t>(bb[r])); }
  for (int r = 0; r < 6; ++r) { probe[0].add(pva[r], raw<int64_t>(pa[r])); probe[1].add(pvb[r], raw<int64_t>(pb[r])); }
  const std::vector<int> got = run_join("null positions", build, 7, probe, 6, 0);
  const int want[6] = {-1, -1, 2, -1, -1, -1};   // only (5, 5) matches, at its first build row
  for (int r = 0; r < 6 && got.size() == 6; ++r) CHECK(got[r] == want[r], "null positions: probe row %d has code %d, expected %d", r, got[r], want[r]);
}

int main() {
  for (size_t B : {0u, 1u, 63u, 64u, 65u, 257u})
    for (size_t P : {0u, 1u, 65u, 300u}) {
      mixed_join(B, P, 1, 0, 1);      // one key on the build side
      mixed_join(B, P, 40, 0, 3);     // duplicate build keys
      mixed_join(B, P, 40, 3, 4);     // 8 hash values: long probe chains, equal tags on different keys
    }
  mixed_join(300, 300, 0, 0, 2, true);   // unique keys, all of them present on both sides unless a NULL hides them
  mixed_join(300, 300, 0, 3, 7, true);
  mixed_join(1000, 5000, 300, 3, 5);
  mixed_join(1000, 5000, 300, 0, 6);
  late_differences();
  prefixes();
  null_positions();
  printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
