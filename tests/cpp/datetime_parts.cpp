// The date code of EXTRACT (qurious_amd/csrc/device/qhip_datetime.inc) as plain host C++, for tests/test_extract_cpu.py.
//
//   datetime_parts UNIT IN OUT
//
// UNIT: -1 Date32 (days), 0 / 3 / 6 / 9 Timestamp(s / ms / us / ns), Date64 = 3. IN: n little-endian int64 values. OUT: for every
// part in QH_DT_* order (year, month, day, hour, minute, second, week) n int64 results, then for every part n validity bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../qurious_amd/csrc/device/qhip_datetime.inc"

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s UNIT IN OUT\n", argv[0]); return 2; }
  const int unit = atoi(argv[1]);
  FILE* f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 1; }
  std::vector<long long> in;
  long long buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(long long), 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(f);
  const int parts = QH_DT_WEEK + 1;
  const size_t n = in.size();
  std::vector<long long> val(n * parts);
  std::vector<unsigned char> ok(n * parts);
  for (int p = 0; p < parts; ++p)
    for (size_t i = 0; i < n; ++i) {
      long long r = 0;
      ok[(size_t)p * n + i] = qh_dt_extract(p, unit, in[i], r) ? 1 : 0;
      val[(size_t)p * n + i] = r;
    }
  FILE* o = fopen(argv[3], "wb");
  if (!o) { perror(argv[3]); return 1; }
  if (fwrite(val.data(), sizeof(long long), val.size(), o) != val.size() || fwrite(ok.data(), 1, ok.size(), o) != ok.size()) return 1;
  return fclose(o) == 0 ? 0 : 1;
}
