// parquet_gzip_tests.cpp — the gzip switch of the device Parquet decoder without a device (tests/test_parquet_gzip_cpu.py builds
// and runs this, plainly and under the address and undefined-behaviour sanitizers; nothing of it is loaded into Python). It
// contains the page walk with the gzip switch (qurious_amd/csrc/parquet_meta.hpp) and the whole of the DEFLATE decoder
// k_pq_ungzip runs (csrc/device/qhip_inflate.inc: the same text, with loops over 64 lanes where the kernel has its lanes). Every
// member is decoded from and into heap blocks of exactly its sizes, and the tables are a heap block of their own.
//
//   streams IN OUT      IN: u32 count, then per member u32 bytes, u32 declared size, the bytes. OUT, per member, after the host's
//                       check of the member header: u32 reason (0, or a QH_PQ_R_GZIP_*), u32 forms (bit QH_INFLF_*: what of the
//                       format the member used), u32 bytes, the output
//   pages FILE TYPES PROJ LEVEL ENCODINGS CODECS GZIP OUT
//                       the page walk at the four switches: "NEEDS_HOST reason rowgroup column page", or "PAGES gzip zstd snappy"
//                       and into OUT, per GZIP page in table order: u32 page, u32 reason, u32 bytes, the unpacked page
//
// The exactly-sized heap blocks and the type codes are parquet_tests.cpp's own: that file is included as it is, its main under
// another name.
static unsigned g_forms;
#define QH_INFL_FORM(bit) (g_forms |= 1u << (bit))
#define main parquet_tests_main
#include "parquet_tests.cpp"
#undef main

static void put32(FILE* f, uint32_t v) { fwrite(&v, 4, 1, f); }

// one member, from and into blocks of its own
static uint32_t ungzip(const uint8_t* src, uint32_t n_in, uint32_t start, uint8_t* dst, uint32_t n_out) {
  std::unique_ptr<qh_infl_tables> T(new qh_infl_tables);
  memset(T.get(), 0xAB, sizeof(qh_infl_tables));
  return qh_inflate_member(src, n_in, start, dst, n_out, T.get(), 0);
}

static int streams(const char* path, const char* out_path) {
  const std::vector<uint8_t> raw = read_file(path);
  FILE* f = fopen(out_path, "wb");
  if (!f) return 2;
  size_t at = 4;
  uint32_t count = 0;
  if (raw.size() < 4) return 2;
  memcpy(&count, raw.data(), 4);
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t n = 0, declared = 0;
    if (raw.size() - at < 8) return 2;
    memcpy(&n, raw.data() + at, 4);
    memcpy(&declared, raw.data() + at + 4, 4);
    at += 8;
    if (raw.size() - at < n) return 2;
    Heap in(n);
    if (n) memcpy(in.p, raw.data() + at, n);
    at += n;
    infl_u32 start = 0;
    g_forms = 0;
    uint32_t reason = (uint32_t)qh_gzip_check_member(in.p, in.n, declared, &start);   // (the host's part: before a slot is reserved)
    Heap out(reason ? 0 : declared, 0xAB);
    if (!reason) reason = ungzip(in.p, (uint32_t)in.n, start, out.p, (uint32_t)out.n);
    put32(f, reason ? QH_PQ_R_GZIP_BASE + reason : 0);
    put32(f, g_forms);
    put32(f, reason ? 0 : declared);
    if (!reason && declared) fwrite(out.p, 1, declared, f);
  }
  fclose(f);
  return 0;
}

static int pages(const char* path, const char* type_codes, const char* proj_text, int level, int encodings, int codecs, int gzip, const char* out_path) {
  const std::vector<uint8_t> raw = read_file(path);
  Heap file(raw.size());
  if (!raw.empty()) memcpy(file.p, raw.data(), raw.size());
  std::vector<ArrowType> types;
  for (const char* p = type_codes; *p;) {
    const char* e = strchr(p, ',');
    types.push_back(parse_type(e ? std::string(p, e) : std::string(p)));
    if (!e) break;
    p = e + 1;
  }
  std::vector<int32_t> proj;
  if (strcmp(proj_text, "-") != 0) for (const char* p = proj_text; *p;) { proj.push_back(atoi(p)); const char* e = strchr(p, ','); if (!e) break; p = e + 1; }
  else for (size_t k = 0; k < types.size(); ++k) proj.push_back((int32_t)k);
  Plan plan;
  try {
    plan = plan_file(file.p, file.n, nullptr, types, proj, level, encodings, codecs, gzip);
  } catch (const PqNeedsHost& e) {
    printf("NEEDS_HOST %d %lld %lld %lld\n", e.reason, (long long)e.row_group, (long long)e.column, (long long)e.page);
    return 0;
  }
  FILE* f = fopen(out_path, "wb");
  if (!f) return 2;
  // the slots of the three tables lie in the unpack area, 16-byte aligned, apart from each other; the sources inside the upload
  std::vector<const qh_pq_unpack*> all;
  for (const qh_pq_unpack& u : plan.unpack) all.push_back(&u);
  for (const qh_pq_unpack& u : plan.unzstd) all.push_back(&u);
  for (const qh_pq_unpack& u : plan.ungzip) all.push_back(&u);
  uint64_t sum = 0;
  for (const qh_pq_unpack* u : all) {
    if (u->dst < plan.unpack_base || (u->dst & 15) || u->dst + u->dst_size > plan.packed_bytes() || u->src + u->src_size > plan.upload_bytes) { fprintf(stderr, "a slot outside the unpack area\n"); return 3; }
    if (plan.pages[u->page].pos != u->dst || plan.pages[u->page].size != u->dst_size) { fprintf(stderr, "a page that is not its slot\n"); return 3; }
    for (const qh_pq_unpack* v : all)
      if (v != u && v->dst < u->dst + u->dst_size && u->dst < v->dst + v->dst_size) { fprintf(stderr, "two slots overlap\n"); return 3; }
    sum += ((uint64_t)u->dst_size + 15) & ~(uint64_t)15;
  }
  if (sum != plan.unpack_bytes || (all.empty() && plan.packed_bytes() != plan.upload_bytes)) { fprintf(stderr, "the unpack area's size is not its slots'\n"); return 3; }
  printf("PAGES %zu %zu %zu\n", plan.ungzip.size(), plan.unzstd.size(), plan.unpack.size());
  for (const qh_pq_unpack& u : plan.ungzip) {
    Heap in(u.src_size), out(u.dst_size, 0xAB);
    for (const Range& r : plan.ranges)
      if (u.src >= r.buf_off && u.src + u.src_size <= r.buf_off + r.bytes) memcpy(in.p, file.p + r.file_off + (u.src - r.buf_off), u.src_size);
    const uint32_t reason = ungzip(in.p, u.src_size, u.start, out.p, u.dst_size);
    put32(f, u.page);
    put32(f, reason ? QH_PQ_R_GZIP_BASE + reason : 0);
    put32(f, u.dst_size);
    if (u.dst_size) fwrite(out.p, 1, u.dst_size, f);
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "streams")) return streams(argv[2], argv[3]);
  if (argc == 10 && !strcmp(argv[1], "pages")) return pages(argv[2], argv[3], argv[4], atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), argv[9]);
  if (argc == 5) return parquet_tests_main(argc, argv);   // (the five-argument calls still answer as they did)
  fprintf(stderr, "usage: streams IN OUT | pages FILE TYPES PROJ LEVEL ENCODINGS CODECS GZIP OUT\n");
  return 2;
}
