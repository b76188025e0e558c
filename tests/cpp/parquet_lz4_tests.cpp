// parquet_lz4_tests.cpp — the lz4 switch of the device Parquet decoder without a device (tests/test_parquet_lz4_cpu.py builds and
// runs this, plainly and under the address and undefined-behaviour sanitizers; nothing of it is loaded into Python). It contains
// the page walk with the lz4 switch (qurious_amd/csrc/parquet_meta.hpp) and the whole of the LZ4 block decoder k_pq_unlz4 runs
// (csrc/device/qhip_lz4.inc: the same text, with loops over 64 lanes where the kernel has its lanes). Every block is decoded
// from and into heap blocks of exactly its sizes — an empty one is an allocation of no bytes — and the tile is a heap block of
// its own.
//
//   streams IN OUT      IN: u32 count, then per block u32 bytes, u32 declared size, the bytes. OUT, per block, after the host's
//                       size check: u32 reason (0, or a QH_PQ_R_LZ4_*), u32 forms (bit QH_LZ4F_*: what of the format the block
//                       used), u32 bytes, the output
//   frames IN OUT       IN as for streams, each entry a page payload of the legacy id. OUT, per payload: u32 verdict (1 Hadoop's
//                       frames, 0 one bare block), u32 reason of a frame the host refuses (0 or a QH_PQ_R_LZ4_*), u32 frames,
//                       then per frame u32 where its block begins, u32 its bytes, u32 its uncompressed size
//   pages FILE TYPES PROJ LEVEL ENCODINGS CODECS GZIP LZ4 OUT
//                       the page walk at the five switches: "NEEDS_HOST reason rowgroup column page", or "PAGES lz4 gzip zstd
//                       snappy" and into OUT, per entry of the LZ4 table in table order: u32 page, u32 reason, u32 where in the
//                       page its slice begins, u32 bytes, the unpacked bytes
//
// The type codes are parquet_tests.cpp's own: that file is included as it is, its main under another name.
static unsigned g_forms;
#define QH_LZ4_FORM(bit) (g_forms |= 1u << (bit))
#define main parquet_tests_main
#include "parquet_tests.cpp"
#undef main

static void put32(FILE* f, uint32_t v) { fwrite(&v, 4, 1, f); }

// a heap block of exactly n bytes
struct Exact {
  std::unique_ptr<uint8_t[]> p;
  size_t n;
  explicit Exact(size_t bytes, int fill = 0) : p(new uint8_t[bytes]), n(bytes) { if (bytes) memset(p.get(), fill, bytes); }
};

// one block, from and into blocks of its own
static uint32_t unlz4(const uint8_t* src, uint32_t n_in, uint8_t* dst, uint32_t n_out) {
  Exact tile(QH_LZ4_TILE, 0xAB);
  return qh_lz4_block(src, n_in, dst, n_out, tile.p.get(), 0);
}

// IN's entries: (bytes, declared size)
static bool entries(const std::vector<uint8_t>& raw, std::vector<std::pair<std::vector<uint8_t>, uint32_t>>* out) {
  size_t at = 4;
  uint32_t count = 0;
  if (raw.size() < 4) return false;
  memcpy(&count, raw.data(), 4);
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t n = 0, declared = 0;
    if (raw.size() - at < 8) return false;
    memcpy(&n, raw.data() + at, 4);
    memcpy(&declared, raw.data() + at + 4, 4);
    at += 8;
    if (raw.size() - at < n) return false;
    out->emplace_back(std::vector<uint8_t>(raw.begin() + (long)at, raw.begin() + (long)(at + n)), declared);
    at += n;
  }
  return true;
}

static int streams(const char* path, const char* out_path) {
  std::vector<std::pair<std::vector<uint8_t>, uint32_t>> all;
  if (!entries(read_file(path), &all)) return 2;
  FILE* f = fopen(out_path, "wb");
  if (!f) return 2;
  for (const auto& e : all) {
    const uint32_t n = (uint32_t)e.first.size(), declared = e.second;
    Exact in(n);
    if (n) memcpy(in.p.get(), e.first.data(), n);
    g_forms = 0;
    uint32_t reason = (uint32_t)qh_lz4_check_sizes(n, declared);   // (the host's part: before a slot is reserved)
    Exact out(reason ? 0 : declared, 0xAB);
    if (!reason) reason = unlz4(in.p.get(), n, out.p.get(), declared);
    put32(f, reason ? QH_PQ_R_LZ4_BASE + reason : 0);
    put32(f, g_forms);
    put32(f, reason ? 0 : declared);
    if (!reason && declared) fwrite(out.p.get(), 1, declared, f);
  }
  fclose(f);
  return 0;
}

static int frames(const char* path, const char* out_path) {
  std::vector<std::pair<std::vector<uint8_t>, uint32_t>> all;
  if (!entries(read_file(path), &all)) return 2;
  FILE* f = fopen(out_path, "wb");
  if (!f) return 2;
  for (const auto& e : all) {
    const uint32_t n = (uint32_t)e.first.size();
    Exact in(n);
    if (n) memcpy(in.p.get(), e.first.data(), n);
    lz4_u32 count = 0;
    int bad = 0;
    const int framed = qh_lz4_hadoop_scan(in.p.get(), n, e.second, &count, &bad);
    put32(f, (uint32_t)framed);
    put32(f, framed && bad ? (uint32_t)(QH_PQ_R_LZ4_BASE + bad) : 0);
    put32(f, framed ? count : 0);
    if (!framed) continue;
    lz4_u64 at = 0;
    lz4_u32 usize = 0, csize = 0;
    while (qh_lz4_hadoop_next(in.p.get(), n, &at, &usize, &csize)) { put32(f, (uint32_t)(at - csize)); put32(f, csize); put32(f, usize); }
  }
  fclose(f);
  return 0;
}

static int pages(const char* path, const char* type_codes, const char* proj_text, int level, int encodings, int codecs, int gzip, int lz4, const char* out_path) {
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
    plan = plan_file(file.p, file.n, nullptr, types, proj, level, encodings, codecs, gzip, lz4);
  } catch (const PqNeedsHost& e) {
    printf("NEEDS_HOST %d %lld %lld %lld\n", e.reason, (long long)e.row_group, (long long)e.column, (long long)e.page);
    return 0;
  }
  FILE* f = fopen(out_path, "wb");
  if (!f) return 2;
  // the slots of the four tables lie in the unpack area, 16-byte aligned, apart from each other; the sources inside the upload.
  // A slot is a page's: the entries of the other three tables fill one each, the LZ4 entries of a page tile theirs in order.
  struct Slot { uint64_t dst, size; };
  std::vector<Slot> slots;
  auto whole = [&](const qh_pq_unpack& u) {
    if (plan.pages[u.page].pos != u.dst || plan.pages[u.page].size != u.dst_size) { fprintf(stderr, "a page that is not its slot\n"); exit(3); }
    slots.push_back(Slot{u.dst, u.dst_size});
  };
  for (const qh_pq_unpack& u : plan.unpack) whole(u);
  for (const qh_pq_unpack& u : plan.unzstd) whole(u);
  for (const qh_pq_unpack& u : plan.ungzip) whole(u);
  for (size_t k = 0; k < plan.unlz4.size();) {
    const uint32_t page = plan.unlz4[k].page;
    uint64_t at = plan.pages[page].pos;
    for (; k < plan.unlz4.size() && plan.unlz4[k].page == page; ++k) {
      if (plan.unlz4[k].dst != at) { fprintf(stderr, "the entries of a page do not tile its slot\n"); return 3; }
      at += plan.unlz4[k].dst_size;
    }
    if (at != plan.pages[page].pos + plan.pages[page].size) { fprintf(stderr, "the entries of a page do not fill its slot\n"); return 3; }
    slots.push_back(Slot{plan.pages[page].pos, plan.pages[page].size});
  }
  uint64_t sum = 0;
  for (const Slot& s : slots) {
    if (s.dst < plan.unpack_base || (s.dst & 15) || s.dst + s.size > plan.packed_bytes()) { fprintf(stderr, "a slot outside the unpack area\n"); return 3; }
    for (const Slot& v : slots)
      if (&v != &s && v.dst < s.dst + s.size && s.dst < v.dst + v.size) { fprintf(stderr, "two slots overlap\n"); return 3; }
    sum += (s.size + 15) & ~(uint64_t)15;
  }
  if (sum != plan.unpack_bytes || (slots.empty() && plan.packed_bytes() != plan.upload_bytes)) { fprintf(stderr, "the unpack area's size is not its slots'\n"); return 3; }
  printf("PAGES %zu %zu %zu %zu\n", plan.unlz4.size(), plan.ungzip.size(), plan.unzstd.size(), plan.unpack.size());
  for (const qh_pq_unpack& u : plan.unlz4) {
    if (u.src + u.src_size > plan.upload_bytes) { fprintf(stderr, "a source outside the upload\n"); return 3; }
    Exact in(u.src_size), out(u.dst_size, 0xAB);
    for (const Range& r : plan.ranges)
      if (u.src_size && u.src >= r.buf_off && u.src + u.src_size <= r.buf_off + r.bytes) memcpy(in.p.get(), file.p + r.file_off + (u.src - r.buf_off), u.src_size);
    const uint32_t reason = unlz4(in.p.get(), u.src_size, out.p.get(), u.dst_size);
    put32(f, u.page);
    put32(f, reason ? QH_PQ_R_LZ4_BASE + reason : 0);
    put32(f, (uint32_t)(u.dst - plan.pages[u.page].pos));
    put32(f, u.dst_size);
    if (u.dst_size) fwrite(out.p.get(), 1, u.dst_size, f);
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "streams")) return streams(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "frames")) return frames(argv[2], argv[3]);
  if (argc == 11 && !strcmp(argv[1], "pages")) return pages(argv[2], argv[3], argv[4], atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), atoi(argv[9]), argv[10]);
  if (argc == 5) return parquet_tests_main(argc, argv);   // (the five-argument calls still answer as they did)
  fprintf(stderr, "usage: streams IN OUT | frames IN OUT | pages FILE TYPES PROJ LEVEL ENCODINGS CODECS GZIP LZ4 OUT\n");
  return 2;
}
