// parquet_snappy_tests.cpp — format level 2 of the device Parquet decoder without a device (tests/test_parquet_snappy_cpu.py
// builds and runs this, plainly and under the address and undefined-behaviour sanitizers; nothing of it is loaded into Python).
// It contains the page walk at level 2 (qurious_amd/csrc/parquet_meta.hpp) and the token code of k_pq_unsnap
// (csrc/device/qhip_snappy.inc), driven by loops that stand for the 64 lanes of kernels_parquet.hip. Every buffer is a heap
// allocation of exactly the size its data has: a stream's input, its output, the device buffer of a whole file.
//
//   decode FILE TYPES PROJ LEVEL   as parquet_tests' decode, at format level LEVEL: the Snappy pages are unpacked into the unpack
//                                  area first -> "ROWS n", "NULLS ..", rows | "NEEDS_HOST reason rowgroup column page"
//   streams FILE                   FILE: u32 count, then per stream u32 bytes, u32 declared size, the bytes. Per stream, after the
//                                  host's checks of its sizes: "OK <hex of the output>" or "REASON r" (r: a QH_PQ_R_SNAPPY_*)
//
// The level, string and value passes, the exactly-sized heap blocks and the type codes are parquet_tests.cpp's own: that file is
// included as it is, its main under another name.
#define main parquet_tests_main
#include "parquet_tests.cpp"
#undef main

// ---- k_pq_unsnap, one stream: the walk is the kernel's; a lane loop stands where the kernel spreads bytes over the lanes, and
// a copy's lanes all load before any of them stores, as one vector load and one vector store do
static uint32_t unsnap(const uint8_t* src, uint64_t n_in, uint32_t start, uint8_t* dst, uint64_t n_out) {
  uint64_t ip = start, op = 0;
  while (ip < n_in) {
    if (op == n_out) return QH_SNAP_E_INPUT;
    qh_snap_elem e;
    int reason = qh_snap_element(src + ip, n_in - ip, &e);
    if (reason) return (uint32_t)reason;
    ip += e.header;
    reason = qh_snap_check(&e, n_in - ip, op, n_out);
    if (reason) return (uint32_t)reason;
    if (e.kind == QH_SNAP_LITERAL) {
      for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint64_t i = lane; i < e.len; i += 64) dst[op + i] = src[ip + i];
      ip += e.len;
    } else {
      uint8_t got[64];
      for (uint32_t lane = 0; lane < 64; ++lane) if (lane < e.len) got[lane] = dst[qh_snap_copy_src(op, e.offset, lane)];
      for (uint32_t lane = 0; lane < 64; ++lane) if (lane < e.len) dst[op + lane] = got[lane];
    }
    op += e.len;
  }
  return op != n_out ? (uint32_t)QH_SNAP_E_INPUT : (uint32_t)QH_SNAP_OK;
}

static int streams(const char* path) {
  const std::vector<uint8_t> raw = read_file(path);
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
    sn_u32 start = 0;
    uint32_t reason = (uint32_t)qh_snap_check_sizes(in.p, in.n, declared, &start);   // (the host's part: before a slot is reserved)
    if (reason) { printf("REASON %u\n", QH_PQ_R_SNAPPY_BASE + reason); continue; }
    Heap out(declared, 0xAB);
    reason = unsnap(in.p, in.n, start, out.p, out.n);
    if (reason) { printf("REASON %u\n", QH_PQ_R_SNAPPY_BASE + reason); continue; }
    printf("OK ");
    for (size_t b = 0; b < out.n; ++b) printf("%02x", out.p[b]);
    printf("\n");
  }
  return 0;
}

// ---- a whole file at a format level (parquet_tests.cpp's decode, with the unpack pass in front and the buffer sized for it)
static int decode2(const char* path, const char* type_codes, const char* proj_text, int level) {
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
    plan = plan_file(file.p, file.n, nullptr, types, proj, level);
  } catch (const PqNeedsHost& e) {
    printf("NEEDS_HOST %d %lld %lld %lld\n", e.reason, (long long)e.row_group, (long long)e.column, (long long)e.page);
    return 0;
  }
  const uint64_t R = plan.num_rows, words = (R + 63) / 64, buf_bytes = plan.buffer_bytes();
  Heap buf((size_t)buf_bytes, 0xAB);   // (no slack: the device's vector loads read it, these loops must not)
  for (const Range& r : plan.ranges) memcpy(buf.p + r.buf_off, file.p + r.file_off, (size_t)r.bytes);
  FirstError unpack_err;
  uint64_t slot_end = plan.unpack_base;
  for (const qh_pq_unpack& u : plan.unpack) {
    // the slots lie one behind the other, 16-byte aligned, behind the upload; the sources inside it
    if (u.dst != slot_end || (u.dst & 15) || u.dst + u.dst_size > buf_bytes || u.src + u.src_size > plan.upload_bytes) { fprintf(stderr, "a slot outside the unpack area\n"); return 3; }
    slot_end = u.dst + (((uint64_t)u.dst_size + 15) & ~(uint64_t)15);
    if (plan.pages[u.page].pos != u.dst || plan.pages[u.page].size != u.dst_size) { fprintf(stderr, "a page that is not its slot\n"); return 3; }
    // each stream from and into blocks of its own exact size, so that one page cannot read or write another's bytes unseen
    Heap in(u.src_size), out(u.dst_size, 0xAB);
    memcpy(in.p, buf.p + u.src, u.src_size);
    const uint32_t reason = unsnap(in.p, in.n, u.start, out.p, out.n);
    if (reason) unpack_err.report(u.page, QH_PQ_R_SNAPPY_BASE + reason);
    memcpy(buf.p + u.dst, out.p, u.dst_size);
  }
  if (slot_end != buf_bytes && !plan.unpack.empty()) { fprintf(stderr, "the unpack area's size is not its slots'\n"); return 3; }
  const size_t ncols = proj.size();
  std::vector<std::unique_ptr<Heap>> keep;
  auto heap = [&](size_t n, int fill) { keep.emplace_back(new Heap(n, fill)); return keep.back()->p; };
  std::vector<qh_pq_col> cols(ncols);
  for (size_t k = 0; k < ncols; ++k) {
    const ColPlan& cp = plan.cols[k];
    qh_pq_col& d = cols[k];
    memset(&d, 0, sizeof d);
    if (cp.optional) d.valid = (pq_u64*)heap(words * 8, 0);
    if (cp.utf8) {
      d.values = heap((size_t)(R + 1) * 4, 0xAB);
      d.strpos = (pq_u64*)heap((size_t)R * 8, 0xAB);
      d.ent = (qh_pq_ent*)heap((size_t)(R + cp.dict_entries) * sizeof(qh_pq_ent), 0xAB);
    } else if (cp.boolean) d.values = heap(words * 8, 0);
    else d.values = heap((size_t)R * cp.width, 0xAB);
    d.phys = cp.phys; d.flba = cp.flba; d.width = cp.width; d.narrow = cp.narrow;
  }
  // the later passes run whatever the unpack pass found, as on the device: they must stay inside the slots of refused pages
  std::vector<qh_pq_state> state(plan.pages.size());
  std::vector<uint64_t> nulls(ncols, 0), utf8(ncols, 0);
  FirstError err;
  for (size_t p = 0; p < plan.pages.size(); ++p)
    if (plan.pages[p].enc != QH_PQ_ENC_DICTPAGE) levels_page(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err, nulls[plan.pages[p].col]);
  if (err.word == ~0ULL)
    for (size_t p = 0; p < plan.pages.size(); ++p) strings_page(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err);
  if (err.word == ~0ULL)
    for (size_t p = 0; p < plan.pages.size(); ++p)
      if (plan.pages[p].enc != QH_PQ_ENC_DICTPAGE) values_page(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err, utf8[plan.pages[p].col]);
  const uint64_t offender = unpack_err.word != ~0ULL ? unpack_err.word : err.word;   // (the unpack word first, as parquet.cpp reads them)
  if (offender != ~0ULL) {
    const PageWhere& w = plan.where[(size_t)(offender >> 8)];
    printf("NEEDS_HOST %d %lld %lld %lld\n", (int)(offender & 0xFF), (long long)w.row_group, (long long)w.column, (long long)w.page);
    return 0;
  }
  printf("ROWS %llu\nNULLS", (unsigned long long)R);
  for (size_t k = 0; k < ncols; ++k) printf(" %llu", (unsigned long long)nulls[k]);
  printf("\n");
  for (uint64_t r = 0; r < R; ++r) {
    for (size_t k = 0; k < ncols; ++k) {
      const qh_pq_col& d = cols[k];
      const ArrowType& ty = types[(size_t)proj[k]];
      if (k) putchar('\t');
      if (d.valid && !((d.valid[r >> 6] >> (r & 63)) & 1)) { putchar('N'); continue; }
      switch (ty.id) {
        case QHIP_BOOL: putchar((((uint64_t*)d.values)[r >> 6] >> (r & 63)) & 1 ? '1' : '0'); break;
        case QHIP_INT8: printf("%d", (int)((int8_t*)d.values)[r]); break;
        case QHIP_INT16: printf("%d", (int)((int16_t*)d.values)[r]); break;
        case QHIP_INT32: case QHIP_DATE32: printf("%d", ((int32_t*)d.values)[r]); break;
        case QHIP_UINT8: printf("%u", (unsigned)((uint8_t*)d.values)[r]); break;
        case QHIP_UINT16: printf("%u", (unsigned)((uint16_t*)d.values)[r]); break;
        case QHIP_UINT32: printf("%u", ((uint32_t*)d.values)[r]); break;
        case QHIP_FLOAT32: printf("%08x", ((uint32_t*)d.values)[r]); break;
        case QHIP_UINT64: printf("%llu", (unsigned long long)((uint64_t*)d.values)[r]); break;
        case QHIP_FLOAT64: printf("%016llx", (unsigned long long)((uint64_t*)d.values)[r]); break;
        case QHIP_DECIMAL128: print_i128(((uint64_t*)d.values)[2 * r], ((uint64_t*)d.values)[2 * r + 1]); break;
        case QHIP_UTF8: {
          putchar('s');
          const uint32_t len = ((uint32_t*)d.values)[r];
          const uint64_t pos = d.strpos[r];
          if (pos > buf_bytes || len > buf_bytes - pos) { fprintf(stderr, "a string outside the buffer\n"); return 3; }
          for (uint32_t b = 0; b < len; ++b) printf("%02x", buf.p[pos + b]);
          break;
        }
        default: printf("%lld", (long long)((int64_t*)d.values)[r]); break;   // Int64, Timestamp
      }
    }
    putchar('\n');
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "decode")) return decode2(argv[2], argv[3], argv[4], atoi(argv[5]));
  if (argc == 3 && !strcmp(argv[1], "streams")) return streams(argv[2]);
  if (argc == 5) return parquet_tests_main(argc, argv);   // (the five-argument calls still answer as they did)
  fprintf(stderr, "usage: decode FILE TYPES PROJ LEVEL | streams FILE\n");
  return 2;
}
