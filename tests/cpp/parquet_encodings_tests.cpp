// parquet_encodings_tests.cpp — encoding set 2 of the device Parquet decoder without a device (tests/test_parquet_encodings_cpu.py
// builds and runs this, plainly and under the address and undefined-behaviour sanitizers; nothing of it is loaded into Python).
// It contains the page walk at an encoding set (qurious_amd/csrc/parquet_meta.hpp: DataPageHeaderV2, the new encodings, the
// decoded area) and the code the kernels share with the host (csrc/device/qhip_parquet.inc, qhip_delta.inc), driven by loops
// that stand for the 64 lanes of k_pq_levels, k_pq_delta and k_pq_values_ext. Every stream is decoded from and into heap blocks
// of exactly its size.
//
//   decode FILE TYPES PROJ LEVEL ENCODINGS   as parquet_snappy_tests' decode, at an encoding set
//   delta FILE    FILE: u32 count, then per stream u32 bytes, u32 width (4 | 8), u32 expected count, the bytes. Per stream
//                 "OK end v0 v1 .." (unsigned, of the width) or "REASON r"
//   header HEX SET2                          one Thrift page header: "type num_values encoding has_v2 header_bytes"
//
// The unpack pass, the string pass, the exactly-sized heap blocks and the type codes are the other two files' own: they are
// included as they are, in a namespace of their own, so that their main is not this one. That holds only while every header
// those two files include (parquet_snappy_tests.cpp, and parquet_tests.cpp through it) is included here first, outside the
// namespace: their include guards then make the inner #include lines empty. A header added to either of them must be added to
// the list below as well, or its declarations land inside other_programs and this file stops compiling, with errors that point
// into the standard library. The older files cannot offer their helpers in a header of their own without being changed, and
// existing test files stay as they are.
//
// levels_page2, delta_stream and values_page2 below are the kernels' bodies (kernels_parquet.hip: k_pq_levels' V2 branch,
// k_pq_delta, pq_values_body's kExt branches) written out again with loops for the lanes; only the QH_PQ_HD functions they call
// are one text for both compilers. What keeps the copies and the kernels together is the GPU suite: tests/test_gpu_parquet_encodings.py
// decodes the same files and the same raw streams on the device and compares with what these loops answered. A change to a
// kernel's body is made here too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "parquet_meta.hpp"

namespace other_programs {
#include "parquet_snappy_tests.cpp"
}
using namespace other_programs;
using namespace qhip_pq;

// ---- k_pq_levels, one page, with the V2 placement
static void levels_page2(const uint8_t* buf, const qh_pq_page& pg, const qh_pq_col& col, qh_pq_state& st, uint64_t page, FirstError& err, uint64_t& nulls) {
  if (!(pg.flags & QH_PQ_F_V2)) { levels_page(buf, pg, col, st, page, err, nulls); return; }
  const uint64_t n = pg.num_values;
  if (!col.valid) { st.nonnull = (uint32_t)n; st.values_off = 0; return; }
  Heap lev(pg.lev_size);   // (exactly the level bytes)
  memcpy(lev.p, buf + pg.lev_pos, pg.lev_size);
  const uint8_t* s = lev.p;
  const uint32_t len = pg.lev_size;
  uint32_t reason = QH_PQ_OK;
  pq_u64 cpos = 0;
  uint64_t row = 0, nonnull = 0;
  qh_pq_run run;
  qh_pq_run_init(&run);
  while (!reason && row < n) {
    reason = (uint32_t)qh_pq_next_run(s, len, &cpos, 1, &run);
    if (reason) break;
    uint64_t take = run.count;
    const uint64_t left = n - row;
    if (run.packed) { if (take >= left + 8) reason = QH_PQ_R_RUN_COUNT; else if (take > left) take = left; }
    else if (take > left) reason = QH_PQ_R_RUN_COUNT;
    else if (run.value > 1) reason = QH_PQ_R_LEVEL_VALUE;
    if (reason) break;
    const uint64_t g0 = pg.first_row + row;
    if (run.packed || run.value)
      for (uint64_t w = g0 >> 6; w <= ((g0 + take - 1) >> 6); ++w) {
        const uint64_t bits = qh_pq_level_word(s, &run, g0, take, w);
        if (w * 64 >= g0 && w * 64 + 64 <= g0 + take) col.valid[w] = bits; else col.valid[w] |= bits;
        nonnull += (uint64_t)__builtin_popcountll(bits);
      }
    row += take;
  }
  st.nonnull = (uint32_t)nonnull;
  st.values_off = 0;
  if (!reason && n - nonnull != (uint64_t)pg.num_nulls) reason = QH_PQ_R_V2_NULLS;
  if (reason) err.report(page, reason); else nulls += n - nonnull;
}

// ---- k_pq_delta, one stream s[0 .. size) of `count` expected values: the walk is the kernel's, the arrays stand for the lanes.
// Dense values go to out (count * width bytes); lengths become ent[0 .. count) with positions relative to `src`.
static uint32_t delta_stream(const uint8_t* s, uint64_t size, uint64_t count, uint32_t width, bool lengths, uint8_t* out, qh_pq_ent* ent, uint64_t src, uint64_t* end) {
  const uint32_t bits = width * 8;
  qh_dl_head h;
  memset(&h, 0, sizeof h);
  uint32_t reason = (uint32_t)qh_dl_header(s, size, &h);
  if (!reason && (uint64_t)h.total != count) reason = QH_PQ_R_DELTA_COUNT;
  uint64_t pos = 0, carry = 0, produced = 0, sum = 0;
  auto store = [&](uint64_t i, uint64_t v) { if (width == 4) { const uint32_t x = (uint32_t)v; memcpy(out + 4 * i, &x, 4); } else memcpy(out + 8 * i, &v, 8); };
  if (!reason) {
    pos = h.end;
    if (count) {
      carry = h.first; produced = 1;
      if (lengths) {
        if ((int)(uint32_t)carry < 0) reason = QH_PQ_R_DELTA_LENGTH;
        else { ent[0].pos = 0; ent[0].len = (uint32_t)carry; ent[0].pad = 0; }
        sum = (uint32_t)carry;
      } else store(0, carry);
    }
  }
  while (!reason && produced < count) {
    pq_u64 min_delta = 0, wat = 0, at = 0;
    reason = (uint32_t)qh_dl_block(s, size, pos, h.mpb, &min_delta, &wat, &at);
    if (reason) break;
    const uint64_t left = count - produced, in_block = left < (uint64_t)h.block ? left : (uint64_t)h.block;
    const uint64_t mbytes = h.vpm >> 3;
    uint32_t cur_m = 0, cur_w = s[wat];
    reason = (uint32_t)qh_dl_miniblock(cur_w, bits, h.vpm, size - at);
    for (uint64_t k0 = 0; !reason && k0 < in_block; k0 += 64) {
      const uint64_t last = k0 + 63 < in_block ? k0 + 63 : in_block - 1;
      const uint32_t m_lo = (uint32_t)(k0 / h.vpm), m_hi = (uint32_t)(last / h.vpm);
      if (m_lo != cur_m) {
        at += mbytes * cur_w; cur_m = m_lo; cur_w = s[wat + cur_m];
        reason = (uint32_t)qh_dl_miniblock(cur_w, bits, h.vpm, size - at);
        if (reason) break;
      }
      uint64_t next_at = 0;
      uint32_t next_w = 0;
      if (m_hi != m_lo) {
        next_at = at + mbytes * cur_w; next_w = s[wat + m_hi];
        reason = (uint32_t)qh_dl_miniblock(next_w, bits, h.vpm, size - next_at);
        if (reason) break;
      }
      uint64_t val[64];
      bool active[64];
      uint64_t run = carry;
      for (int lane = 0; lane < 64; ++lane) {   // (the inclusive scan: lane l holds carry + x[0] + .. + x[l])
        const uint64_t v = k0 + (uint64_t)lane;
        active[lane] = v <= last;
        uint64_t x = 0;
        if (active[lane]) {
          const uint32_t mi = (uint32_t)(v / h.vpm);
          const uint64_t kk = v - (uint64_t)mi * h.vpm;
          x = (mi == m_lo ? qh_dl_extract(s + at, kk, cur_w) : qh_dl_extract(s + next_at, kk, next_w)) + min_delta;
        }
        run += x;
        val[lane] = run;
      }
      carry = val[63];
      if (lengths) {
        for (int lane = 0; lane < 64; ++lane) if (active[lane] && (int)(uint32_t)val[lane] < 0) reason = QH_PQ_R_DELTA_LENGTH;
        if (reason) break;
        for (int lane = 0; lane < 64; ++lane) {
          if (!active[lane]) continue;
          const uint32_t len = (uint32_t)val[lane];
          qh_pq_ent& e = ent[produced + k0 + (uint64_t)lane];
          e.pos = sum; e.len = len; e.pad = 0;
          sum += len;
        }
      } else {
        for (int lane = 0; lane < 64; ++lane) if (active[lane]) store(produced + k0 + (uint64_t)lane, val[lane]);
      }
      if (m_hi != m_lo) { at = next_at; cur_w = next_w; cur_m = m_hi; }
    }
    if (reason) break;
    pos = at + mbytes * cur_w;
    produced += in_block;
  }
  if (!reason && lengths) {
    if (sum > size - pos) reason = QH_PQ_R_DELTA_LENGTH;
    else for (uint64_t i = 0; i < count; ++i) ent[i].pos += src + pos;
  }
  *end = pos;
  return reason;
}

// ---- k_pq_values_ext, one page (parquet_tests.cpp's values_page with the body's kExt branches)
static void values_page2(const uint8_t* buf, const qh_pq_page& pg, const qh_pq_col& col, const qh_pq_state& st, uint64_t page, FirstError& err, uint64_t& utf8_bytes) {
  if (pg.enc < QH_PQ_ENC_RLE_BOOL) { values_page(buf, pg, col, st, page, err, utf8_bytes); return; }
  const uint64_t nn = st.nonnull;
  const uint32_t pw = qh_pq_phys_bytes(col.phys, col.flba);
  const bool delta = pg.enc == QH_PQ_ENC_DELTA, rleb = pg.enc == QH_PQ_ENC_RLE_BOOL, bss = pg.enc == QH_PQ_ENC_BSS;
  const uint64_t vsize = delta ? nn * pw : (uint64_t)pg.size - st.values_off;
  Heap region((size_t)vsize);   // (exactly the values region: a gather outside it is a report)
  if (vsize) memcpy(region.p, delta ? buf + pg.dict_pos : buf + pg.pos + st.values_off, (size_t)vsize);
  const uint8_t* v = region.p;
  uint32_t reason = QH_PQ_OK, w = 0;
  const uint8_t* s = v;
  uint64_t slen = 0;
  if (rleb) {
    if (nn) {
      if (vsize < 4) reason = QH_PQ_R_RLE_LENGTH;
      else { slen = qh_pq_le32(v); s = v + 4; w = 1; if (slen > vsize - 4) reason = QH_PQ_R_RLE_LENGTH; }
    }
  } else if (bss) { if (nn * pw != vsize) reason = QH_PQ_R_BSS_SIZE; }
  else if (col.phys == QH_PQ_P_BOOL) { if ((nn + 7) / 8 > vsize) reason = QH_PQ_R_VALUES_SHORT; }
  else if (col.phys != QH_PQ_P_BYTES) { if (nn * pw > vsize) reason = QH_PQ_R_VALUES_SHORT; }
  qh_pq_run run;
  qh_pq_run_init(&run);
  pq_u64 cpos = 0;
  uint64_t base = 0, bytes = 0;
  const uint64_t r_begin = pg.first_row, r_end = r_begin + pg.num_values;
  for (uint64_t t0 = r_begin & ~(uint64_t)63; !reason && t0 < r_end; t0 += 64) {
    bool in[64], valid[64];
    uint64_t idx[64];
    uint32_t index[64] = {0};
    for (int l = 0; l < 64; ++l) {
      const uint64_t row = t0 + (uint64_t)l;
      in[l] = row >= r_begin && row < r_end;
      valid[l] = in[l] && (!col.valid || ((col.valid[t0 >> 6] >> l) & 1ULL));
      idx[l] = base;
      if (valid[l]) ++base;
    }
    if (base > nn) { reason = QH_PQ_R_VALUES_SHORT; break; }
    if (rleb) {
      reason = cursor_step(s, slen, &cpos, w, &run, valid, idx, base, index);
      if (reason) break;
      for (int l = 0; l < 64; ++l) if (valid[l] && index[l] > 1) reason = QH_PQ_R_RLE_LENGTH;
      if (reason) break;
    }
    uint64_t word = 0;
    for (int l = 0; l < 64 && !reason; ++l) {
      const uint64_t row = t0 + (uint64_t)l;
      pq_u64 lo = 0, hi = 0;
      if (col.phys == QH_PQ_P_BYTES) {
        if (!in[l]) continue;
        qh_pq_ent e; e.pos = 0; e.len = 0; e.pad = 0;
        if (valid[l]) e = col.ent[pg.ent + idx[l]];
        ((uint32_t*)col.values)[row] = e.len; col.strpos[row] = e.pos; bytes += e.len;
      } else if (col.phys == QH_PQ_P_BOOL) {
        if (valid[l] && (rleb ? index[l] != 0 : (bool)((v[idx[l] >> 3] >> (idx[l] & 7)) & 1))) word |= 1ULL << l;
      } else {
        if (valid[l]) {
          if (bss) qh_pq_read_value_bss(v, nn, idx[l], col.phys, col.flba, &lo, &hi);
          else qh_pq_read_value(v + idx[l] * pw, col.phys, col.flba, &lo, &hi);
          if (col.narrow && !qh_pq_in_range(lo, col.width, col.narrow)) { reason = QH_PQ_R_RANGE; break; }
        }
        if (in[l]) qh_pq_store(col.values, row, col.width, lo, hi);
      }
    }
    if (col.phys == QH_PQ_P_BOOL && word) ((uint64_t*)col.values)[t0 >> 6] |= word;
  }
  if (reason) err.report(page, reason); else utf8_bytes += bytes;
}

// ---- a whole file at a format level and an encoding set
static int decode3(const char* path, const char* type_codes, const char* proj_text, int level, int encodings) {
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
    plan = plan_file(file.p, file.n, nullptr, types, proj, level, encodings);
  } catch (const PqNeedsHost& e) {
    printf("NEEDS_HOST %d %lld %lld %lld\n", e.reason, (long long)e.row_group, (long long)e.column, (long long)e.page);
    return 0;
  }
  const uint64_t R = plan.num_rows, words = (R + 63) / 64, buf_bytes = plan.buffer_bytes();
  Heap buf((size_t)buf_bytes, 0xAB);
  for (const Range& r : plan.ranges) memcpy(buf.p + r.buf_off, file.p + r.file_off, (size_t)r.bytes);
  FirstError unpack_err;
  uint64_t slot_end = plan.unpack_base;
  for (const qh_pq_unpack& u : plan.unpack) {
    if (u.dst != slot_end || (u.dst & 15) || u.dst + u.dst_size > plan.packed_bytes() || u.src + u.src_size > plan.upload_bytes) { fprintf(stderr, "a slot outside the unpack area\n"); return 3; }
    slot_end = u.dst + (((uint64_t)u.dst_size + 15) & ~(uint64_t)15);
    if (plan.pages[u.page].pos != u.dst || plan.pages[u.page].size != u.dst_size) { fprintf(stderr, "a page that is not its slot\n"); return 3; }
    Heap in(u.src_size), out(u.dst_size, 0xAB);
    memcpy(in.p, buf.p + u.src, u.src_size);
    const uint32_t reason = unsnap(in.p, in.n, u.start, out.p, out.n);
    if (reason) unpack_err.report(u.page, QH_PQ_R_SNAPPY_BASE + reason);
    memcpy(buf.p + u.dst, out.p, u.dst_size);
  }
  if (!plan.unpack.empty() && slot_end != plan.packed_bytes()) { fprintf(stderr, "the unpack area's size is not its slots'\n"); return 3; }
  for (const qh_pq_page& pg : plan.pages)   // a V2 page's levels lie in the upload, every page inside the buffer
    if (pg.pos + pg.size > buf_bytes || ((pg.flags & QH_PQ_F_V2) && pg.lev_pos + pg.lev_size > plan.upload_bytes)) { fprintf(stderr, "a page outside the buffer\n"); return 3; }
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
  std::vector<qh_pq_state> state(plan.pages.size());
  std::vector<uint64_t> nulls(ncols, 0), utf8(ncols, 0);
  FirstError err;
  for (size_t p = 0; p < plan.pages.size(); ++p)
    if (plan.pages[p].enc != QH_PQ_ENC_DICTPAGE) levels_page2(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err, nulls[plan.pages[p].col]);
  // the delta pass: each stream from a block of exactly its bytes into a block of exactly its slot
  uint64_t dslot_end = plan.decoded_base;
  if (err.word == ~0ULL)
    for (const qh_pq_dstream& d : plan.delta) {
      const qh_pq_page& pg = plan.pages[d.page];
      const qh_pq_state& st = state[d.page];
      const bool lengths = d.width & QH_PQ_DS_LENGTHS;
      const uint32_t width = d.width & 0xFF;
      const uint64_t slot = (uint64_t)pg.num_values * width;
      if (!lengths) {
        if (d.dst != dslot_end || (d.dst & 15) || d.dst + slot > buf_bytes || pg.dict_pos != d.dst) { fprintf(stderr, "a slot outside the decoded area\n"); return 3; }
        dslot_end = d.dst + ((slot + 15) & ~(uint64_t)15);
      }
      if (!st.nonnull) continue;
      const uint64_t src = pg.pos + st.values_off, size = (uint64_t)pg.size - st.values_off;
      Heap in((size_t)size), out(lengths ? 0 : (size_t)((uint64_t)st.nonnull * width), 0xAB);
      if (size) memcpy(in.p, buf.p + src, (size_t)size);
      std::unique_ptr<qh_pq_ent[]> ents(new qh_pq_ent[lengths ? st.nonnull : 1]);   // (exactly the page's entries)
      uint64_t end = 0;
      const uint32_t reason = delta_stream(in.p, size, st.nonnull, width, lengths, out.p, ents.get(), src, &end);
      if (reason) { err.report(d.page, reason); continue; }
      if (lengths) memcpy(cols[pg.col].ent + pg.ent, ents.get(), (size_t)st.nonnull * sizeof(qh_pq_ent));
      else memcpy(buf.p + d.dst, out.p, out.n);
    }
  if (plan.decoded_bytes && dslot_end != buf_bytes && err.word == ~0ULL) { fprintf(stderr, "the decoded area's size is not its slots'\n"); return 3; }
  if (err.word == ~0ULL)
    for (size_t p = 0; p < plan.pages.size(); ++p)
      if (plan.pages[p].enc != QH_PQ_ENC_DELTA_LEN) strings_page(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err);
  if (err.word == ~0ULL)
    for (size_t p = 0; p < plan.pages.size(); ++p)
      if (plan.pages[p].enc != QH_PQ_ENC_DICTPAGE) values_page2(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err, utf8[plan.pages[p].col]);
  const uint64_t offender = unpack_err.word != ~0ULL ? unpack_err.word : err.word;
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

// ---- raw streams, as qhip_parquet_delta_decode takes them
static int delta_streams(const char* path) {
  const std::vector<uint8_t> raw = read_file(path);
  size_t at = 4;
  uint32_t count = 0;
  if (raw.size() < 4) return 2;
  memcpy(&count, raw.data(), 4);
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t n = 0, width = 0, expect = 0;
    if (raw.size() - at < 12) return 2;
    memcpy(&n, raw.data() + at, 4);
    memcpy(&width, raw.data() + at + 4, 4);
    memcpy(&expect, raw.data() + at + 8, 4);
    at += 12;
    if (raw.size() - at < n || (width != 4 && width != 8)) return 2;
    Heap in(n), out((size_t)expect * width, 0xAB);
    if (n) memcpy(in.p, raw.data() + at, n);
    at += n;
    uint64_t end = 0;
    const uint32_t reason = delta_stream(in.p, in.n, expect, width, false, out.p, nullptr, 0, &end);
    if (reason) { printf("REASON %u\n", reason); continue; }
    printf("OK %llu", (unsigned long long)end);
    for (uint32_t i = 0; i < expect; ++i) {
      if (width == 4) { uint32_t v; memcpy(&v, out.p + 4 * (size_t)i, 4); printf(" %u", v); }
      else { uint64_t v; memcpy(&v, out.p + 8 * (size_t)i, 8); printf(" %llu", (unsigned long long)v); }
    }
    printf("\n");
  }
  return 0;
}

// ---- one page header, as the walk reads it
static int page_header(const char* hex, bool set2) {
  const size_t n = strlen(hex) / 2;
  Heap in(n);
  for (size_t i = 0; i < n; ++i) { unsigned b = 0; if (sscanf(hex + 2 * i, "%2x", &b) != 1) return 2; in.p[i] = (uint8_t)b; }
  try {
    const PageHeader h = read_page_header(in.p, in.n, set2);
    printf("%d %lld %lld %d %llu\n", h.type, (long long)h.num_values, (long long)h.encoding, (int)h.has_v2, (unsigned long long)h.header_bytes);
  } catch (const PqNeedsHost& e) { printf("NEEDS_HOST %d\n", e.reason); }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7 && !strcmp(argv[1], "decode")) return decode3(argv[2], argv[3], argv[4], atoi(argv[5]), atoi(argv[6]));
  if (argc == 3 && !strcmp(argv[1], "delta")) return delta_streams(argv[2]);
  if (argc == 4 && !strcmp(argv[1], "header")) return page_header(argv[2], atoi(argv[3]) != 0);
  if (argc == 5 || argc == 6) return other_programs::main(argc, argv);   // (the other two files' calls still answer as they did)
  fprintf(stderr, "usage: decode FILE TYPES PROJ LEVEL ENCODINGS | delta FILE\n");
  return 2;
}
