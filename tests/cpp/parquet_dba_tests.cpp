// parquet_dba_tests.cpp — the DELTA_BYTE_ARRAY switch of the device Parquet decoder without a device (tests/test_parquet_dba_cpu.py
// builds and runs this, plainly and under the address and undefined-behaviour sanitizers; nothing of it is loaded into Python).
// It contains the page walk with the switch (qurious_amd/csrc/parquet_meta.hpp) and the code the kernels share with the host
// (csrc/device/qhip_delta.inc, qhip_dba.inc), driven by loops that stand for the 64 lanes of k_pq_delta_dba, k_pq_dba_copy and
// k_pq_dba_fill. Every stream is decoded from a heap block of exactly its size, every column's data into one of exactly its bytes.
//
//   decode FILE TYPES PROJ LEVEL ENCODINGS DBA   as parquet_encodings_tests' decode, with the switch; a Utf8 value is printed
//                                               from the column's data, where the fill has put it together
//   dba FILE      FILE: u32 count, then per stream u32 bytes, u32 width (0: BYTE_ARRAY, 1..16), u32 expected count, the bytes.
//                 Per stream "OK hex hex .." (a value of no bytes is "-") or "REASON r"
//
// The other passes are the older files' own: they are included as they are, in a namespace of their own, under the rule that
// parquet_encodings_tests.cpp states (every header they include is included here first). dba_walks, copy_rows and fill_rows
// below are the kernels' bodies (kernels_parquet.hip: pq_delta_body<true>, k_pq_dba_copy, k_pq_dba_fill) written out again with
// loops for the lanes; only the QH_PQ_HD functions they call are one text for both compilers. What keeps the copies and the
// kernels together is the GPU suite: tests/test_gpu_parquet_dba.py decodes the same files and the same raw streams on the
// device and compares with what these loops answered. A change to a kernel's body is made here too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "parquet_meta.hpp"

namespace older_programs {
#include "parquet_encodings_tests.cpp"
}
using namespace older_programs;
using namespace older_programs::other_programs;
using namespace qhip_pq;

// ---- pq_delta_body<true>, one stream s[0 .. size) of `count` expected values whose bytes begin at `src` in the buffer: both
// walks, ent[0 .. count) as the kernel leaves them. *end: where the suffix bytes begin in s.
static uint32_t dba_walks(const uint8_t* s0, uint64_t size, uint64_t count, uint32_t flba, qh_pq_ent* ent, uint64_t src, uint64_t* end) {
  uint32_t reason = QH_PQ_OK;
  uint64_t begin = 0, pos = 0, sum = 0;
  for (uint32_t walk = 0; walk < 2 && !reason; ++walk) {
    const bool pre = walk == 0;
    begin += pos;
    const uint8_t* s = s0 + begin;
    const uint64_t ssize = size - begin;
    qh_dl_head h;
    memset(&h, 0, sizeof h);
    reason = (uint32_t)qh_dl_header(s, ssize, &h);
    if (!reason && (uint64_t)h.total != count) reason = QH_PQ_R_DELTA_COUNT;
    uint64_t carry = 0, produced = 0;
    uint32_t prev_len = 0;
    pos = 0; sum = 0;
    if (!reason) {
      pos = h.end;
      if (count) {
        carry = h.first; produced = 1;
        if (pre) {
          reason = (uint32_t)qh_dba_check_prefix((uint32_t)carry, true);
          if (!reason) ent[0].pad = 0;
        } else {
          reason = (uint32_t)qh_dba_check_value(0, (uint32_t)carry, 0, flba);
          if (!reason) { ent[0].pos = 0; ent[0].len = (uint32_t)carry; ent[0].pad = 0; }
          sum = (uint32_t)carry; prev_len = (uint32_t)carry;
        }
      }
    }
    while (!reason && produced < count) {
      pq_u64 min_delta = 0, wat = 0, at = 0;
      reason = (uint32_t)qh_dl_block(s, ssize, pos, h.mpb, &min_delta, &wat, &at);
      if (reason) break;
      const uint64_t left = count - produced, in_block = left < (uint64_t)h.block ? left : (uint64_t)h.block;
      const uint64_t mbytes = h.vpm >> 3;
      uint32_t cur_m = 0, cur_w = s[wat];
      reason = (uint32_t)qh_dl_miniblock(cur_w, 32, h.vpm, ssize - at);
      for (uint64_t k0 = 0; !reason && k0 < in_block; k0 += 64) {
        const uint64_t last = k0 + 63 < in_block ? k0 + 63 : in_block - 1;
        const uint32_t m_lo = (uint32_t)(k0 / h.vpm), m_hi = (uint32_t)(last / h.vpm);
        if (m_lo != cur_m) {
          at += mbytes * cur_w; cur_m = m_lo; cur_w = s[wat + cur_m];
          reason = (uint32_t)qh_dl_miniblock(cur_w, 32, h.vpm, ssize - at);
          if (reason) break;
        }
        uint64_t next_at = 0;
        uint32_t next_w = 0;
        if (m_hi != m_lo) {
          next_at = at + mbytes * cur_w; next_w = s[wat + m_hi];
          reason = (uint32_t)qh_dl_miniblock(next_w, 32, h.vpm, ssize - next_at);
          if (reason) break;
        }
        uint64_t val[64];
        bool active[64];
        uint64_t run = carry;
        for (int lane = 0; lane < 64; ++lane) {
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
        if (pre) {
          for (int lane = 0; lane < 64 && !reason; ++lane) if (active[lane]) reason = (uint32_t)qh_dba_check_prefix((uint32_t)val[lane], false);
          if (reason) break;
          for (int lane = 0; lane < 64; ++lane) if (active[lane]) ent[produced + k0 + (uint64_t)lane].pad = (uint32_t)val[lane];
        } else {
          uint32_t full[64] = {0}, pfx[64] = {0};
          for (int lane = 0; lane < 64; ++lane) {
            if (active[lane]) pfx[lane] = ent[produced + k0 + (uint64_t)lane].pad;
            full[lane] = pfx[lane] + (uint32_t)val[lane];
          }
          for (int lane = 0; lane < 64 && !reason; ++lane)   // (the lowest lane's reason counts)
            if (active[lane]) reason = (uint32_t)qh_dba_check_value(pfx[lane], (uint32_t)val[lane], lane ? full[lane - 1] : prev_len, flba);
          if (reason) break;
          prev_len = full[last - k0];
          for (int lane = 0; lane < 64; ++lane) {
            if (!active[lane]) continue;
            qh_pq_ent& e = ent[produced + k0 + (uint64_t)lane];
            e.pos = sum; e.len = full[lane]; e.pad = pfx[lane];
            sum += (uint32_t)val[lane];
          }
        }
        if (m_hi != m_lo) { at = next_at; cur_w = next_w; cur_m = m_hi; }
      }
      if (reason) break;
      pos = at + mbytes * cur_w;
      produced += in_block;
    }
    if (!reason && !pre) {
      reason = (uint32_t)qh_dba_check_total(sum, ssize - pos);
      if (!reason) for (uint64_t i = 0; i < count; ++i) ent[i].pos += src + begin + pos;
    }
  }
  *end = begin + pos;
  return reason;
}

// ---- k_pq_dba_fill: the rows or values [r_begin, r_end), 64 per step. off / prefix / valid answer for one of them; data is the
// block the prefixes are filled into (and the sources read from).
template <class Off, class Prefix, class Valid>
static void fill_rows(uint8_t* data, uint64_t r_begin, uint64_t r_end, Off off, Prefix prefix, Valid is_valid) {
  uint64_t before = 0;
  bool have = false;
  for (uint64_t t0 = r_begin & ~(uint64_t)63; t0 < r_end; t0 += 64) {
    bool valid[64];
    uint32_t p[64];
    uint64_t o[64], there = 0;
    bool longp = false;
    for (int l = 0; l < 64; ++l) {
      const uint64_t r = t0 + (uint64_t)l;
      valid[l] = r >= r_begin && r < r_end && is_valid(r);
      p[l] = valid[l] ? prefix(r) : 0; o[l] = valid[l] ? off(r) : 0;
      if (valid[l]) there |= 1ULL << l;
      if (valid[l] && p[l] > QH_DBA_STEP_PREFIX) longp = true;
    }
    if (!there) continue;
    if (longp) {
      for (int l = 0; l < 64; ++l) {
        if (!valid[l]) continue;
        if (have) for (uint32_t b = 0; b < p[l]; ++b) data[o[l] + b] = data[before + b];
        before = o[l]; have = true;
      }
    } else {
      for (uint32_t j = 0;; ++j) {
        uint64_t need = 0, m = 0;
        for (int l = 0; l < 64; ++l) { if (valid[l] && p[l] > j) need |= 1ULL << l; if (valid[l] && p[l] <= j) m |= 1ULL << l; }
        if (!need) break;
        uint8_t got[64];   // (every lane loads, then every lane stores: the step reads nothing that it writes)
        bool store[64];
        for (int l = 0; l < 64; ++l) {
          const int sl = qh_dba_source_lane(m, l);
          store[l] = valid[l] && p[l] > j && (sl >= 0 || have);
          if (store[l]) got[l] = data[(sl >= 0 ? o[sl] : before) + j];
        }
        for (int l = 0; l < 64; ++l) if (store[l]) data[o[l] + j] = got[l];
      }
      before = o[63 - __builtin_clzll(there)]; have = true;
    }
  }
}

// ---- k_pq_dba_copy: row k's suffix to data[off[k] + prefix[k] ..)
static bool copy_rows(const uint8_t* buf, uint64_t buf_bytes, const pq_u64* strpos, const uint32_t* off, const uint32_t* prefix, uint64_t nrows, uint8_t* data) {
  for (uint64_t k = 0; k < nrows; ++k) {
    const uint32_t p = prefix ? prefix[k] : 0, whole = off[k + 1] - off[k], len = p < whole ? whole - p : 0;
    if (strpos[k] > buf_bytes || len > buf_bytes - strpos[k]) return false;
    for (uint32_t b = 0; b < len; ++b) data[off[k] + p + b] = buf[strpos[k] + b];
  }
  return true;
}

// ---- a whole file at a format level, an encoding set and the switch
static int decode4(const char* path, const char* type_codes, const char* proj_text, int level, int encodings, int dba) {
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
    plan = plan_file(file.p, file.n, nullptr, types, proj, level, encodings, 1, 0, 0, dba);
  } catch (const PqNeedsHost& e) {
    printf("NEEDS_HOST %d %lld %lld %lld\n", e.reason, (long long)e.row_group, (long long)e.column, (long long)e.page);
    return 0;
  }
  const uint64_t R = plan.num_rows, words = (R + 63) / 64, buf_bytes = plan.buffer_bytes();
  Heap buf((size_t)buf_bytes, 0xAB);
  for (const Range& r : plan.ranges) memcpy(buf.p + r.buf_off, file.p + r.file_off, (size_t)r.bytes);
  FirstError unpack_err;
  for (const qh_pq_unpack& u : plan.unpack) {
    if ((u.dst & 15) || u.dst + u.dst_size > plan.packed_bytes() || u.src + u.src_size > plan.upload_bytes) { fprintf(stderr, "a slot outside the unpack area\n"); return 3; }
    Heap in(u.src_size), out(u.dst_size, 0xAB);
    memcpy(in.p, buf.p + u.src, u.src_size);
    const uint32_t reason = unsnap(in.p, in.n, u.start, out.p, out.n);
    if (reason) unpack_err.report(u.page, QH_PQ_R_SNAPPY_BASE + reason);
    memcpy(buf.p + u.dst, out.p, u.dst_size);
  }
  for (const qh_pq_page& pg : plan.pages)
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
      if (cp.dba) d.prefix = (pq_u32*)heap((size_t)R * 4, 0);
    } else if (cp.boolean) d.values = heap(words * 8, 0);
    else d.values = heap((size_t)R * cp.width, 0xAB);
    d.phys = cp.phys; d.flba = cp.flba; d.width = cp.width; d.narrow = cp.narrow;
  }
  std::vector<qh_pq_state> state(plan.pages.size());
  std::vector<uint64_t> nulls(ncols, 0), utf8(ncols, 0);
  FirstError err;
  for (size_t p = 0; p < plan.pages.size(); ++p)
    if (plan.pages[p].enc != QH_PQ_ENC_DICTPAGE) levels_page2(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err, nulls[plan.pages[p].col]);
  // the delta pass: each stream from a block of exactly its bytes; the slots of the decoded area one behind the other
  uint64_t dslot_end = plan.decoded_base;
  size_t fv = 0;
  if (err.word == ~0ULL)
    for (const qh_pq_dstream& d : plan.delta) {
      const qh_pq_page& pg = plan.pages[d.page];
      const qh_pq_state& st = state[d.page];
      const bool lengths = d.width & QH_PQ_DS_LENGTHS, isdba = d.width & QH_PQ_DS_DBA;
      const uint32_t width = d.width & 0xFF;
      const uint64_t src = pg.pos + st.values_off, size = (uint64_t)pg.size - st.values_off;
      if (isdba) {
        const qh_pq_fill* fj = nullptr;
        if (width) {   // a FIXED_LEN_BYTE_ARRAY page: its values' slot, then its entries' slot
          fj = &plan.fill_values[fv++];
          const uint64_t vbytes = (uint64_t)pg.num_values * width;
          if (fj->page != d.page || fj->out != dslot_end || (fj->out & 15) || fj->first != fj->out + ((vbytes + 15) & ~(uint64_t)15) || d.dst != fj->first ||
              fj->first + (uint64_t)pg.num_values * sizeof(qh_pq_ent) > buf_bytes || pg.dict_pos != fj->out || fj->width != width) { fprintf(stderr, "a slot outside the decoded area\n"); return 3; }
          dslot_end = fj->first + (uint64_t)pg.num_values * sizeof(qh_pq_ent);
        }
        if (!st.nonnull) continue;
        Heap in((size_t)size);
        if (size) memcpy(in.p, buf.p + src, (size_t)size);
        std::unique_ptr<qh_pq_ent[]> ents(new qh_pq_ent[st.nonnull]);   // (exactly the page's entries)
        uint64_t end = 0;
        const uint32_t reason = dba_walks(in.p, size, st.nonnull, width, ents.get(), src, &end);
        if (reason) { err.report(d.page, reason); continue; }
        for (uint32_t i = 0; i < st.nonnull; ++i)
          if (ents[i].pos < src || ents[i].pos + (ents[i].len - ents[i].pad) > src + size) { fprintf(stderr, "a suffix outside its page\n"); return 3; }
        if (!width) { memcpy(cols[pg.col].ent + pg.ent, ents.get(), (size_t)st.nonnull * sizeof(qh_pq_ent)); continue; }
        // k_pq_dba_fill in value space: each value's suffix, then the prefixes, into a block of exactly the dense values
        Heap dense((size_t)st.nonnull * width, 0xAB);
        for (uint32_t i = 0; i < st.nonnull; ++i)
          for (uint32_t b = ents[i].pad; b < ents[i].len; ++b) dense.p[(uint64_t)i * width + b] = buf.p[ents[i].pos + (b - ents[i].pad)];
        fill_rows(dense.p, 0, st.nonnull, [&](uint64_t i) { return i * width; }, [&](uint64_t i) { return ents[i].pad; }, [](uint64_t) { return true; });
        memcpy(buf.p + fj->out, dense.p, dense.n);
        continue;
      }
      const uint64_t slot = (uint64_t)pg.num_values * width;
      if (!lengths) {
        if (d.dst != dslot_end || (d.dst & 15) || d.dst + slot > buf_bytes || pg.dict_pos != d.dst) { fprintf(stderr, "a slot outside the decoded area\n"); return 3; }
        dslot_end = d.dst + ((slot + 15) & ~(uint64_t)15);
      }
      if (!st.nonnull) continue;
      Heap in((size_t)size), out(lengths ? 0 : (size_t)((uint64_t)st.nonnull * width), 0xAB);
      if (size) memcpy(in.p, buf.p + src, (size_t)size);
      std::unique_ptr<qh_pq_ent[]> ents(new qh_pq_ent[lengths ? st.nonnull : 1]);
      uint64_t end = 0;
      const uint32_t reason = delta_stream(in.p, size, st.nonnull, width, lengths, out.p, ents.get(), src, &end);
      if (reason) { err.report(d.page, reason); continue; }
      if (lengths) memcpy(cols[pg.col].ent + pg.ent, ents.get(), (size_t)st.nonnull * sizeof(qh_pq_ent));
      else memcpy(buf.p + d.dst, out.p, out.n);
    }
  if (plan.decoded_bytes && dslot_end != buf_bytes && err.word == ~0ULL) { fprintf(stderr, "the decoded area's size is not its slots'\n"); return 3; }
  if (err.word == ~0ULL)
    for (size_t p = 0; p < plan.pages.size(); ++p)
      if (plan.pages[p].enc != QH_PQ_ENC_DELTA_LEN && plan.pages[p].enc != QH_PQ_ENC_DBA) strings_page(buf.p, plan.pages[p], cols[plan.pages[p].col], state[p], p, err);
  if (err.word == ~0ULL)
    for (size_t p = 0; p < plan.pages.size(); ++p) {
      const qh_pq_page& pg = plan.pages[p];
      if (pg.enc == QH_PQ_ENC_DICTPAGE) continue;
      const qh_pq_col& col = cols[pg.col];
      values_page2(buf.p, pg, col, state[p], p, err, utf8[pg.col]);
      if (pg.enc == QH_PQ_ENC_DBA && col.prefix) {   // (pq_values_body: the prefix length beside length and position)
        uint64_t idx = 0;
        for (uint64_t row = pg.first_row; row < pg.first_row + pg.num_values; ++row)
          if (!col.valid || ((col.valid[row >> 6] >> (row & 63)) & 1)) col.prefix[row] = col.ent[pg.ent + idx++].pad;
      }
    }
  const uint64_t offender = unpack_err.word != ~0ULL ? unpack_err.word : err.word;
  if (offender != ~0ULL) {
    const PageWhere& w = plan.where[(size_t)(offender >> 8)];
    printf("NEEDS_HOST %d %lld %lld %lld\n", (int)(offender & 0xFF), (long long)w.row_group, (long long)w.column, (long long)w.page);
    return 0;
  }
  // behind the wait: lengths into offsets, the bytes into a block of exactly their sum, the prefixes of the DELTA_BYTE_ARRAY pages
  std::vector<uint8_t*> data(ncols, nullptr);
  for (size_t k = 0; k < ncols; ++k) {
    if (!plan.cols[k].utf8) continue;
    uint32_t* off = (uint32_t*)cols[k].values;
    uint64_t total = 0;
    for (uint64_t r = 0; r < R; ++r) { const uint32_t len = off[r]; off[r] = (uint32_t)total; total += len; }
    if (total != utf8[k] || total > 0x7fffffffULL) { fprintf(stderr, "a column's bytes are not its lengths'\n"); return 3; }
    off[R] = (uint32_t)total;
    data[k] = heap((size_t)total, 0xAB);
    if (!copy_rows(buf.p, buf_bytes, cols[k].strpos, off, cols[k].prefix, R, data[k])) { fprintf(stderr, "a string outside the buffer\n"); return 3; }
  }
  for (const qh_pq_fill& fj : plan.fill_rows) {
    const qh_pq_col& col = cols[fj.col];
    const uint32_t* off = (const uint32_t*)col.values;
    const pq_u64* vw = nulls[fj.col] ? col.valid : nullptr;   // (a column without NULLs has dropped its validity by then)
    fill_rows(data[fj.col], fj.first, fj.first + fj.n, [&](uint64_t r) { return (uint64_t)off[r]; }, [&](uint64_t r) { return col.prefix[r]; },
              [&](uint64_t r) { return !vw || ((vw[r >> 6] >> (r & 63)) & 1); });
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
          const uint32_t* off = (const uint32_t*)d.values;
          for (uint32_t b = off[r]; b < off[r + 1]; ++b) printf("%02x", data[k][b]);
          break;
        }
        default: printf("%lld", (long long)((int64_t*)d.values)[r]); break;   // Int64, Timestamp
      }
    }
    putchar('\n');
  }
  return 0;
}

// ---- raw streams, as qhip_parquet_dba_decode takes them
static int dba_streams(const char* path) {
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
    if (raw.size() - at < n || width > 16) return 2;
    Heap in(n);
    if (n) memcpy(in.p, raw.data() + at, n);
    at += n;
    std::unique_ptr<qh_pq_ent[]> ents(new qh_pq_ent[expect ? expect : 1]);
    uint64_t end = 0;
    const uint32_t reason = dba_walks(in.p, in.n, expect, width, ents.get(), 0, &end);
    if (reason) { printf("REASON %u\n", reason); continue; }
    std::vector<pq_u64> strpos(expect);
    std::vector<uint32_t> off(expect + 1, 0), prefix(expect);
    uint64_t total = 0;
    for (uint32_t i = 0; i < expect; ++i) { strpos[i] = ents[i].pos; prefix[i] = ents[i].pad; off[i] = (uint32_t)total; total += ents[i].len; }
    off[expect] = (uint32_t)total;
    Heap data((size_t)total, 0xAB);
    if (!copy_rows(in.p, in.n, strpos.data(), off.data(), prefix.data(), expect, data.p)) { fprintf(stderr, "a suffix outside its stream\n"); return 3; }
    fill_rows(data.p, 0, expect, [&](uint64_t r) { return (uint64_t)off[r]; }, [&](uint64_t r) { return prefix[r]; }, [](uint64_t) { return true; });
    printf("OK");
    for (uint32_t i = 0; i < expect; ++i) {
      putchar(' ');
      if (off[i] == off[i + 1]) putchar('-');
      for (uint32_t b = off[i]; b < off[i + 1]; ++b) printf("%02x", data.p[b]);
    }
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 8 && !strcmp(argv[1], "decode")) return decode4(argv[2], argv[3], argv[4], atoi(argv[5]), atoi(argv[6]), atoi(argv[7]));
  if (argc == 3 && !strcmp(argv[1], "dba")) return dba_streams(argv[2]);
  return older_programs::main(argc, argv);   // (the older files' calls still answer as they did)
}
