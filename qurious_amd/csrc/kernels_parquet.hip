// kernels_parquet.hip — Parquet pages in HBM -> typed Arrow columns (gfx950, wave64), compiled ahead of time. The host side is
// parquet.cpp (qhip_table_from_parquet); the per-run and per-value code is device/qhip_parquet.inc, shared with the CPU tests.
// Replaces the reference's host Parquet reader (datasource/file/parquet.rs) for files inside the coverage of DESIGN §3.9.
//
// The unit of parallelism is the page: one wavefront each. Serial work happens per run header and per BYTE_ARRAY length prefix
// only; the values of a run are spread over the lanes.
//   k_pq_unsnap   format level 2 only: a Snappy page of the uploaded chunks -> its uncompressed bytes in the unpack area
//   k_pq_levels   RLE / bit-packed definition levels -> validity words, the page's non-NULL count, the column's NULL count
//   k_pq_strings  the length chain of a Utf8 dictionary page or PLAIN data page, staged through LDS -> (length, position)
//   k_pq_values   64 rows per step: rank among the non-NULL rows -> value index -> run cursor -> dictionary gather or PLAIN read
//
// Nothing here trusts the file: every run, index and length is checked against its stream, dictionary or page before it is
// followed, and the first offender (page << 8 | reason) makes the whole call answer "needs host".
#include <hip/hip_runtime.h>

#include "device/qhip_status.h"
#include "device/qhip_device.hpp"
#include "kernels_parquet.hpp"
#include "device/qhip_snappy.inc"

namespace qhip {

typedef u32 pq_v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void pq_report(u64* err, u64 page, u32 reason) {
  const u64 mine = (page << 8) | reason;
  if (mine < __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(err, mine);
}

// One wavefront per page. Every lane parses the run header (the same bytes: one broadcast load), then lane l builds validity
// word first + l, first + l + 64, ... of the run. A word the run covers whole belongs to nobody else and is stored; a word
// shared with the neighbouring run or page is OR-ed into the zeroed bitmap.
__global__ __launch_bounds__(QH_BLOCK) void k_pq_levels(const u8* __restrict__ buf, const qh_pq_page* __restrict__ pages, u32 npages,
                                                        const qh_pq_col* __restrict__ cols, qh_pq_state* state, u64* err, u64* null_counts) {
  const u32 page = (blockIdx.x * QH_BLOCK + threadIdx.x) >> 6;
  if (page >= npages) return;
  const qh_pq_page pg = pages[page];
  if (pg.enc == QH_PQ_ENC_DICTPAGE) return;
  const qh_pq_col col = cols[pg.col];
  const int lane = qh_lane();
  const u64 n = pg.num_values;
  if (!col.valid) {   // a required column has no levels: the values begin the page
    if (lane == 0) { state[page].nonnull = (u32)n; state[page].values_off = 0; }
    return;
  }
  const u8* p = buf + pg.pos;
  u32 reason = QH_PQ_OK, len = 0;
  if (pg.size < 4) reason = QH_PQ_R_LEVELS_LENGTH;
  else {
    len = qh_pq_le32(p);
    if (len > pg.size - 4) reason = QH_PQ_R_LEVELS_LENGTH;
  }
  const u8* s = p + 4;
  u64 cpos = 0, row = 0;
  u32 nonnull = 0;
  qh_pq_run run;
  qh_pq_run_init(&run);
  while (!reason && row < n) {
    reason = (u32)qh_pq_next_run(s, len, &cpos, 1, &run);
    if (reason) break;
    u64 take = run.count;
    const u64 left = n - row;
    if (run.packed) {
      if (take >= left + 8) reason = QH_PQ_R_RUN_COUNT;   // (the last group of 8 may be padded, no more)
      else if (take > left) take = left;
    } else if (take > left) reason = QH_PQ_R_RUN_COUNT;
    else if (run.value > 1) reason = QH_PQ_R_LEVEL_VALUE;
    if (reason) break;
    const u64 g0 = pg.first_row + row;
    if (run.packed || run.value) {
      const u64 wlast = (g0 + take - 1) >> 6;
      for (u64 w = (g0 >> 6) + (u64)lane; w <= wlast; w += 64) {
        const u64 bits = qh_pq_level_word(s, &run, g0, take, w);
        if (w * 64 >= g0 && w * 64 + 64 <= g0 + take) col.valid[w] = bits;
        else if (bits) atomicOr((unsigned long long*)&col.valid[w], bits);
        nonnull += (u32)__builtin_popcountll(bits);
      }
    }
    row += take;
  }
  const u32 total = (u32)qh_wave_sum_u64((u64)nonnull);
  if (lane == 0) {
    state[page].nonnull = total;
    state[page].values_off = 4 + len;
    if (reason) pq_report(err, page, reason);
    else if (n > total) atomicAdd(&null_counts[pg.col], n - (u64)total);   // (one atomic per page)
  }
}

// One wavefront (a workgroup of its own, so that the barrier is the wavefront's) walks one length chain. The chain's bytes are
// staged into LDS 1 KB at a time with aligned 16-byte loads; the step itself — read 4 bytes, check, follow — is the same in
// every lane, and lane k & 63 keeps entry k, so that 64 entries leave in one coalesced store. A length is checked against the
// region's end before it is followed; a long string simply moves the tile.
constexpr u32 kPqTile = 1024;
__global__ __launch_bounds__(64) void k_pq_strings(const u8* __restrict__ buf, u64 buf_bytes, const qh_pq_page* __restrict__ pages, u32 npages,
                                                   const qh_pq_col* __restrict__ cols, const qh_pq_state* __restrict__ state, u64* err) {
  __shared__ __attribute__((aligned(16))) u8 tile[kPqTile];
  const u32 page = blockIdx.x;
  if (page >= npages) return;
  const qh_pq_page pg = pages[page];
  const qh_pq_col col = cols[pg.col];
  if (col.phys != QH_PQ_P_BYTES || pg.enc == QH_PQ_ENC_DICT) return;
  if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ULL) return;   // (the level pass found an offender: its state is void)
  const int lane = qh_lane();
  u64 base = pg.pos, size = pg.size, count = pg.num_values;
  if (pg.enc == QH_PQ_ENC_PLAIN) {
    const qh_pq_state st = state[page];
    base += st.values_off; size -= st.values_off; count = st.nonnull;
  }
  qh_pq_ent* ent = col.ent + pg.ent;
  u64 q = 0, tbase = ~0ULL, mypos = 0;
  u32 mylen = 0, reason = QH_PQ_OK;
  for (u64 k = 0; k < count; ++k) {
    if (!qh_pq_chain_has_prefix(q, size)) { reason = QH_PQ_R_BYTE_ARRAY; break; }
    const u64 at = base + q;
    if (tbase == ~0ULL || at < tbase || at + 4 > tbase + kPqTile) {
      __syncthreads();
      tbase = at & ~(u64)15;
      // (a vector that begins inside the buffer may reach 15 bytes past it: the allocation's slack)
      const u64 o = (u64)lane * 16;
      if (tbase + o < buf_bytes) *(pq_v4u*)(tile + o) = *(const pq_v4u*)(buf + tbase + o);
      __syncthreads();
    }
    const u32 len = qh_pq_le32(tile + (at - tbase));
    if (!qh_pq_chain_fits(q, size, len)) { reason = QH_PQ_R_BYTE_ARRAY; break; }
    if ((int)(k & 63) == lane) { mylen = len; mypos = at + 4; }
    q += 4 + (u64)len;
    if ((k & 63) == 63 || k + 1 == count) {
      const u64 mine = (k & ~(u64)63) + (u64)lane;
      if (mine <= k) { qh_pq_ent e; e.pos = mypos; e.len = mylen; e.pad = 0; ent[mine] = e; }
    }
  }
  if (reason && lane == 0) pq_report(err, page, reason);
}

// Format level 2: one wavefront (a workgroup of its own) unpacks one Snappy page from the uploaded chunks into its slot of the
// unpack area, both in `buf`. The walk over the elements is serial and wave-uniform — input position, output position and the
// element are the same in every lane: the tag and its length or offset bytes are read from a 1 KB tile of the input staged in
// LDS as k_pq_strings stages its chains, and a literal that lies inside the tile is taken from there. The bytes of an element
// are spread over the lanes: a literal in strides of 64, four loads in flight per lane; a copy (at most 64 bytes) in one step,
// lane l taking the byte qh_snap_copy_src names, which earlier elements stored — never this one.
// Those bytes were stored by other lanes of this wavefront and are read back from global memory. That rests on one rule: a
// wavefront's vector memory instructions are issued in program order to the one L1 of its CU, write-through, so a load behind a
// store of the same wavefront returns the stored bytes whichever lane stored them (LLVM's AMDGPU memory model for gfx90a / gfx942:
// no action is needed for coherence between the lanes of a wavefront). The wavefront-scope fence per element keeps the compiler
// to the same order and costs no instruction. So `buf` is neither const nor __restrict__ here.
// Checks come before every access (qh_snap_check); a refused page leaves its slot half written, which the later passes read as
// they read any page: untrusted, inside the slot. status (the raw-stream entry): 0 or the error per stream, where not null.
__global__ __launch_bounds__(64) void k_pq_unsnap(u8* buf, u64 buf_bytes, const qh_pq_unpack* __restrict__ tab, u32 n, u64* err, u32* status) {
  __shared__ __attribute__((aligned(16))) u8 tile[kPqTile];
  const u32 k = blockIdx.x;
  if (k >= n) return;
  const qh_pq_unpack u = tab[k];
  const u32 lane = (u32)qh_lane();
  const u8* src = buf + u.src;
  u8* dst = buf + u.dst;
  const u64 n_in = u.src_size, n_out = u.dst_size;
  u64 ip = u.start, op = 0, tbase = ~0ULL;
  u32 reason = QH_SNAP_OK;
  while (ip < n_in) {
    if (op == n_out) { reason = QH_SNAP_E_INPUT; break; }   // (input left behind a full page)
    const u64 at = u.src + ip;
    if (tbase == ~0ULL || at < tbase || at + 5 > tbase + kPqTile) {
      __syncthreads();
      tbase = at & ~(u64)15;
      // (a vector that begins inside the buffer may reach 15 bytes past it: the allocation's slack)
      const u64 o = (u64)lane * 16;
      if (tbase + o < buf_bytes) *(pq_v4u*)(tile + o) = *(const pq_v4u*)(buf + tbase + o);
      __syncthreads();
    }
    qh_snap_elem e;
    reason = (u32)qh_snap_element(tile + (at - tbase), n_in - ip, &e);
    if (reason) break;
    ip += e.header;
    reason = (u32)qh_snap_check(&e, n_in - ip, op, n_out);
    if (reason) break;
    if (e.kind == QH_SNAP_LITERAL) {
      const u64 from = u.src + ip;
      if (from + e.len <= tbase + kPqTile) {
        for (u64 i = lane; i < e.len; i += 64) dst[op + i] = tile[from - tbase + i];
      } else {
        const u8* s = src + ip;
        u8* d = dst + op;
        for (u64 i = lane; i < e.len; i += 256) {
          const bool h1 = i + 64 < e.len, h2 = i + 128 < e.len, h3 = i + 192 < e.len;
          const u8 b0 = s[i], b1 = h1 ? s[i + 64] : (u8)0, b2 = h2 ? s[i + 128] : (u8)0, b3 = h3 ? s[i + 192] : (u8)0;
          d[i] = b0;
          if (h1) d[i + 64] = b1;
          if (h2) d[i + 128] = b2;
          if (h3) d[i + 192] = b3;
        }
      }
      ip += e.len;
    } else if ((u64)lane < e.len) {
      dst[op + lane] = dst[qh_snap_copy_src(op, e.offset, lane)];
    }
    op += e.len;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  if (!reason && op != n_out) reason = QH_SNAP_E_INPUT;   // (the input ended with output missing)
  if (lane == 0) {
    if (status) status[k] = reason;
    if (reason && err) pq_report(err, u.page, QH_PQ_R_SNAPPY_BASE + reason);
  }
}

// One wavefront per data page, 64 rows per step, the steps aligned to the column's 64-row words: a lane's row is word * 64 +
// lane, its validity bit is bit `lane` of one word, and a Boolean column's word is one ballot. The lane's value index is the
// page's running non-NULL count plus its rank in the step. Dictionary pages: a run cursor moves forward under wave-uniform
// control until the step's highest index is inside or behind it; a lane whose index lies in the current run takes the RLE
// value or extracts its bits.
__global__ __launch_bounds__(QH_BLOCK) void k_pq_values(const u8* __restrict__ buf, const qh_pq_page* __restrict__ pages, u32 npages,
                                                        const qh_pq_col* __restrict__ cols, const qh_pq_state* __restrict__ state, u64* err, u64* utf8_bytes) {
  const u32 page = (blockIdx.x * QH_BLOCK + threadIdx.x) >> 6;
  if (page >= npages) return;
  const qh_pq_page pg = pages[page];
  if (pg.enc == QH_PQ_ENC_DICTPAGE) return;
  if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ULL) return;   // (an earlier pass found an offender)
  const qh_pq_col col = cols[pg.col];
  const qh_pq_state st = state[page];
  const int lane = qh_lane();
  const u64 nn = st.nonnull;
  const u8* v = buf + pg.pos + st.values_off;
  const u64 vsize = (u64)pg.size - st.values_off;
  const u32 pw = qh_pq_phys_bytes(col.phys, col.flba);
  const bool dict = pg.enc == QH_PQ_ENC_DICT;
  u32 reason = QH_PQ_OK, w = 0;
  const u8* s = v;
  u64 slen = 0;
  if (dict) {
    if (nn) {
      if (vsize < 1) reason = QH_PQ_R_VALUES_SHORT;
      else {
        w = v[0]; s = v + 1; slen = vsize - 1;
        if (w > 32) reason = QH_PQ_R_BIT_WIDTH;
      }
    }
  } else if (col.phys == QH_PQ_P_BOOL) {
    if ((nn + 7) / 8 > vsize) reason = QH_PQ_R_VALUES_SHORT;
  } else if (col.phys != QH_PQ_P_BYTES) {
    if (nn * pw > vsize) reason = QH_PQ_R_VALUES_SHORT;
  }
  qh_pq_run run;
  qh_pq_run_init(&run);
  u64 cpos = 0, base = 0, mybytes = 0;
  const u64 r_begin = pg.first_row, r_end = r_begin + pg.num_values;
  for (u64 t0 = r_begin & ~(u64)63; !reason && t0 < r_end; t0 += 64) {
    const u64 row = t0 + (u64)lane;
    const bool in = row >= r_begin && row < r_end;
    bool valid = in;
    if (in && col.valid) valid = (col.valid[t0 >> 6] >> lane) & 1ULL;
    const u64 m = qh_ballot(valid);
    const u64 idx = base + (u64)__builtin_popcountll(m & ((1ULL << lane) - 1ULL));
    base += (u64)__builtin_popcountll(m);
    if (base > nn) { reason = QH_PQ_R_VALUES_SHORT; break; }   // (cannot happen: the bitmap is what the level pass counted)
    u32 index = 0;
    if (dict) {
      bool served = !valid;
      for (;;) {
        if (!served && idx >= run.start && idx < run.start + run.count) { index = qh_pq_run_value(s, &run, idx, w); served = true; }
        if (run.start + run.count >= base) break;
        reason = (u32)qh_pq_next_run(s, slen, &cpos, w, &run);
        if (reason) break;
      }
      if (reason) break;
      if (qh_ballot(valid && index >= pg.dict_n)) { reason = QH_PQ_R_DICT_INDEX; break; }
    }
    u64 lo = 0, hi = 0, spos = 0;
    u32 slen_row = 0;
    bool bit = false;
    if (valid) {
      if (col.phys == QH_PQ_P_BYTES) {
        const qh_pq_ent e = col.ent[pg.ent + (dict ? (u64)index : idx)];
        spos = e.pos; slen_row = e.len;
      } else if (col.phys == QH_PQ_P_BOOL) {
        bit = (v[idx >> 3] >> (idx & 7)) & 1;
      } else {
        const u8* src = dict ? buf + pg.dict_pos + (u64)index * pw : v + idx * pw;
        qh_pq_read_value(src, col.phys, col.flba, &lo, &hi);
      }
    }
    if (qh_ballot(valid && col.narrow && !qh_pq_in_range(lo, col.width, col.narrow))) { reason = QH_PQ_R_RANGE; break; }
    if (col.phys == QH_PQ_P_BYTES) {
      if (in) { ((u32*)col.values)[row] = slen_row; col.strpos[row] = spos; mybytes += slen_row; }
    } else if (col.phys == QH_PQ_P_BOOL) {
      const u64 word = qh_ballot(valid && bit);
      if (lane == 0 && word) atomicOr((unsigned long long*)&((u64*)col.values)[t0 >> 6], word);   // (the first and last word are shared with the neighbouring pages)
    } else if (in) {
      qh_pq_store(col.values, row, col.width, lo, hi);   // (a NULL row's slot is zero)
    }
  }
  const u64 bytes = qh_wave_sum_u64(mybytes);
  if (lane == 0) {
    if (reason) pq_report(err, page, reason);
    else if (bytes) atomicAdd(&utf8_bytes[pg.col], bytes);
  }
}

// ---------------------------------------------------------------- launchers
void launch_pq_levels(const uint8_t* buf, const qh_pq_page* pages, uint32_t npages, const qh_pq_col* cols, qh_pq_state* state, uint64_t* err, uint64_t* null_counts,
                      hipStream_t s) {
  if (!npages) return;
  const unsigned g = (unsigned)(((uint64_t)npages * 64 + QH_BLOCK - 1) / QH_BLOCK);
  hipLaunchKernelGGL(k_pq_levels, dim3(g), dim3(QH_BLOCK), 0, s, (const u8*)buf, pages, (u32)npages, cols, state, (u64*)err, (u64*)null_counts);
}
void launch_pq_unsnap(uint8_t* buf, uint64_t buf_bytes, const qh_pq_unpack* tab, uint32_t n, uint64_t* err, uint32_t* status, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_pq_unsnap, dim3(n), dim3(64), 0, s, (u8*)buf, (u64)buf_bytes, tab, (u32)n, (u64*)err, (u32*)status);
}
void launch_pq_strings(const uint8_t* buf, uint64_t buf_bytes, const qh_pq_page* pages, uint32_t npages, const qh_pq_col* cols, const qh_pq_state* state, uint64_t* err,
                       hipStream_t s) {
  if (!npages) return;
  hipLaunchKernelGGL(k_pq_strings, dim3(npages), dim3(64), 0, s, (const u8*)buf, (u64)buf_bytes, pages, (u32)npages, cols, state, (u64*)err);
}
void launch_pq_values(const uint8_t* buf, const qh_pq_page* pages, uint32_t npages, const qh_pq_col* cols, const qh_pq_state* state, uint64_t* err, uint64_t* utf8_bytes,
                      hipStream_t s) {
  if (!npages) return;
  const unsigned g = (unsigned)(((uint64_t)npages * 64 + QH_BLOCK - 1) / QH_BLOCK);
  hipLaunchKernelGGL(k_pq_values, dim3(g), dim3(QH_BLOCK), 0, s, (const u8*)buf, pages, (u32)npages, cols, state, (u64*)err, (u64*)utf8_bytes);
}

}  // namespace qhip
