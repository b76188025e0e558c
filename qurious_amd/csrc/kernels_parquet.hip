// kernels_parquet.hip — Parquet pages in HBM -> typed Arrow columns (gfx950, wave64), compiled ahead of time. The host side is
// parquet.cpp (qhip_table_from_parquet); the per-run and per-value code is device/qhip_parquet.inc, shared with the CPU tests.
// Replaces the reference's host Parquet reader (datasource/file/parquet.rs) for files inside the coverage of DESIGN §3.9.
//
// The unit of parallelism is the page: one wavefront each. Serial work happens per run header and per BYTE_ARRAY length prefix
// only; the values of a run are spread over the lanes.
//   k_pq_unsnap   format level 2 only: a Snappy page of the uploaded chunks -> its uncompressed bytes in the unpack area
//   k_pq_unzstd   codec set 2 only: a ZSTD page of the uploaded chunks -> its uncompressed bytes in the unpack area
//   k_pq_ungzip   the gzip switch only: a GZIP page of the uploaded chunks -> its uncompressed bytes in the unpack area
//   k_pq_unlz4    the lz4 switch only: an LZ4 block of the uploaded chunks -> its uncompressed bytes in the unpack area
//   k_pq_levels   RLE / bit-packed definition levels -> validity words, the page's non-NULL count, the column's NULL count
//   k_pq_strings  the length chain of a Utf8 dictionary page or PLAIN data page, staged through LDS -> (length, position)
//   k_pq_delta    encoding set 2 only: a DELTA_BINARY_PACKED stream -> dense values in the decoded area, or a Utf8 page's entries
//   k_pq_values   64 rows per step: rank among the non-NULL rows -> value index -> run cursor -> dictionary gather or PLAIN read
//   k_pq_values_ext  encoding set 2 only: the same body for RLE Boolean, BYTE_STREAM_SPLIT and DELTA_* pages
//   k_pq_delta_dba  the DELTA_BYTE_ARRAY switch only: k_pq_delta's body for a page's prefix and suffix lengths -> its entries
//   k_pq_dba_copy / k_pq_dba_fill  the DELTA_BYTE_ARRAY switch only: suffixes into place, then the prefixes, 64 rows per step
//
// Nothing here trusts the file: every run, index and length is checked against its stream, dictionary or page before it is
// followed, and the first offender (page << 8 | reason) makes the whole call answer "needs host".
#include <hip/hip_runtime.h>

#include "device/qhip_status.h"
#include "device/qhip_device.hpp"
#include "kernels_parquet.hpp"
#include "device/qhip_snappy.inc"
#include "device/qhip_zstd.inc"
#include "device/qhip_inflate.inc"
#include "device/qhip_lz4.inc"

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
  const bool v2 = pg.flags & QH_PQ_F_V2;   // (encoding set 2: the stream lies at lev_pos, lev_size bytes the host has checked, no prefix)
  u32 reason = QH_PQ_OK, len = 0;
  if (v2) len = pg.lev_size;
  else if (pg.size < 4) reason = QH_PQ_R_LEVELS_LENGTH;
  else {
    len = qh_pq_le32(p);
    if (len > pg.size - 4) reason = QH_PQ_R_LEVELS_LENGTH;
  }
  const u8* s = v2 ? buf + pg.lev_pos : p + 4;
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
    state[page].values_off = v2 ? 0 : 4 + len;
    if (!reason && v2 && n - (u64)total != (u64)pg.num_nulls) reason = QH_PQ_R_V2_NULLS;
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
  if (col.phys != QH_PQ_P_BYTES || pg.enc == QH_PQ_ENC_DICT || pg.enc == QH_PQ_ENC_DELTA_LEN || pg.enc == QH_PQ_ENC_DBA) return;   // (k_pq_delta wrote a DELTA_LENGTH or DELTA_BYTE_ARRAY page's entries)
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

// Codec set 2: one wavefront (a workgroup of its own) unpacks one ZSTD page, a whole Zstandard frame, from the uploaded chunks
// into its slot of the unpack area, both in `buf`. The decoder is device/qhip_zstd.inc, which says how: the walk over blocks,
// table descriptions and sequences is wave-uniform, with the Huffman and FSE tables of the page in LDS (10 148 bytes, all lanes
// storing the same cell); Huffman literals are decoded by up to four lanes, a stream each, into the tail of the page's own slot;
// the bytes of a literal run and of a match are spread over the lanes, a match 64 bytes per step. Bytes that other lanes of the
// wavefront stored are read back from global memory under the rule k_pq_unsnap rests on, so `buf` is neither const nor
// __restrict__ here either. The host has checked the frame header and the chain of block headers (qh_zstd_check_frame); the
// walk checks them again as it goes, and every length, count, accuracy, weight and offset before it is followed. The content
// checksum is not verified. A refused page leaves its slot half written.
__global__ __launch_bounds__(64) void k_pq_unzstd(u8* buf, const qh_pq_unpack* __restrict__ tab, u32 n, u64* err, u32* status) {
  __shared__ qh_zs_tables T;
  const u32 k = blockIdx.x;
  if (k >= n) return;
  const qh_pq_unpack u = tab[k];
  const u32 lane = (u32)qh_lane();
  const u32 reason = qh_zstd_frame(buf + u.src, u.src_size, u.start, buf + u.dst, u.dst_size, &T, lane);
  if (lane == 0) {
    if (status) status[k] = reason;
    if (reason && err) pq_report(err, u.page, QH_PQ_R_ZSTD_BASE + reason);
  }
}

// The gzip switch: one wavefront (a workgroup of its own) unpacks one GZIP page, a gzip member around one DEFLATE stream, from
// the uploaded chunks into its slot of the unpack area, both in `buf`. The decoder is device/qhip_inflate.inc, which says how:
// the walk over blocks, code lengths and symbols is wave-uniform; the decode tables of the block's two Huffman codes lie in LDS
// (7 316 bytes) and are built by the lanes together, lane L counting and placing the symbols of length L, then a symbol per
// lane filling its cells; decoded literals are gathered a lane each and stored up to 64 at a time; a stored block's bytes and a
// match are spread over the lanes, a match 64 bytes per step. Bytes that other lanes of the wavefront stored are read back
// from global memory under the rule k_pq_unsnap rests on, so `buf` is neither const nor __restrict__ here either. The host has
// checked the member header and ISIZE (qh_gzip_check_member); the walk checks every length, count, code and distance before it
// is followed. The CRC32 is not verified. A refused page leaves its slot half written.
__global__ __launch_bounds__(64) void k_pq_ungzip(u8* buf, const qh_pq_unpack* __restrict__ tab, u32 n, u64* err, u32* status) {
  __shared__ qh_infl_tables T;
  const u32 k = blockIdx.x;
  if (k >= n) return;
  const qh_pq_unpack u = tab[k];
  const u32 lane = (u32)qh_lane();
  const u32 reason = qh_inflate_member(buf + u.src, u.src_size, u.start, buf + u.dst, u.dst_size, &T, lane);
  if (lane == 0) {
    if (status) status[k] = reason;
    if (reason && err) pq_report(err, u.page, QH_PQ_R_GZIP_BASE + reason);
  }
}

// The lz4 switch: one wavefront (a workgroup of its own) unpacks one bare LZ4 block — an LZ4_RAW page, a legacy LZ4 page, or one
// frame of a legacy page in Hadoop's framing, which the host has split — from the uploaded chunks into its slot, or its slice
// of the page's slot, in the unpack area, both in `buf`. The decoder is device/qhip_lz4.inc, which says how: k_pq_unsnap's
// sibling. The walk over the sequences is wave-uniform and, each byte it reads declared uniform, scalar; token, extension and
// offset bytes come from a 1 KB tile of the input staged in LDS, and a literal run that lies inside the tile is taken from
// there; literals and match bytes are spread over the lanes, four loads in flight, a match of any length in 64-byte steps under
// qh_snap_copy_src's modulo rule. Bytes that other lanes of the wavefront stored are read back from global memory under the
// rule k_pq_unsnap rests on, with its wavefront-scope fence per sequence, so `buf` is neither const nor __restrict__ here
// either. The host has checked the 255x bound (qh_lz4_check_sizes); the walk checks every length and offset before it is
// followed. A refused block leaves its slot half written.
static_assert(QH_LZ4_TILE == kPqTile, "the LZ4 decoder's tile is the one the other walks stage their input in");
__global__ __launch_bounds__(64) void k_pq_unlz4(u8* buf, const qh_pq_unpack* __restrict__ tab, u32 n, u64* err, u32* status) {
  __shared__ __attribute__((aligned(16))) u8 tile[kPqTile];
  const u32 k = blockIdx.x;
  if (k >= n) return;
  const qh_pq_unpack u = tab[k];
  const u32 lane = (u32)qh_lane();
  const u32 reason = qh_lz4_block(buf + u.src, u.src_size, buf + u.dst, u.dst_size, tile, lane);
  if (lane == 0) {
    if (status) status[k] = reason;
    if (reason && err) pq_report(err, u.page, QH_PQ_R_LZ4_BASE + reason);
  }
}

// One wavefront per data page, 64 rows per step, the steps aligned to the column's 64-row words: a lane's row is word * 64 +
// lane, its validity bit is bit `lane` of one word, and a Boolean column's word is one ballot. The lane's value index is the
// page's running non-NULL count plus its rank in the step. Dictionary pages: a run cursor moves forward under wave-uniform
// control until the step's highest index is inside or behind it; a lane whose index lies in the current run takes the RLE
// value or extracts its bits.
//
// Encoding set 2 adds a second instance of the same body, k_pq_values_ext, for the pages k_pq_values leaves alone: RLE Boolean
// values (the run cursor at width 1, the "index" taken as the bit, no dictionary), BYTE_STREAM_SPLIT (one more gather),
// DELTA_BINARY_PACKED (read as PLAIN from the slot k_pq_delta filled) and DELTA_LENGTH_BYTE_ARRAY (the entries k_pq_delta
// wrote) and, with the DELTA_BYTE_ARRAY switch, DELTA_BYTE_ARRAY: a Utf8 page's entries, whose prefix lengths are scattered to
// the column's per-row array beside length and position; a FIXED_LEN_BYTE_ARRAY page arrives as QH_PQ_ENC_DELTA, dense in its
// slot behind k_pq_dba_fill. It is launched only for a file that has such a page; kExt = false compiles to the kernel of
// encoding set 1.
template <bool kExt>
__device__ __forceinline__ void pq_values_body(const u8* __restrict__ buf, const qh_pq_page* __restrict__ pages, u32 npages, const qh_pq_col* __restrict__ cols,
                                               const qh_pq_state* __restrict__ state, u64* err, u64* utf8_bytes) {
  const u32 page = (blockIdx.x * QH_BLOCK + threadIdx.x) >> 6;
  if (page >= npages) return;
  const qh_pq_page pg = pages[page];
  if (kExt ? pg.enc < QH_PQ_ENC_RLE_BOOL : pg.enc >= QH_PQ_ENC_DICTPAGE) return;
  if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ULL) return;   // (an earlier pass found an offender)
  const qh_pq_col col = cols[pg.col];
  const qh_pq_state st = state[page];
  const int lane = qh_lane();
  const u64 nn = st.nonnull;
  const u32 pw = qh_pq_phys_bytes(col.phys, col.flba);
  const bool delta = kExt && pg.enc == QH_PQ_ENC_DELTA;   // (its nn dense values lie in its slot of the decoded area)
  const u8* v = delta ? buf + pg.dict_pos : buf + pg.pos + st.values_off;
  const u64 vsize = delta ? nn * pw : (u64)pg.size - st.values_off;
  const bool dict = pg.enc == QH_PQ_ENC_DICT;
  const bool rleb = kExt && pg.enc == QH_PQ_ENC_RLE_BOOL, bss = kExt && pg.enc == QH_PQ_ENC_BSS;
  const bool runs = dict || rleb;
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
  } else if (rleb) {
    if (nn) {
      if (vsize < 4) reason = QH_PQ_R_RLE_LENGTH;
      else {
        slen = qh_pq_le32(v); s = v + 4; w = 1;
        if (slen > vsize - 4) reason = QH_PQ_R_RLE_LENGTH;
      }
    }
  } else if (bss) {
    if (nn * pw != vsize) reason = QH_PQ_R_BSS_SIZE;   // (no stride is guessed)
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
    if (runs) {
      bool served = !valid;
      for (;;) {
        if (!served && idx >= run.start && idx < run.start + run.count) { index = qh_pq_run_value(s, &run, idx, w); served = true; }
        if (run.start + run.count >= base) break;
        reason = (u32)qh_pq_next_run(s, slen, &cpos, w, &run);
        if (reason) break;
      }
      if (reason) break;
      if (dict && qh_ballot(valid && index >= pg.dict_n)) { reason = QH_PQ_R_DICT_INDEX; break; }
      if (rleb && qh_ballot(valid && index > 1)) { reason = QH_PQ_R_RLE_LENGTH; break; }
    }
    u64 lo = 0, hi = 0, spos = 0;
    u32 slen_row = 0;
    bool bit = false;
    if (valid) {
      if (col.phys == QH_PQ_P_BYTES) {
        const qh_pq_ent e = col.ent[pg.ent + (dict ? (u64)index : idx)];
        spos = e.pos; slen_row = e.len;
        // (a DELTA_BYTE_ARRAY page: pos is where the suffix lies, and the row's prefix length goes to the column's zeroed array)
        if (kExt && pg.enc == QH_PQ_ENC_DBA && col.prefix) col.prefix[row] = e.pad;
      } else if (col.phys == QH_PQ_P_BOOL) {
        bit = rleb ? index != 0 : (v[idx >> 3] >> (idx & 7)) & 1;
      } else if (bss) {
        qh_pq_read_value_bss(v, nn, idx, col.phys, col.flba, &lo, &hi);
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

__global__ __launch_bounds__(QH_BLOCK) void k_pq_values(const u8* __restrict__ buf, const qh_pq_page* __restrict__ pages, u32 npages,
                                                        const qh_pq_col* __restrict__ cols, const qh_pq_state* __restrict__ state, u64* err, u64* utf8_bytes) {
  pq_values_body<false>(buf, pages, npages, cols, state, err, utf8_bytes);
}
__global__ __launch_bounds__(QH_BLOCK) void k_pq_values_ext(const u8* __restrict__ buf, const qh_pq_page* __restrict__ pages, u32 npages,
                                                            const qh_pq_col* __restrict__ cols, const qh_pq_state* __restrict__ state, u64* err, u64* utf8_bytes) {
  pq_values_body<true>(buf, pages, npages, cols, state, err, utf8_bytes);
}

__device__ __forceinline__ u64 pq_shfl_up64(u64 v, int d) {
  const u32 lo = (u32)__shfl_up((int)(u32)v, d, 64), hi = (u32)__shfl_up((int)(u32)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 pq_incl_scan64(u64 v, int lane) {
  for (int d = 1; d < 64; d <<= 1) { const u64 t = pq_shfl_up64(v, d); if (lane >= d) v += t; }
  return v;
}
__device__ __forceinline__ u64 pq_lane63(u64 v) {
  return ((u64)(u32)__shfl((int)(u32)(v >> 32), 63, 64) << 32) | (u32)__shfl((int)(u32)v, 63, 64);
}

// Encoding set 2: one wavefront (a workgroup of its own) per DELTA_BINARY_PACKED stream (device/qhip_delta.inc). The walk over
// the stream header and the block headers is serial and wave-uniform: every lane parses the same bytes. The values are taken 64
// per step: a step lies in one block and touches at most two miniblocks (a miniblock holds a multiple of 32 values), whose
// widths and byte positions every lane knows; lane l extracts delta k0 + l with byte loads of its own miniblock, adds the
// block's min delta, the wavefront scans (six rounds of __shfl_up on 64-bit values: the sums wrap mod 2^64, and a 4-byte type
// keeps the low half, which is the sum mod 2^32), the step's carry is added and lane 63's value is the next carry.
// A stream of a page (pages != NULL) is where the level pass says the values begin and has the page's non-NULL count; a raw
// stream (qhip_parquet_delta_decode) is what its table entry says. Dense values go to the stream's slot, from where
// k_pq_values_ext reads the page as PLAIN. The lengths of DELTA_LENGTH_BYTE_ARRAY get a second scan and become the page's
// (length, position) entries, what k_pq_strings writes for a PLAIN page: the bytes begin where the length stream ends, which is
// known only behind the last block, so the positions are written relative to it and every lane moves the entries it wrote
// itself (entry i > 0 belongs to lane (i - 1) & 63: a block is a multiple of 128 values) once the walk is over.
// Every loop advances by a block that holds a value and at least one byte, or by 64 values of it: bounded by the count, which
// the page's rows bound, and by the stream's bytes. A refused stream leaves its slot half written; nobody reads it.
// The DELTA_BYTE_ARRAY switch: a stream marked QH_PQ_DS_DBA is walked twice by the same code, first the prefix lengths, which
// go to the pad field of the entries, then, from where that stream ended, the suffix lengths, which become the entries' length
// (prefix + suffix) and the position of the suffix bytes as a DELTA_LENGTH_BYTE_ARRAY page's lengths do. The second walk reads
// back the prefix lengths the first one stored, from whichever lane: k_pq_unsnap's rule, with its fence between the walks. Each
// length is checked (device/qhip_dba.inc) before anything is made of it; of several offenders in a step the lowest lane's counts.
// Those streams have an instance of the body of their own, k_pq_delta_dba, launched only where there is one, so that
// k_pq_delta compiles to what it was; each instance leaves the other's streams alone.
template <bool kDba>
__device__ __forceinline__ void pq_delta_body(u8* buf, const qh_pq_dstream* __restrict__ tab, u32 n, const qh_pq_page* __restrict__ pages,
                                              const qh_pq_col* __restrict__ cols, const qh_pq_state* __restrict__ state, u64* err, u32* status, u64* ends) {
  const u32 k = blockIdx.x;
  if (k >= n) return;
  const qh_pq_dstream t = tab[k];
  if (kDba != ((t.width & QH_PQ_DS_DBA) != 0)) return;
  const int lane = qh_lane();
  u64 src = t.src, size = t.src_size, count = t.count;
  const bool dba = kDba;
  const bool lengths = t.width & QH_PQ_DS_LENGTHS;
  const u32 width = t.width & 0xFFu, bits = dba ? 32u : width * 8;
  qh_pq_ent* ent = dba ? (qh_pq_ent*)(buf + t.dst) : nullptr;
  if (pages) {
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ULL) return;   // (the level pass found an offender: its state is void)
    const qh_pq_page pg = pages[t.page];
    const qh_pq_state st = state[t.page];
    src = pg.pos + st.values_off; size = (u64)pg.size - st.values_off; count = st.nonnull;
    if (!count) return;   // (a page without non-NULL rows is not looked at beyond its levels)
    if (lengths || (dba && !width)) ent = cols[pg.col].ent + pg.ent;
  }
  u8* out = buf + t.dst;
  u32 reason = QH_PQ_OK;
  u64 begin = 0, pos = 0, sum = 0;   // begin: where this walk's stream begins behind src; sum (lengths): bytes of the values so far
  const u32 walks = dba ? 2u : 1u;
  for (u32 walk = 0; walk < walks && !reason; ++walk) {
    const bool pre = dba && walk == 0, suf = dba && walk == 1, lens = lengths || suf;
    begin += pos;
    const u8* s = buf + src + begin;
    const u64 ssize = size - begin;
    qh_dl_head h;
    reason = (u32)qh_dl_header(s, ssize, &h);
    if (!reason && (u64)h.total != count) reason = QH_PQ_R_DELTA_COUNT;
    u64 carry = 0, produced = 0;
    u32 prev_len = 0;   // (suffix walk) the length of the value before the step
    pos = 0; sum = 0;
    if (!reason) {
      pos = h.end;
      if (count) {
        carry = h.first; produced = 1;
        if (pre) {
          reason = (u32)qh_dba_check_prefix((u32)carry, true);
          if (!reason && lane == 0) ent[0].pad = 0;
        } else if (lens) {
          if (suf) reason = (u32)qh_dba_check_value(0, (u32)carry, 0, width);
          else if ((int)(u32)carry < 0) reason = QH_PQ_R_DELTA_LENGTH;
          if (!reason && lane == 0) { qh_pq_ent e; e.pos = 0; e.len = (u32)carry; e.pad = 0; ent[0] = e; }
          sum = (u32)carry; prev_len = (u32)carry;
        } else if (lane == 0) {
          if (width == 4) ((u32*)out)[0] = (u32)carry; else ((u64*)out)[0] = carry;
        }
      }
    }
    while (!reason && produced < count) {
      u64 min_delta = 0, wat = 0, at = 0;
      reason = (u32)qh_dl_block(s, ssize, pos, h.mpb, &min_delta, &wat, &at);
      if (reason) break;
      const u64 left = count - produced, in_block = left < (u64)h.block ? left : (u64)h.block;
      const u64 mbytes = h.vpm >> 3;   // bytes of a miniblock per bit of width
      u32 cur_m = 0, cur_w = s[wat];
      reason = (u32)qh_dl_miniblock(cur_w, bits, h.vpm, ssize - at);
      for (u64 k0 = 0; !reason && k0 < in_block; k0 += 64) {
        const u64 last = k0 + 63 < in_block ? k0 + 63 : in_block - 1;
        const u32 m_lo = (u32)(k0 / h.vpm), m_hi = (u32)(last / h.vpm);
        if (m_lo != cur_m) {   // the step before ended with its miniblock
          at += mbytes * cur_w; cur_m = m_lo; cur_w = s[wat + cur_m];
          reason = (u32)qh_dl_miniblock(cur_w, bits, h.vpm, ssize - at);
          if (reason) break;
        }
        u64 next_at = 0;
        u32 next_w = 0;
        if (m_hi != m_lo) {
          next_at = at + mbytes * cur_w; next_w = s[wat + m_hi];
          reason = (u32)qh_dl_miniblock(next_w, bits, h.vpm, ssize - next_at);
          if (reason) break;
        }
        const u64 v = k0 + (u64)lane;
        const bool active = v <= last;
        u64 x = 0;
        if (active) {
          const u32 mi = (u32)(v / h.vpm);
          const u64 kk = v - (u64)mi * h.vpm;
          x = (mi == m_lo ? qh_dl_extract(s + at, kk, cur_w) : qh_dl_extract(s + next_at, kk, next_w)) + min_delta;
        }
        const u64 val = carry + pq_incl_scan64(x, lane);
        carry = pq_lane63(val);   // (an idle lane adds 0: lane 63 holds the step's last value)
        if (pre) {
          if (qh_ballot(active && qh_dba_check_prefix((u32)val, false))) { reason = QH_PQ_R_DBA_PREFIX; break; }
          if (active) ent[produced + v].pad = (u32)val;
        } else if (lens) {
          const u32 len = (u32)val;   // (suffix walk: the suffix length)
          u32 pfx = 0, full = len;
          if (suf) {
            if (active) pfx = ent[produced + v].pad;
            full = pfx + len;
            u32 before = (u32)__shfl_up((int)full, 1, 64);
            if (lane == 0) before = prev_len;
            const u32 bad = active ? (u32)qh_dba_check_value(pfx, len, before, width) : 0u;
            const u64 who = qh_ballot(bad != 0);
            if (who) { reason = qh_readlane32(bad, __builtin_ctzll(who)); break; }
            prev_len = qh_readlane32(full, (int)(last - k0));
          } else if (qh_ballot(active && (int)len < 0)) { reason = QH_PQ_R_DELTA_LENGTH; break; }
          const u64 incl = pq_incl_scan64(active ? (u64)len : 0, lane);
          if (active) { qh_pq_ent e; e.pos = sum + incl - len; e.len = full; e.pad = pfx; ent[produced + v] = e; }
          sum += pq_lane63(incl);
        } else if (active) {
          if (width == 4) ((u32*)out)[produced + v] = (u32)val; else ((u64*)out)[produced + v] = val;
        }
        if (m_hi != m_lo) { at = next_at; cur_w = next_w; cur_m = m_hi; }
      }
      if (reason) break;
      pos = at + mbytes * cur_w;   // (the last miniblock that holds a value is stored whole)
      produced += in_block;
    }
    if (!reason && lens) {
      if (suf) reason = (u32)qh_dba_check_total(sum, ssize - pos);
      else if (sum > ssize - pos) reason = QH_PQ_R_DELTA_LENGTH;
      if (!reason) {
        const u64 base = src + begin + pos;
        if (lane == 0 && count) ent[0].pos = base;   // (a raw stream may hold no value: then it has no entry either)
        for (u64 i = 1 + (u64)lane; i < count; i += 64) ent[i].pos += base;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  if (lane == 0) {
    if (status) status[k] = reason;
    if (ends) ends[k] = begin + pos;
    if (reason && err) pq_report(err, t.page, reason);
  }
}

__global__ __launch_bounds__(64) void k_pq_delta(u8* buf, const qh_pq_dstream* __restrict__ tab, u32 n, const qh_pq_page* __restrict__ pages,
                                                 const qh_pq_col* __restrict__ cols, const qh_pq_state* __restrict__ state, u64* err, u32* status, u64* ends) {
  pq_delta_body<false>(buf, tab, n, pages, cols, state, err, status, ends);
}
__global__ __launch_bounds__(64) void k_pq_delta_dba(u8* buf, const qh_pq_dstream* __restrict__ tab, u32 n, const qh_pq_page* __restrict__ pages,
                                                     const qh_pq_col* __restrict__ cols, const qh_pq_state* __restrict__ state, u64* err, u32* status, u64* ends) {
  pq_delta_body<true>(buf, tab, n, pages, cols, state, err, status, ends);
}

// The DELTA_BYTE_ARRAY switch, a Utf8 column that has such a page, behind the scan of its lengths into offsets: k_csv_copy_utf8
// with a prefix. Row k's value is off[k + 1] - off[k] bytes long, of which the last (length - prefix[k]) lie in the page at
// strpos[k]: they go to data[off[k] + prefix[k] ..), up to 64 by the row's own lane, longer ones by the whole wavefront. A row
// of another page of the column has prefix 0 and is copied whole. The first prefix[k] bytes are k_pq_dba_fill's.
__global__ __launch_bounds__(QH_BLOCK) void k_pq_dba_copy(const u8* __restrict__ buf, const u64* __restrict__ strpos, const u32* __restrict__ off,
                                                          const u32* __restrict__ prefix, u64 nrows, u8* __restrict__ data) {
  const u64 nwords = (nrows + 63) / 64;
  const u64 wave_global = ((u64)blockIdx.x * QH_BLOCK + threadIdx.x) >> 6;
  const u64 nwaves = ((u64)gridDim.x * QH_BLOCK) >> 6;
  const int lane = qh_lane();
  for (u64 j = wave_global; j < nwords; j += nwaves) {
    const u64 k = j * 64 + lane;
    u64 src = 0;
    u32 dst = 0, len = 0;
    if (k < nrows) {
      const u32 p = prefix[k], whole = off[k + 1] - off[k];
      src = strpos[k]; dst = off[k] + p; len = p < whole ? whole - p : 0u;   // (p <= whole was checked: the value is prefix + suffix)
    }
    if (len <= 64) for (u32 b = 0; b < len; ++b) data[dst + b] = buf[src + b];
    u64 big = qh_ballot(len > 64);
    while (big) {
      const int l = __builtin_ctzll(big);
      big &= big - 1;
      const u64 s2 = qh_readlane64(src, l);
      const u32 d2 = qh_readlane32(dst, l), n2 = qh_readlane32(len, l);
      for (u32 b = lane; b < n2; b += 64) data[d2 + b] = buf[s2 + b];
    }
  }
}

// The DELTA_BYTE_ARRAY switch: the prefixes. One wavefront (a workgroup of its own) per page, 64 rows of it per step, lane =
// row; the suffixes are in place. Byte j < prefix[r] of row r is byte j of the row before it, which took it from the row before
// that unless it is one of its own suffix bytes: so it is byte j of the nearest earlier non-NULL row k with prefix[k] <= j, and
// there a suffix byte. Inside a step that row is found with one ballot of "non-NULL and prefix <= j" and the highest set bit
// below the lane (qh_dba_source_lane): at byte j the lanes with prefix <= j are read and the others written, so a step reads
// nothing that it writes. Where no lane below qualifies, the byte is byte j of the last non-NULL row of the steps before, which
// is complete by then: that load does read what this wavefront stored in an earlier step, from whichever lane, under the rule
// k_pq_unsnap rests on, with its wavefront-scope fence per step. A step that holds a prefix above 64 bytes walks its rows in
// order instead, the whole wavefront copying each row's prefix from the row before, 64 bytes per trip, a fence per row. NULL
// rows are idle lanes and never a source; rows outside the page are idle too. Every prefix was checked by k_pq_delta against
// the length of the value before it, and the page's first is 0, so every source lies in a row of the page.
// Row space (off != NULL; a Utf8 column behind the host wait and k_pq_dba_copy): a job is the rows [first, first + n) of the
// column, the steps aligned to its 64-row validity words; valid == NULL means every row is there. Value space (off == NULL; a
// FIXED_LEN_BYTE_ARRAY page behind k_pq_delta, before the wait): a job's entries lie at data[first ..), value i goes to
// data[out + i * width ..) and there are state[page].nonnull of them; each lane first copies its own suffix (at most 16 bytes)
// from where its entry says, then the fill runs as above after a fence. A set err word means the entries may be half written:
// the wavefront leaves.
__device__ __forceinline__ u64 pq_shfl64(u64 v, int from) {
  return ((u64)(u32)__shfl((int)(u32)(v >> 32), from, 64) << 32) | (u32)__shfl((int)(u32)v, from, 64);
}
__global__ __launch_bounds__(64) void k_pq_dba_fill(u8* data, const qh_pq_fill* __restrict__ jobs, u32 n, const u32* __restrict__ off, const u32* __restrict__ prefix,
                                                    const u64* __restrict__ valid_words, const qh_pq_state* __restrict__ state, const u64* err) {
  const u32 k = blockIdx.x;
  if (k >= n) return;
  const qh_pq_fill job = jobs[k];
  const int lane = qh_lane();
  const bool rows = off != nullptr;
  u64 r_begin = 0, r_end = 0;
  const qh_pq_ent* ent = nullptr;
  if (rows) { r_begin = job.first; r_end = job.first + job.n; }
  else {
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ULL) return;
    r_end = state[job.page].nonnull;
    ent = (const qh_pq_ent*)(data + job.first);
  }
  u64 before = 0;        // where the last non-NULL row of the steps before begins in data
  bool have = false;
  for (u64 t0 = r_begin & ~(u64)63; t0 < r_end; t0 += 64) {
    const u64 r = t0 + (u64)lane;
    bool valid = r >= r_begin && r < r_end;
    if (valid && rows && valid_words) valid = (valid_words[t0 >> 6] >> lane) & 1ULL;
    u32 p = 0;
    u64 o = 0;
    if (valid) {
      if (rows) { p = prefix[r]; o = off[r]; }
      else {
        const qh_pq_ent e = ent[r];
        p = e.pad; o = job.out + r * job.width;
        for (u32 b = p; b < e.len; ++b) data[o + b] = data[e.pos + (b - p)];   // (e.len is the width: k_pq_delta checked it)
      }
    }
    const u64 there = qh_ballot(valid);
    if (!there) continue;
    if (!rows) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (qh_ballot(valid && p > QH_DBA_STEP_PREFIX)) {
      u64 todo = there;
      while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        const u32 pl = qh_readlane32(p, l);
        const u64 ol = qh_readlane64(o, l);
        if (have) for (u32 b = lane; b < pl; b += 64) data[ol + b] = data[before + b];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        before = ol; have = true;
      }
    } else {
      for (u32 j = 0; qh_ballot(valid && p > j); ++j) {
        const u64 m = qh_ballot(valid && p <= j);
        const int sl = qh_dba_source_lane(m, lane);
        const u64 so = pq_shfl64(o, sl < 0 ? lane : sl);
        if (valid && p > j && (sl >= 0 || have)) data[o + j] = data[(sl >= 0 ? so : before) + j];
      }
      before = qh_readlane64(o, 63 - __builtin_clzll(there)); have = true;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  }
}

// ---------------------------------------------------------------- launchers
void launch_pq_delta(uint8_t* buf, const qh_pq_dstream* tab, uint32_t n, const qh_pq_page* pages, const qh_pq_col* cols, const qh_pq_state* state, uint64_t* err,
                     uint32_t* status, uint64_t* ends, uint32_t kinds, hipStream_t s) {
  if (!n) return;
  if (kinds & 1u) hipLaunchKernelGGL(k_pq_delta, dim3(n), dim3(64), 0, s, (u8*)buf, tab, (u32)n, pages, cols, state, (u64*)err, (u32*)status, (u64*)ends);
  if (kinds & 2u) hipLaunchKernelGGL(k_pq_delta_dba, dim3(n), dim3(64), 0, s, (u8*)buf, tab, (u32)n, pages, cols, state, (u64*)err, (u32*)status, (u64*)ends);
}
void launch_pq_dba_copy(const uint8_t* buf, const uint64_t* strpos, const uint32_t* offsets, const uint32_t* prefix, uint64_t nrows, uint8_t* data, hipStream_t s) {
  if (!nrows) return;
  uint64_t g = ((nrows + 63) / 64 * 64 + QH_BLOCK - 1) / QH_BLOCK;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(k_pq_dba_copy, dim3((unsigned)g), dim3(QH_BLOCK), 0, s, (const u8*)buf, (const u64*)strpos, (const u32*)offsets, (const u32*)prefix, (u64)nrows,
                     (u8*)data);
}
void launch_pq_dba_fill(uint8_t* data, const qh_pq_fill* jobs, uint32_t n, const uint32_t* off, const uint32_t* prefix, const uint64_t* valid, const qh_pq_state* state,
                        const uint64_t* err, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_pq_dba_fill, dim3(n), dim3(64), 0, s, (u8*)data, jobs, (u32)n, (const u32*)off, (const u32*)prefix, (const u64*)valid, state, (const u64*)err);
}
void launch_pq_values_ext(const uint8_t* buf, const qh_pq_page* pages, uint32_t npages, const qh_pq_col* cols, const qh_pq_state* state, uint64_t* err,
                          uint64_t* utf8_bytes, hipStream_t s) {
  if (!npages) return;
  const unsigned g = (unsigned)(((uint64_t)npages * 64 + QH_BLOCK - 1) / QH_BLOCK);
  hipLaunchKernelGGL(k_pq_values_ext, dim3(g), dim3(QH_BLOCK), 0, s, (const u8*)buf, pages, (u32)npages, cols, state, (u64*)err, (u64*)utf8_bytes);
}
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
void launch_pq_unzstd(uint8_t* buf, const qh_pq_unpack* tab, uint32_t n, uint64_t* err, uint32_t* status, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_pq_unzstd, dim3(n), dim3(64), 0, s, (u8*)buf, tab, (u32)n, (u64*)err, (u32*)status);
}
void launch_pq_ungzip(uint8_t* buf, const qh_pq_unpack* tab, uint32_t n, uint64_t* err, uint32_t* status, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_pq_ungzip, dim3(n), dim3(64), 0, s, (u8*)buf, tab, (u32)n, (u64*)err, (u32*)status);
}
void launch_pq_unlz4(uint8_t* buf, const qh_pq_unpack* tab, uint32_t n, uint64_t* err, uint32_t* status, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_pq_unlz4, dim3(n), dim3(64), 0, s, (u8*)buf, tab, (u32)n, (u64*)err, (u32*)status);
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
