// kernels_csv.hip — CSV text in HBM -> typed Arrow columns (gfx950, wave64), compiled ahead of time. The host side is csv.cpp
// (qhip_table_from_csv); the per-byte and per-field code is device/qhip_csv.inc, shared with the CPU tests. Replaces the
// reference's host CSV reader (datasource/file/csv.rs:33-70) for files inside the strict grammar of DESIGN §3.8.
//
//   k_csv_scan<false>  every byte once, 16 per lane and load: record ends per 16 KB chunk, structural needs-host reasons
//   k_csv_scan<true>   the same walk again with the scanned chunk counts: where every record starts (u64)
//   k_csv_decode<G>    one record per lane, 256 consecutive records per workgroup, their bytes staged in LDS (G = 1: the plain
//                      walk; G = 2: quoted fields, Boolean, Timestamp)
//   k_csv_copy_utf8    string bytes from the file into the column's data buffer, at the scanned offsets
//   k_csv_copy_utf8_q  ... with doubled quotes undoubled (grammar level 2)
//
// Every byte offset into the file is 64 bits wide. Vector loads may read up to 15 bytes past the file's end: every device
// allocation carries 64 bytes of slack (DevBuf::alloc), and what is read there is masked out before it is looked at.
#include <hip/hip_runtime.h>
#include <cstring>

#include "device/qhip_status.h"
#include "device/qhip_device.hpp"
#include "device/qhip_csv.inc"
#include "common.hpp"
#include "kernels.hpp"

namespace qhip {

static_assert(sizeof(CsvCol) == sizeof(qh_csv_col) && kCsvCols == QH_CSV_MAX_COLS, "host and device descriptors of a CSV column differ");
static_assert(kCsvChunk == QH_BLOCK * 16 * 4, "a scan chunk is four 16-byte vectors per thread");
struct CsvColsArg { qh_csv_col c[QH_CSV_MAX_COLS]; };

typedef u32 csv_v4u __attribute__((ext_vector_type(4)));

// the smallest (position << 8 | reason) wins: the first offending byte / record and why. Offenders are rare, and a lane whose
// word is not below the current one stays off the atomic.
__device__ __forceinline__ void csv_report(u64* err, u64 where, u32 reason) {
  const u64 mine = (where << 8) | reason;
  if (mine < __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(err, mine);
}

__device__ __forceinline__ u32 csv_wave_incl_scan(u32 v) {
  const int lane = qh_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u32 t = (u32)__shfl_up((int)v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// is file position q a line feed, for the look-back of the byte after it? The position in front of the data counts as one.
__device__ __forceinline__ bool csv_is_lf_before(const u8* buf, u64 d0, u64 q_plus_1) {
  if (q_plus_1 == d0) return true;
  return q_plus_1 > d0 && buf[q_plus_1 - 1] == '\n';
}

// One workgroup per 16 KB chunk of the file; lane t of iteration `it` owns the 16 aligned bytes at chunk + it * 4096 + t * 16
// (consecutive lanes, consecutive vectors: coalesced). Bytes outside [d0, n) are masked. A record ends at every '\n'.
//   WRITE = false: counts[chunk] = record ends in the chunk, *total += them; quote bytes, lone '\r' and empty lines -> *err
//   WRITE = true : counts[] holds the exclusive scan; starts[1 + rank of the '\n'] = its position + 1
// The look-back (is the byte before this "\n" or "\r\n" another '\n': an empty line) and the look-ahead (is the byte after
// this '\r' a '\n') cross vector, lane and workgroup edges by reading the neighbouring bytes themselves, which the neighbouring
// lane has just pulled into the cache.
template <bool WRITE>
__global__ __launch_bounds__(QH_BLOCK) void k_csv_scan(const u8* __restrict__ buf, u64 d0, u64 n, int quote, u32* counts, u64* starts, u64* err,
                                                       u64* total, u32 tail) {
  __shared__ u32 wtot[QH_BLOCK / 64];
  const u64 chunk = (u64)blockIdx.x * kCsvChunk;
  u32 running = WRITE ? counts[blockIdx.x] : 0u;   // records that end before this iteration's bytes
  u32 mine = 0;
  if (WRITE && blockIdx.x == 0 && threadIdx.x == 0) starts[0] = d0;
#pragma unroll 1
  for (int it = 0; it < 4; ++it) {
    const u64 pos = chunk + (u64)it * (QH_BLOCK * 16) + (u64)threadIdx.x * 16;
    u32 lf = 0, cr = 0, qt = 0;
    if (pos < n && pos + 16 > d0) {
      const csv_v4u v = *(const csv_v4u*)(buf + pos);   // (aligned; past n: inside the allocation's slack)
      const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const u32 cls = qh_csv_byte_class((u8)(w[j >> 2] >> (8 * (j & 3))), quote);
        lf |= (cls & QH_CSV_B_LF ? 1u : 0u) << j;
        cr |= (cls & QH_CSV_B_CR ? 1u : 0u) << j;
        qt |= (cls & QH_CSV_B_QUOTE ? 1u : 0u) << j;
      }
      u32 in = 0xFFFFu;
      if (pos < d0) in &= 0xFFFFu << (u32)(d0 - pos);
      if (pos + 16 > n) in &= 0xFFFFu >> (u32)(pos + 16 - n);
      lf &= in; cr &= in; qt &= in;
    }
    if (!WRITE) {
      if (qt) csv_report(err, pos + (u32)__builtin_ctz(qt), QH_CSV_R_QUOTE);
      if (cr) {
        // the byte after lane position 15 is the next vector's first (or past the end: then the '\r' is alone)
        u32 lf_next = lf >> 1;
        if ((cr & 0x8000u) && pos + 16 < n && buf[pos + 16] == '\n') lf_next |= 0x8000u;
        const u32 lone = cr & ~lf_next;
        if (lone) csv_report(err, pos + (u32)__builtin_ctz(lone), QH_CSV_R_LONE_CR);
      }
      if (lf) {
        // bit j + 2 of lx / cx: position pos + j is a '\n' / '\r'; bits 1 and 0: the two bytes in front of the vector
        u32 lx = lf << 2, cx = cr << 2;
        if (pos < d0 && pos + 16 >= d0) lx |= 1u << (u32)(d0 - 1 - pos + 2);   // the position in front of the data counts as '\n'
        if (lf & 3u) {
          if (csv_is_lf_before(buf, d0, pos)) lx |= 2u;
          if (pos >= 1 && csv_is_lf_before(buf, d0, pos - 1)) lx |= 1u;
          if (pos > d0 && buf[pos - 1] == '\r') cx |= 2u;
        }
        // '\n' at j is an empty line when j - 1 is a '\n', or j - 1 is a '\r' and j - 2 is a '\n'
        const u32 empty = lf & (((lx >> 1) | ((cx >> 1) & lx)) & 0xFFFFu);
        if (empty) csv_report(err, pos + (u32)__builtin_ctz(empty), QH_CSV_R_EMPTY_LINE);
      }
      mine += (u32)__builtin_popcount(lf);
    } else {
      const u32 c = (u32)__builtin_popcount(lf);
      const u32 incl = csv_wave_incl_scan(c);
      const int wave = threadIdx.x >> 6;
      if (qh_lane() == 63) wtot[wave] = incl;
      __syncthreads();
      u32 before = running + incl - c;
      u32 all = 0;
#pragma unroll
      for (int w = 0; w < QH_BLOCK / 64; ++w) { if (w < wave) before += wtot[w]; all += wtot[w]; }
      running += all;
      __syncthreads();   // (wtot is written again in the next iteration)
      u32 m = lf;
      u64 r = (u64)before + 1;
      while (m) {
        const u32 j = (u32)__builtin_ctz(m);
        m &= m - 1;
        starts[r++] = pos + j + 1;
      }
    }
  }
  if (!WRITE) {
    const u32 w = (u32)qh_wave_sum_u64(mine);
    if (qh_lane() == 0) wtot[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
      u32 t = 0;
      for (int k = 0; k < QH_BLOCK / 64; ++k) t += wtot[k];
      counts[blockIdx.x] = t;
      if (t) atomicAdd(total, (u64)t);   // (one atomic per 16 KB of text)
    }
  } else if (tail && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    // a last record without a line end: it ends where a '\n' at position n would (running = every record end of the file)
    starts[(u64)running + 1] = n + 1;
  }
}

// One record per lane, a workgroup on 256 consecutive records, a wavefront on 64: the validity word of 64 rows is one ballot
// (no atomics on the bitmaps). The records of a workgroup are one contiguous byte range of the file: it is staged into LDS with
// coalesced 16-byte loads and every lane walks its record there (walking global memory byte by byte, 64 lanes touch 64 different
// lines per load). A range that does not fit (one very long field) is walked in global memory instead. The parsers take
// generic pointers, so both paths run the same code.
// GRAMMAR = 1: the plain walk (qh_csv_decode_record). GRAMMAR = 2 (qhip_ctx_set_csv_grammar): the quote-aware walk, an
// instantiation of its own so that the plain one carries nothing of it; the quote byte travels in bits 8.. of `delim` as
// quote + 1 (0: no byte is a quote), and a Boolean column's values word of 64 rows is a ballot like its validity word.
constexpr u32 kCsvLdsBytes = 48 * 1024;
template <int GRAMMAR>
__global__ __launch_bounds__(QH_BLOCK) void k_csv_decode(const u8* __restrict__ buf, u64 n, const u64* __restrict__ starts, u64 nrec, CsvColsArg cols,
                                                         int ncols, u32 nfields, u32 delim, u64* err, u64* null_counts, u64* utf8_bytes) {
  __shared__ __attribute__((aligned(16))) u8 tile[kCsvLdsBytes];
  const u64 r0 = (u64)blockIdx.x * QH_BLOCK;
  const u64 r1 = r0 + QH_BLOCK < nrec ? r0 + QH_BLOCK : nrec;
  const u64 t_begin = starts[r0];
  u64 t_end = starts[r1];
  if (t_end > n) t_end = n;                    // (the virtual line end behind a last record without one)
  const u64 base = t_begin & ~(u64)15;
  const u64 span = t_end - base;
  const bool staged = span <= kCsvLdsBytes;     // workgroup-uniform
  if (staged) {
    // (the last vector may reach up to 15 bytes past t_end <= n: inside the slack behind the file's allocation)
    for (u64 o = (u64)threadIdx.x * 16; o < span; o += (u64)QH_BLOCK * 16) *(csv_v4u*)(tile + o) = *(const csv_v4u*)(buf + base + o);
  }
  __syncthreads();
  const u64 row = r0 + threadIdx.x;
  const bool active = row < nrec;
  u64 vm = 0, tm = 0;
  if (active) {
    const u64 s = starts[row];
    u64 len = starts[row + 1] - 1 - s;          // without the '\n'
    const u8* p = staged ? tile + (s - base) : buf + s;
    if (len > 0 && p[len - 1] == '\r') --len;   // ... and without the '\r' of a "\r\n"
    int reason;
    if constexpr (GRAMMAR == 1) reason = qh_csv_decode_record(cols.c, ncols, nfields, (u8)delim, p, len, row, s, &vm);
    else reason = qh_csv_decode_record_q(cols.c, ncols, nfields, (u8)delim, (int)(delim >> 8) - 1, p, len, row, s, &vm, &tm);
    if (reason != QH_CSV_OK) csv_report(err, row, (u32)reason);
  }
  const u64 live = qh_ballot(active);
  const int lane = qh_lane();
  for (int k = 0; k < ncols; ++k) {
    const u64 word = qh_ballot(active && ((vm >> k) & 1ULL));
    if constexpr (GRAMMAR == 2) {
      if (cols.c[k].kind == QH_CSV_K_BOOL) {
        const u64 truth = qh_ballot(active && ((tm >> k) & 1ULL));   // (a NULL row's bit is 0)
        if (lane == 0 && live) ((u64*)cols.c[k].values)[row >> 6] = truth;
      }
    }
    u64 bytes = 0;
    if (cols.c[k].kind == QH_CSV_K_UTF8) bytes = qh_wave_sum_u64(active ? (u64)((const u32*)cols.c[k].values)[row] : 0ULL);
    if (lane == 0 && live) {
      cols.c[k].valid[row >> 6] = word;
      const u32 nulls = (u32)(__builtin_popcountll(live) - __builtin_popcountll(word));
      if (nulls) atomicAdd(&null_counts[k], (u64)nulls);
      if (bytes) atomicAdd(&utf8_bytes[k], bytes);
    }
  }
}

// Row k's bytes: file[strpos[k] .. + (off[k + 1] - off[k])) -> data[off[k] ..]. One wavefront per 64 rows: a row of up to 64
// bytes is copied by its own lane, longer ones by the whole wavefront afterwards (k_gather_utf8_bytes' scheme).
__global__ __launch_bounds__(QH_BLOCK) void k_csv_copy_utf8(const u8* __restrict__ buf, const u64* __restrict__ strpos, const u32* __restrict__ off, u64 nrows,
                                                            u8* __restrict__ data) {
  const u64 nwords = (nrows + 63) / 64;
  const u64 wave_global = ((u64)blockIdx.x * QH_BLOCK + threadIdx.x) >> 6;
  const u64 nwaves = ((u64)gridDim.x * QH_BLOCK) >> 6;
  const int lane = qh_lane();
  for (u64 j = wave_global; j < nwords; j += nwaves) {
    const u64 k = j * 64 + lane;
    u64 src = 0;
    u32 dst = 0, len = 0;
    if (k < nrows) { src = strpos[k]; dst = off[k]; len = off[k + 1] - dst; }
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

// The same at grammar level 2: strpos carries QH_CSV_POS_PAIRS for a row whose field holds doubled quotes (len is the
// UNESCAPED length; the raw span is longer by one byte per pair). Rows without the mark are copied exactly as above. A marked
// row of up to 64 raw bytes is undoubled by its own lane; a longer one (QH_CSV_POS_LONG) by the whole wavefront, 64 raw bytes
// per step: the ballot of "my byte is the quote" tells every lane whether its byte is the dropped half of a pair and where
// the bytes below it go (qh_csv_undouble_*: runs of quotes cross the steps, their parity is carried). The last step may read
// up to 63 bytes behind the field's closing quote: inside the file or the slack behind its allocation, and never written
// (their output position is at or behind the row's end).
__global__ __launch_bounds__(QH_BLOCK) void k_csv_copy_utf8_q(const u8* __restrict__ buf, const u64* __restrict__ strpos, const u32* __restrict__ off, u64 nrows,
                                                              u8* __restrict__ data, u32 quote) {
  const u64 nwords = (nrows + 63) / 64;
  const u64 wave_global = ((u64)blockIdx.x * QH_BLOCK + threadIdx.x) >> 6;
  const u64 nwaves = ((u64)gridDim.x * QH_BLOCK) >> 6;
  const int lane = qh_lane();
  for (u64 j = wave_global; j < nwords; j += nwaves) {
    const u64 k = j * 64 + lane;
    u64 src = 0;
    u32 dst = 0, len = 0;
    if (k < nrows) { src = strpos[k]; dst = off[k]; len = off[k + 1] - dst; }
    const bool pairs = (src & QH_CSV_POS_PAIRS) != 0, wide = (src & QH_CSV_POS_LONG) != 0;
    src &= QH_CSV_POS_MASK;
    if (!pairs) {
      if (len <= 64) for (u32 b = 0; b < len; ++b) data[dst + b] = buf[src + b];
    } else if (!wide) {
      u64 q = src;   // (at most 64 raw bytes)
      for (u32 b = 0; b < len; ++b) {
        const u8 c = buf[q];
        data[dst + b] = c;
        q += c == (u8)quote ? 2 : 1;
      }
    }
    u64 big = qh_ballot(!pairs && len > 64);
    while (big) {
      const int l = __builtin_ctzll(big);
      big &= big - 1;
      const u64 s2 = qh_readlane64(src, l);
      const u32 d2 = qh_readlane32(dst, l), n2 = qh_readlane32(len, l);
      for (u32 b = lane; b < n2; b += 64) data[d2 + b] = buf[s2 + b];
    }
    big = qh_ballot(pairs && wide);
    while (big) {
      const int l = __builtin_ctzll(big);
      big &= big - 1;
      const u64 s2 = qh_readlane64(src, l);
      const u32 d2 = qh_readlane32(dst, l), n2 = qh_readlane32(len, l);
      u64 emitted = 0;
      u32 carry = 0;
      for (u64 raw = 0; emitted < n2; raw += 64) {   // (every step emits at least 32 bytes)
        const u8 c = buf[s2 + raw + lane];
        const u64 quotes = qh_ballot(c == (u8)quote);
        const bool drop = qh_csv_undouble_drops(quotes, carry, lane);
        const u64 dropped = qh_ballot(drop);
        const u64 o = qh_csv_undouble_out(emitted, dropped, lane);
        if (!drop && o < n2) data[d2 + o] = c;
        emitted += (u64)__builtin_popcountll(~dropped);
        carry = qh_csv_undouble_carry(quotes, carry);
      }
    }
  }
}

// ---------------------------------------------------------------- launchers
void launch_csv_scan(const uint8_t* buf, uint64_t d0, uint64_t n, int quote, uint32_t* counts, uint64_t* err, uint64_t* total, hipStream_t s) {
  const uint64_t nchunks = (n + kCsvChunk - 1) / kCsvChunk;
  if (!nchunks) return;
  hipLaunchKernelGGL(k_csv_scan<false>, dim3((unsigned)nchunks), dim3(QH_BLOCK), 0, s, (const u8*)buf, (u64)d0, (u64)n, quote, (u32*)counts, (u64*)nullptr,
                     (u64*)err, (u64*)total, 0u);
}
void launch_csv_starts(const uint8_t* buf, uint64_t d0, uint64_t n, const uint32_t* chunk_offsets, uint64_t* starts, bool tail, hipStream_t s) {
  const uint64_t nchunks = (n + kCsvChunk - 1) / kCsvChunk;
  if (!nchunks) return;
  hipLaunchKernelGGL(k_csv_scan<true>, dim3((unsigned)nchunks), dim3(QH_BLOCK), 0, s, (const u8*)buf, (u64)d0, (u64)n, -1, (u32*)chunk_offsets, (u64*)starts,
                     (u64*)nullptr, (u64*)nullptr, tail ? 1u : 0u);
}
void launch_csv_decode(const uint8_t* buf, uint64_t n, const uint64_t* starts, uint64_t nrec, const CsvCols& cols, int ncols, uint32_t nfields, int delim,
                       uint64_t* err, uint64_t* null_counts, uint64_t* utf8_bytes, hipStream_t s) {
  if (!nrec) return;
  CsvColsArg a;
  memcpy(&a, &cols, sizeof a);
  hipLaunchKernelGGL(k_csv_decode<1>, dim3((unsigned)((nrec + QH_BLOCK - 1) / QH_BLOCK)), dim3(QH_BLOCK), 0, s, (const u8*)buf, (u64)n, (const u64*)starts, (u64)nrec,
                     a, ncols, nfields, (u32)delim, (u64*)err, (u64*)null_counts, (u64*)utf8_bytes);
}
void launch_csv_decode_q(const uint8_t* buf, uint64_t n, const uint64_t* starts, uint64_t nrec, const CsvCols& cols, int ncols, uint32_t nfields, int delim,
                         int quote, uint64_t* err, uint64_t* null_counts, uint64_t* utf8_bytes, hipStream_t s) {
  if (!nrec) return;
  CsvColsArg a;
  memcpy(&a, &cols, sizeof a);
  const u32 dq = (u32)delim | ((u32)(quote + 1) << 8);
  hipLaunchKernelGGL(k_csv_decode<2>, dim3((unsigned)((nrec + QH_BLOCK - 1) / QH_BLOCK)), dim3(QH_BLOCK), 0, s, (const u8*)buf, (u64)n, (const u64*)starts, (u64)nrec,
                     a, ncols, nfields, dq, (u64*)err, (u64*)null_counts, (u64*)utf8_bytes);
}
void launch_csv_copy_utf8(const uint8_t* buf, const uint64_t* strpos, const uint32_t* offsets, uint64_t nrows, uint8_t* data, hipStream_t s) {
  if (!nrows) return;
  uint64_t g = ((nrows + 63) / 64 * 64 + QH_BLOCK - 1) / QH_BLOCK;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(k_csv_copy_utf8, dim3((unsigned)g), dim3(QH_BLOCK), 0, s, (const u8*)buf, (const u64*)strpos, (const u32*)offsets, (u64)nrows, (u8*)data);
}
void launch_csv_copy_utf8_q(const uint8_t* buf, const uint64_t* strpos, const uint32_t* offsets, uint64_t nrows, uint8_t* data, int quote, hipStream_t s) {
  if (!nrows) return;
  uint64_t g = ((nrows + 63) / 64 * 64 + QH_BLOCK - 1) / QH_BLOCK;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(k_csv_copy_utf8_q, dim3((unsigned)g), dim3(QH_BLOCK), 0, s, (const u8*)buf, (const u64*)strpos, (const u32*)offsets, (u64)nrows, (u8*)data,
                     (u32)quote);
}

}  // namespace qhip
