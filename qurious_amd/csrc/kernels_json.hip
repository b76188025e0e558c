// kernels_json.hip — newline-delimited JSON text in HBM -> typed Arrow columns (gfx950, wave64), compiled ahead of time. The host
// side is json.cpp (qhip_table_from_json); the per-record code is device/qhip_json.inc, shared with the CPU tests. Replaces the
// reference's host JSON reader (datasource/file/json.rs) for files inside the strict grammar of DESIGN §3.10.
//
//   k_csv_scan<false / true>  (kernels_csv.hip, as it is, with no quote byte) record ends, structural reasons; record starts
//   k_json_decode             one record per lane, 256 consecutive records per workgroup, their bytes staged in LDS
//   k_json_copy_utf8          string bytes from the file into the column's data buffer, backslash escapes removed
//
// Every byte offset into the file is 64 bits wide. Vector loads may read up to 15 bytes past the file's end, the copy's last step
// up to 63: every device allocation carries 64 bytes of slack (DevBuf::alloc), and what is read there is never looked at.
#include <hip/hip_runtime.h>
#include <cstring>

#include "device/qhip_status.h"
#include "device/qhip_device.hpp"
#include "device/qhip_json.inc"
#include "common.hpp"
#include "kernels.hpp"

namespace qhip {

static_assert(sizeof(JsonDesc) == sizeof(qh_json_desc) && kJsonFields == QH_JSON_MAX_FIELDS && kJsonNameBytes == QH_JSON_MAX_NAME_BYTES,
              "host and device descriptors of a JSON file differ");
static_assert(sizeof(qh_json_desc) + 64 <= 4096, "the decode kernel's arguments stay below 4 KB");
struct JsonDescArg { qh_json_desc d; };

typedef u32 json_v4u __attribute__((ext_vector_type(4)));

// the smallest (record << 8 | reason) wins, as csv_report
__device__ __forceinline__ void json_report(u64* err, u64 where, u32 reason) {
  const u64 mine = (where << 8) | reason;
  if (mine < __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(err, mine);
}

// The shape of k_csv_decode: one record per lane, a workgroup on 256 consecutive records — one contiguous byte range of the
// file, staged into LDS with coalesced 16-byte loads — a wavefront on 64, so that a column's validity word (and a Boolean
// column's values word) of 64 rows is one ballot. A range that does not fit the tile (one very long string) is walked in global
// memory through the same generic pointers. st: [0] the first offender, [2 + c] NULL count and [2 + 64 + c] Utf8 byte total
// of output column c (json.cpp's status words).
constexpr u32 kJsonLdsBytes = 48 * 1024;
__global__ __launch_bounds__(QH_BLOCK) void k_json_decode(const u8* __restrict__ buf, u64 n, const u64* __restrict__ starts, u64 nrec, JsonDescArg arg,
                                                          u32 nfields, u64* st) {
  __shared__ __attribute__((aligned(16))) u8 tile[kJsonLdsBytes];
  const u64 r0 = (u64)blockIdx.x * QH_BLOCK;
  const u64 r1 = r0 + QH_BLOCK < nrec ? r0 + QH_BLOCK : nrec;
  const u64 t_begin = starts[r0];
  u64 t_end = starts[r1];
  if (t_end > n) t_end = n;                    // (the virtual line end behind a last record without one)
  const u64 base = t_begin & ~(u64)15;
  const u64 span = t_end - base;
  const bool staged = span <= kJsonLdsBytes;    // workgroup-uniform
  if (staged) {
    // (the last vector may reach up to 15 bytes past t_end <= n: inside the slack behind the file's allocation)
    for (u64 o = (u64)threadIdx.x * 16; o < span; o += (u64)QH_BLOCK * 16) *(json_v4u*)(tile + o) = *(const json_v4u*)(buf + base + o);
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
    const int reason = qh_json_decode_record(arg.d, nfields, p, len, row, s, &vm, &tm);
    if (reason != QH_CSV_OK) json_report(st, row, (u32)reason);
  }
  const u64 live = qh_ballot(active);
  const int lane = qh_lane();
  for (u32 f = 0; f < nfields; ++f) {
    const int c = arg.d.field[f].col;           // (uniform)
    if (c < 0) continue;
    const u32 kind = arg.d.field[f].kind;
    const u64 word = qh_ballot(active && ((vm >> c) & 1ULL));
    if (kind == QH_CSV_K_BOOL) {
      const u64 truth = qh_ballot(active && ((tm >> c) & 1ULL));   // (a NULL row's bit is 0)
      if (lane == 0 && live) ((u64*)arg.d.out[c].values)[row >> 6] = truth;
    }
    u64 bytes = 0;
    // (a row that got a value has stored its length; a NULL row's is 0, and a lane whose walk failed may have stored nothing)
    if (kind == QH_CSV_K_UTF8) bytes = qh_wave_sum_u64(active && ((vm >> c) & 1ULL) ? (u64)((const u32*)arg.d.out[c].values)[row] : 0ULL);
    if (lane == 0 && live) {
      arg.d.out[c].valid[row >> 6] = word;
      const u32 nulls = (u32)(__builtin_popcountll(live) - __builtin_popcountll(word));
      if (nulls) atomicAdd(&st[2 + c], (u64)nulls);
      if (bytes) atomicAdd(&st[2 + QH_JSON_MAX_FIELDS + c], bytes);
    }
  }
}

// Row k's bytes: file[strpos[k] ..) -> data[off[k] .. off[k + 1]). One wavefront per 64 rows. A row without QH_JSON_POS_ESC is
// copied exactly as k_csv_copy_utf8 copies it (up to 64 bytes by its own lane, longer ones by the whole wavefront). A marked
// row (its length in `off` is the UNESCAPED one) of up to 64 raw bytes is unescaped by its own lane; a longer one
// (QH_JSON_POS_LONG) by the whole wavefront, 64 raw bytes per step: from the ballot of "my byte is a backslash" every lane knows
// whether its byte introduces an escape (dropped), stands behind an introducer (translated) and where the bytes below it go
// (qh_json_unescape_*; runs of backslashes cross the steps, their parity is carried). No lane walks a long value byte by byte.
// The last step may read up to 63 bytes behind the value's closing quote: inside the file or the slack behind its allocation,
// and never written (their output position is at or behind the row's end).
__global__ __launch_bounds__(QH_BLOCK) void k_json_copy_utf8(const u8* __restrict__ buf, const u64* __restrict__ strpos, const u32* __restrict__ off, u64 nrows,
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
    const bool esc = (src & QH_JSON_POS_ESC) != 0, wide = (src & QH_JSON_POS_LONG) != 0;
    src &= QH_JSON_POS_MASK;
    if (!esc) {
      if (len <= 64) for (u32 b = 0; b < len; ++b) data[dst + b] = buf[src + b];
    } else if (!wide) {
      u64 q = src;   // (at most 64 raw bytes)
      for (u32 b = 0; b < len; ++b) {
        u8 c = buf[q++];
        if (c == '\\') c = qh_json_unescape_byte(buf[q++]);
        data[dst + b] = c;
      }
    }
    u64 big = qh_ballot(!esc && len > 64);
    while (big) {
      const int l = __builtin_ctzll(big);
      big &= big - 1;
      const u64 s2 = qh_readlane64(src, l);
      const u32 d2 = qh_readlane32(dst, l), n2 = qh_readlane32(len, l);
      for (u32 b = lane; b < n2; b += 64) data[d2 + b] = buf[s2 + b];
    }
    big = qh_ballot(esc && wide);
    while (big) {
      const int l = __builtin_ctzll(big);
      big &= big - 1;
      const u64 s2 = qh_readlane64(src, l);
      const u32 d2 = qh_readlane32(dst, l), n2 = qh_readlane32(len, l);
      u64 emitted = 0;
      u32 carry = 0;
      for (u64 raw = 0; emitted < n2; raw += 64) {   // (every step emits at least 32 bytes)
        const u8 c = buf[s2 + raw + lane];
        const u64 slashes = qh_ballot(c == '\\');
        const bool drop = qh_json_unescape_drops(slashes, carry, lane);
        const u64 dropped = qh_ballot(drop);
        const u64 o = qh_csv_undouble_out(emitted, dropped, lane);
        if (!drop && o < n2) data[d2 + o] = qh_json_unescape_escaped(dropped, carry, lane) ? qh_json_unescape_byte(c) : c;
        emitted += (u64)__builtin_popcountll(~dropped);
        carry = qh_csv_undouble_carry(slashes, carry);
      }
    }
  }
}

// ---------------------------------------------------------------- launchers
void launch_json_decode(const uint8_t* buf, uint64_t n, const uint64_t* starts, uint64_t nrec, const JsonDesc& desc, uint32_t nfields, uint64_t* status,
                        hipStream_t s) {
  if (!nrec) return;
  JsonDescArg a;
  memcpy(&a, &desc, sizeof a);
  hipLaunchKernelGGL(k_json_decode, dim3((unsigned)((nrec + QH_BLOCK - 1) / QH_BLOCK)), dim3(QH_BLOCK), 0, s, (const u8*)buf, (u64)n, (const u64*)starts, (u64)nrec, a,
                     nfields, (u64*)status);
}
void launch_json_copy_utf8(const uint8_t* buf, const uint64_t* strpos, const uint32_t* offsets, uint64_t nrows, uint8_t* data, hipStream_t s) {
  if (!nrows) return;
  uint64_t g = ((nrows + 63) / 64 * 64 + QH_BLOCK - 1) / QH_BLOCK;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(k_json_copy_utf8, dim3((unsigned)g), dim3(QH_BLOCK), 0, s, (const u8*)buf, (const u64*)strpos, (const u32*)offsets, (u64)nrows, (u8*)data);
}

}  // namespace qhip
