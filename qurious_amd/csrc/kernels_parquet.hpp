// kernels_parquet.hpp — launchers of kernels_parquet.hip (the device Parquet decoder, parquet.cpp). The page, column
// and state descriptors are the ones of device/qhip_parquet.inc; every pointer is device memory, `buf` the uploaded chunks.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

#include "device/qhip_parquet.inc"
#include "device/qhip_delta.inc"
#include "device/qhip_dba.inc"

namespace qhip {

// encoding set 2: the n DELTA_BINARY_PACKED streams of `tab`, one wavefront each. pages / cols / state not NULL: streams of
// pages, behind the level pass (dense values into their slots of the decoded area, DELTA_LENGTH_BYTE_ARRAY lengths into the
// column's entries). pages NULL: raw streams. err / status / ends (each may be NULL): the first offender; per stream its reason
// and the byte position where it ended. kinds: bit 0, the table holds streams for k_pq_delta; bit 1, it holds DELTA_BYTE_ARRAY
// streams (QH_PQ_DS_DBA), which k_pq_delta_dba, a second instance of the body, walks: a kernel is launched where its bit is set.
void launch_pq_delta(uint8_t* buf, const qh_pq_dstream* tab, uint32_t n, const qh_pq_page* pages, const qh_pq_col* cols, const qh_pq_state* state, uint64_t* err,
                     uint32_t* status, uint64_t* ends, uint32_t kinds, hipStream_t s);
// the DELTA_BYTE_ARRAY switch, a Utf8 column with such a page, behind the offsets' scan: row k's suffix, the last
// off[k + 1] - off[k] - prefix[k] bytes of its value, from buf[strpos[k] ..) to data[off[k] + prefix[k] ..) (k_pq_dba_copy:
// k_csv_copy_utf8 with a prefix; a row of another page has prefix 0)
void launch_pq_dba_copy(const uint8_t* buf, const uint64_t* strpos, const uint32_t* offsets, const uint32_t* prefix, uint64_t nrows, uint8_t* data, hipStream_t s);
// the DELTA_BYTE_ARRAY switch: one wavefront per page of `jobs` fills in the prefixes (k_pq_dba_fill). Row space (off not NULL):
// data is a Utf8 column's data behind launch_pq_dba_copy, off its offsets, prefix its per-row prefix lengths, valid its validity
// words or NULL for "every row"; pages, state, err and status are NULL. Value space (off NULL): data is the buffer, a job's
// entries and its dense slot lie in it, the count is state[job.page].nonnull and a set err word ends the wavefront at once; the
// suffixes are copied by the same kernel.
void launch_pq_dba_fill(uint8_t* data, const qh_pq_fill* jobs, uint32_t n, const uint32_t* off, const uint32_t* prefix, const uint64_t* valid, const qh_pq_state* state,
                        const uint64_t* err, hipStream_t s);
// encoding set 2: k_pq_values' body for the pages it leaves alone (RLE Boolean, BYTE_STREAM_SPLIT, DELTA_*)
void launch_pq_values_ext(const uint8_t* buf, const qh_pq_page* pages, uint32_t npages, const qh_pq_col* cols, const qh_pq_state* state, uint64_t* err,
                          uint64_t* utf8_bytes, hipStream_t s);

// format level 2: the n Snappy streams of `tab` (positions in buf, of buf_bytes bytes plus the allocation's slack), one wavefront
// each, unpacked into their slots. err (may be NULL): the smallest (page << 8 | reason), ~0 when none. status (may be NULL):
// per stream 0 or its QH_SNAP_E_* code.
void launch_pq_unsnap(uint8_t* buf, uint64_t buf_bytes, const qh_pq_unpack* tab, uint32_t n, uint64_t* err, uint32_t* status, hipStream_t s);
// codec set 2: one wavefront per ZSTD page of `tab` (k_pq_unzstd); err / status as for launch_pq_unsnap
void launch_pq_unzstd(uint8_t* buf, const qh_pq_unpack* tab, uint32_t n, uint64_t* err, uint32_t* status, hipStream_t s);
// the gzip switch: one wavefront per GZIP page of `tab` (k_pq_ungzip); err / status as for launch_pq_unsnap
void launch_pq_ungzip(uint8_t* buf, const qh_pq_unpack* tab, uint32_t n, uint64_t* err, uint32_t* status, hipStream_t s);
// the lz4 switch: one wavefront per bare LZ4 block of `tab` (k_pq_unlz4); err / status as for launch_pq_unsnap
void launch_pq_unlz4(uint8_t* buf, const qh_pq_unpack* tab, uint32_t n, uint64_t* err, uint32_t* status, hipStream_t s);
// definition levels -> validity words (zeroed before), per page its non-NULL count and where its values begin, per column its
// NULL count. err: the smallest (page << 8 | reason), ~0 when none.
void launch_pq_levels(const uint8_t* buf, const qh_pq_page* pages, uint32_t npages, const qh_pq_col* cols, qh_pq_state* state, uint64_t* err, uint64_t* null_counts,
                      hipStream_t s);
// the BYTE_ARRAY length chains of the Utf8 columns' dictionary pages and PLAIN data pages -> (length, position) entries
void launch_pq_strings(const uint8_t* buf, uint64_t buf_bytes, const qh_pq_page* pages, uint32_t npages, const qh_pq_col* cols, const qh_pq_state* state, uint64_t* err,
                       hipStream_t s);
// values: bit-unpack, dictionary gather, scatter over NULLs; Utf8 rows get (length, position) and the column its byte total
void launch_pq_values(const uint8_t* buf, const qh_pq_page* pages, uint32_t npages, const qh_pq_col* cols, const qh_pq_state* state, uint64_t* err, uint64_t* utf8_bytes,
                      hipStream_t s);

}  // namespace qhip
