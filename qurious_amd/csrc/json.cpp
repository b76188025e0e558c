// json.cpp — qhip_table_from_json: the bytes of a newline-delimited JSON file -> an HBM-resident table, decoded on the device
// (DESIGN §3.10).
//
// The reference loads JSON on the host (datasource/file/json.rs) and so did this project (pyarrow, then an upload). Here the text
// crosses PCIe once and is decoded where the columns will live. The decoder knows only a strict grammar (device/qhip_json.inc):
// whatever lies outside it makes the whole call answer QHIP_UNSUPPORTED with nothing created, and the caller takes the host
// path, which then produces the lenient readings and the error messages itself. Every value of every record is validated,
// projected or not — the host refuses a file for a bad value in any column — so a projection saves the stores, the string copies
// and the output memory, not the walk.
//
// Passes, all on the context's stream:
//   1 upload           the file into one contiguous device buffer (plain asynchronous copies, 64 MB each)
//   2 k_csv_scan       (as it is, no quote byte) record ends per 16 KB chunk + structural reasons   -> host wait 1: the record count
//   3 record starts    exclusive scan of the chunk counts, k_csv_scan<true> writes the starts (u64)
//   4 k_json_decode    one record per lane: values, validity words, Utf8 lengths + positions        -> host wait 2: reasons, null
//                      counts, Utf8 byte totals (they size the data buffers)
//   5 Utf8             lengths scanned in place into offsets, k_json_copy_utf8 removes the escapes  (no wait: stream-ordered)
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "kernels.hpp"
#include "device/qhip_json.inc"

namespace qhip {

static std::string json_needs_host(unsigned reason, uint64_t record) {
  return std::string("JSON needs the host path: ") + qh_json_reason_text(reason) + " in record " + std::to_string(record);
}

static bool json_is_timestamp(const DType& t) { return t.id >= QHIP_TIMESTAMP_S && t.id <= QHIP_TIMESTAMP_NS; }

static bool json_decodable(const DType& t, int float_parse) {
  if (float_parse >= 2 && t.id == QHIP_FLOAT32) return true;
  if (dtype_is_integer(t) || t.id == QHIP_BOOL || json_is_timestamp(t)) return true;   // (a zoned Timestamp never gets here: dtype_from_format refuses it)
  if (t.id == QHIP_DECIMAL128) return t.scale >= 0 && t.precision >= 1 && t.precision <= 38 && t.scale <= 38;
  return t.id == QHIP_FLOAT64 || t.id == QHIP_DATE32 || t.id == QHIP_UTF8;
}

qhip_table* table_from_json(Ctx* ctx, const ArrowSchema* schema, const uint8_t* bytes, int64_t n_bytes, const int32_t* columns, int32_t n_columns,
                            int64_t batch_rows) {
  if (!schema || !schema->format || strcmp(schema->format, "+s") != 0)
    fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_json: schema must be a struct ('+s') naming every key of a record");
  const int64_t nfields = schema->n_children;
  if (nfields < 1) fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_json: the schema has no fields");
  if (nfields > kJsonFields) fail(QHIP_UNSUPPORTED, "JSON needs the host path: more than " + std::to_string(kJsonFields) + " schema fields");

  // ---- the schema and the projection: every field's type is checked, projected or not, before anything is uploaded
  JsonDesc desc;
  memset(&desc, 0, sizeof desc);
  std::vector<DType> ftypes;
  size_t name_bytes = 0;
  for (int64_t f = 0; f < nfields; ++f) {
    const ArrowSchema* cs = schema->children[f];
    const DType t = dtype_from_format(cs->format);   // (unknown formats, the null type among them: QHIP_UNSUPPORTED)
    if (!json_decodable(t, ctx->float_parse)) fail(QHIP_UNSUPPORTED, "JSON needs the host path: column type " + dtype_name(t) + " is not decoded on the device");
    // (the host refuses a record in which a required field is absent or null; here a missing key and null are simply NULL)
    if (!(cs->flags & ARROW_FLAG_NULLABLE)) fail(QHIP_UNSUPPORTED, std::string("JSON needs the host path: schema field '") + (cs->name ? cs->name : "") + "' is not nullable");
    ftypes.push_back(t);
    const char* name = cs->name ? cs->name : "";
    const size_t nl = strlen(name);
    if (name_bytes + nl > (size_t)kJsonNameBytes) fail(QHIP_UNSUPPORTED, "JSON needs the host path: key names over " + std::to_string(kJsonNameBytes) + " bytes in total");
    for (int64_t g = 0; g < f; ++g)
      if (strcmp(name, schema->children[g]->name ? schema->children[g]->name : "") == 0) fail(QHIP_UNSUPPORTED, "JSON needs the host path: two schema fields of one name");
    JsonField& d = desc.field[f];
    d.name_off = (uint16_t)name_bytes;
    d.name_len = (uint16_t)nl;
    memcpy(desc.names + name_bytes, name, nl);
    name_bytes += nl;
    d.col = -1;
    if (t.id == QHIP_UTF8) d.kind = QH_CSV_K_UTF8;
    else if (t.id == QHIP_BOOL) d.kind = QH_CSV_K_BOOL;
    else if (dtype_is_integer(t)) { d.kind = QH_CSV_K_INT; d.a = dtype_is_signed(t) ? 1 : 0; d.b = (uint8_t)dtype_width(t); }
    else if (t.id == QHIP_DATE32) d.kind = QH_CSV_K_DATE32;
    else if (t.id == QHIP_FLOAT64) d.kind = ctx->float_parse >= 2 ? QH_CSV_K_FLOAT64_FULL : QH_CSV_K_FLOAT64;   // (qhip_ctx_set_float_parse)
    else if (t.id == QHIP_FLOAT32) d.kind = QH_CSV_K_FLOAT32;
    else if (json_is_timestamp(t)) { d.kind = QH_CSV_K_TIMESTAMP; d.a = (uint8_t)(3 * (t.id - QHIP_TIMESTAMP_S)); }
    else { d.kind = QH_CSV_K_DECIMAL128; d.a = (uint8_t)t.precision; d.b = (uint8_t)t.scale; }
  }
  std::vector<int32_t> proj;
  if (columns && n_columns > 0) proj.assign(columns, columns + n_columns);
  else for (int64_t c = 0; c < nfields; ++c) proj.push_back((int32_t)c);
  for (size_t k = 0; k < proj.size(); ++k) {
    const int32_t c = proj[k];
    if (c < 0 || c >= nfields) fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_json: projected column " + std::to_string(c) + " is not in the schema");
    if (desc.field[c].col >= 0) fail(QHIP_UNSUPPORTED, "JSON needs the host path: a field is projected twice");
    desc.field[c].col = (int8_t)k;
  }

  // ---- what the host decides from the file's first bytes
  const uint64_t n = (uint64_t)n_bytes;
  if (n == 0) fail(QHIP_UNSUPPORTED, "JSON needs the host path: the file is empty");
  if (n >= 3 && bytes[0] == 0xEF && bytes[1] == 0xBB && bytes[2] == 0xBF) fail(QHIP_UNSUPPORTED, "JSON needs the host path: the file begins with a byte order mark");
  const bool tail = bytes[n - 1] != '\n';   // a last record without a line end counts

  std::unique_ptr<qhip_table> t(new qhip_table());
  t->ctx = ctx;
  for (size_t k = 0; k < proj.size(); ++k) {
    const ArrowSchema* cs = schema->children[proj[k]];
    t->names.push_back(cs->name ? cs->name : "");
    t->nullable.push_back((cs->flags & ARROW_FLAG_NULLABLE) != 0);
  }
  QHIP_HIP_CHECK(hipSetDevice(ctx->device));
  memset(&ctx->stats, 0, sizeof(ctx->stats));
  ctx->stats_timing_pending = 0;
  ctx->wide_join_stage_ms = 0;
  for (float& ms : ctx->json_pass_ms) ms = 0;
  // (events of this call alone: the context's own five mark other things)
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int k = 0; k < 6; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
  auto mark = [&](int k) {
    if (!ctx->timing) return;
    if (!ev[k]) QHIP_HIP_CHECK(hipEventCreate(&ev[k]));
    QHIP_HIP_CHECK(hipEventRecord(ev[k], ctx->stream));
  };
  time_mark(ctx, 0);
  mark(0);

  // ---- 1. upload
  DevBuf file((size_t)n);
  const size_t kPiece = 64u << 20;
  for (uint64_t o = 0; o < n; o += kPiece)
    QHIP_HIP_CHECK(hipMemcpyAsync((uint8_t*)file.ptr + o, bytes + o, (size_t)std::min<uint64_t>(kPiece, n - o), hipMemcpyHostToDevice, ctx->stream));
  mark(1);
  // status words: [0] first offender (position or row << 8 | reason), [1] record ends, [2 .. 2 + 64) null counts, then Utf8 bytes
  std::vector<uint64_t> st_host(2 + 2 * kJsonFields, 0);
  st_host[0] = ~0ULL;
  DevBuf st(st_host.size() * 8);
  QHIP_HIP_CHECK(hipMemcpyAsync(st.ptr, st_host.data(), st.bytes, hipMemcpyHostToDevice, ctx->stream));
  uint64_t* st_dev = st.as<uint64_t>();
  // ---- 2. record ends: every '\n' ends a record; a line end inside a string shows in the decode as a cut record
  const uint64_t nchunks = (n + kCsvChunk - 1) / kCsvChunk;
  DevBuf counts((size_t)(nchunks + 1) * 4);
  launch_csv_scan(file.as<uint8_t>(), 0, n, -1, counts.as<uint32_t>(), st_dev, st_dev + 1, ctx->stream);
  mark(2);
  std::vector<uint64_t> back(st_host.size());
  copy_sync(ctx->stream, back.data(), st.ptr, 16, hipMemcpyDeviceToHost);   // host wait 1 (also: the upload has left `bytes`)
  if (back[0] != ~0ULL) {
    const uint64_t pos = back[0] >> 8;
    const uint64_t rec = (uint64_t)std::count(bytes, bytes + pos, (uint8_t)'\n') + 1;
    fail(QHIP_UNSUPPORTED, json_needs_host((unsigned)(back[0] & 0xFF), rec));
  }
  const uint64_t R = back[1] + (tail ? 1 : 0);
  if (R >= 0xFFFFFFFFULL) fail(QHIP_UNSUPPORTED, "JSON needs the host path: 2^32 - 1 records or more");
  // ---- 3. record starts
  exclusive_scan_u32(counts.as<uint32_t>(), counts.as<uint32_t>(), nchunks, nullptr, ctx->stream);
  DevBuf starts((size_t)(R + 1) * 8);
  launch_csv_starts(file.as<uint8_t>(), 0, n, counts.as<uint32_t>(), starts.as<uint64_t>(), tail, ctx->stream);
  mark(3);
  // ---- 4. decode
  struct Out { DevColumn col; std::shared_ptr<DevBuf> strpos; };
  std::vector<Out> outs(proj.size());
  for (size_t k = 0; k < proj.size(); ++k) {
    const DType& ty = ftypes[(size_t)proj[k]];
    Out& o = outs[k];
    o.col.type = ty;
    o.col.length = (int64_t)R;
    o.col.validity = std::make_shared<DevBuf>((size_t)((R + 63) / 64) * 8);
    JsonOut& d = desc.out[k];
    d.valid = o.col.validity->as<uint64_t>();
    if (ty.id == QHIP_UTF8) {
      o.col.values = std::make_shared<DevBuf>((size_t)(R + 1) * 4);
      o.strpos = std::make_shared<DevBuf>((size_t)R * 8);
      d.strpos = o.strpos->as<uint64_t>();
    } else if (ty.id == QHIP_BOOL) {
      o.col.values = std::make_shared<DevBuf>((size_t)((R + 63) / 64) * 8);   // bit-packed; the kernel writes whole 64-row words
    } else {
      o.col.values = std::make_shared<DevBuf>((size_t)R * (size_t)dtype_width(ty));
    }
    d.values = o.col.values->ptr;
  }
  time_mark(ctx, 2);
  launch_json_decode(file.as<uint8_t>(), n, starts.as<uint64_t>(), R, desc, (uint32_t)nfields, st_dev, ctx->stream);
  time_mark(ctx, 3);
  mark(4);
  copy_sync(ctx->stream, back.data(), st.ptr, st.bytes, hipMemcpyDeviceToHost);   // host wait 2
  if (back[0] != ~0ULL) fail(QHIP_UNSUPPORTED, json_needs_host((unsigned)(back[0] & 0xFF), (back[0] >> 8) + 1));
  // ---- 5. Utf8 bytes; null counts
  for (size_t k = 0; k < outs.size(); ++k) {
    Out& o = outs[k];
    o.col.null_count = (int64_t)back[2 + k];
    if (o.col.null_count == 0) o.col.validity.reset();   // as upload_column: no NULLs, no bitmap
    if (o.col.type.id != QHIP_UTF8) continue;
    const uint64_t total = back[2 + kJsonFields + k];
    if (total > 0x7fffffffULL) fail(QHIP_UNSUPPORTED, "JSON needs the host path: a Utf8 column of 2 GiB or more");
    o.col.data = std::make_shared<DevBuf>((size_t)total);
    o.col.data_bytes = (int64_t)total;
    uint32_t* off = o.col.values->as<uint32_t>();
    exclusive_scan_u32(off, off, R, off + R, ctx->stream);
    launch_json_copy_utf8(file.as<uint8_t>(), o.strpos->as<uint64_t>(), off, R, o.col.data->as<uint8_t>(), ctx->stream);
  }
  mark(5);
  for (auto& o : outs) t->cols.push_back(std::move(o.col));
  // (the file, the starts and the string positions go back to the pool here: its reuse is ordered on the one stream)
  if (ctx->timing) {
    QHIP_HIP_CHECK(sync_event(ev[5]));
    for (int k = 0; k < 5; ++k) (void)hipEventElapsedTime(&ctx->json_pass_ms[k], ev[k], ev[k + 1]);
  }
  time_mark(ctx, 1);
  t->num_rows = (int64_t)R;
  t->batch_offsets.push_back(0);
  if (R > 0) {
    const uint64_t step = batch_rows > 0 ? (uint64_t)batch_rows : R;
    for (uint64_t r = step; r < R; r += step) t->batch_offsets.push_back((int64_t)r);
    t->batch_offsets.push_back((int64_t)R);
  }
  ctx->stats_timing_pending = ctx->timing ? 2 : 0;
  ctx->stats.rows_in = (int64_t)R;
  ctx->stats.rows_out = (int64_t)R;
  ctx->stats.bytes_per_row_read = R ? (double)n / (double)R : 0.0;
  snprintf(ctx->stats.main_kernel_name, sizeof ctx->stats.main_kernel_name, "k_json_decode");
  return t.release();
}

}  // namespace qhip

using namespace qhip;

extern "C" {

int qhip_table_from_json(qhip_ctx* ctx, const struct ArrowSchema* schema, const void* bytes, int64_t n_bytes, const int32_t* columns, int32_t n_columns,
                         int64_t batch_rows, qhip_table** out) {
  if (!ctx || !out || n_bytes < 0 || (n_bytes > 0 && !bytes) || n_columns < 0) return QHIP_INVALID_ARGUMENT;
  *out = nullptr;
  return guarded(ctx, [&] { *out = table_from_json(ctx, schema, (const uint8_t*)bytes, n_bytes, columns, n_columns, batch_rows); });
}

int qhip_ctx_json_pass_ms(const qhip_ctx* ctx, double* out, int32_t n_out) {
  if (!ctx || !out || n_out != 5) return QHIP_INVALID_ARGUMENT;
  for (int k = 0; k < 5; ++k) out[k] = (double)ctx->json_pass_ms[k];
  return QHIP_OK;
}

}  // extern "C"
