// csv.cpp — qhip_table_from_csv: a CSV file's bytes -> an HBM-resident table, decoded on the device.
//
// The reference loads its tables from CSV on the host (datasource/file/csv.rs:33-70) and so did this project (pyarrow, then an
// upload). Here the text itself crosses PCIe once and is decoded where the columns will live; columns that are not projected
// are never parsed. The decoder knows only a strict canonical grammar (device/qhip_csv.inc): whatever lies outside it makes
// the whole call answer QHIP_UNSUPPORTED with nothing created, and the caller takes the host path, which then produces the
// lenient spellings and the error messages itself. The grammar has two levels (qhip_ctx_set_csv_grammar): 1, the default, knows
// no quotes; 2 adds canonical quoted fields, Boolean and Timestamp columns through instantiations of their own of the decode and
// copy kernels, so that level 1 launches exactly what it launched before.
//
// Passes, all on the context's stream:
//   1 upload           the file into one contiguous device buffer (plain asynchronous copies, 64 MB each)
//   2 k_csv_scan       record ends per 16 KB chunk + structural needs-host reasons          -> host wait 1: the record count
//   3 record starts    exclusive scan of the chunk counts, k_csv_scan<true> writes the starts (u64)
//   4 k_csv_decode     one record per lane: values, validity words, Utf8 lengths + positions -> host wait 2: reasons, null
//                      counts, Utf8 byte totals (they size the data buffers)
//   5 Utf8             lengths scanned in place into offsets, k_csv_copy_utf8                (no wait: stream-ordered)
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "kernels.hpp"
#include "device/qhip_csv.inc"

namespace qhip {

static std::string needs_host(unsigned reason, uint64_t record) {
  return std::string("CSV needs the host path: ") + qh_csv_reason_text(reason) + " in record " + std::to_string(record);
}

static bool is_timestamp(const DType& t) { return t.id >= QHIP_TIMESTAMP_S && t.id <= QHIP_TIMESTAMP_NS; }

static bool csv_decodable(const DType& t, int grammar, int float_parse) {
  if (dtype_is_integer(t)) return true;
  if (float_parse >= 2 && t.id == QHIP_FLOAT32) return true;
  if (grammar >= 2 && (t.id == QHIP_BOOL || is_timestamp(t))) return true;   // (a zoned Timestamp never gets here: dtype_from_format refuses it)
  if (t.id == QHIP_DECIMAL128) return t.scale >= 0 && t.precision >= 1 && t.precision <= 38 && t.scale <= 38;
  return t.id == QHIP_FLOAT64 || t.id == QHIP_DATE32 || t.id == QHIP_UTF8;
}

qhip_table* table_from_csv(Ctx* ctx, const ArrowSchema* schema, const uint8_t* bytes, int64_t n_bytes, const qhip_csv_options* opt_in,
                           const int32_t* columns, int32_t n_columns, int64_t batch_rows) {
  if (!schema || !schema->format || strcmp(schema->format, "+s") != 0)
    fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_csv: schema must be a struct ('+s') naming every field of a record");
  const int64_t nfields = schema->n_children;
  if (nfields < 1) fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_csv: the schema has no fields");
  qhip_csv_options opt;
  opt.has_header = 1; opt.delimiter = ','; opt.quote = '"'; opt.escape = -1;
  if (opt_in) opt = *opt_in;
  if (opt.delimiter < 1 || opt.delimiter > 255 || opt.delimiter == '\n' || opt.delimiter == '\r' || opt.delimiter == opt.quote)
    fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_csv: the delimiter must be one byte other than a line end or the quote");
  if (opt.escape >= 0) fail(QHIP_UNSUPPORTED, "CSV needs the host path: an escape character is set");
  if (opt.quote > 255) fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_csv: the quote must be one byte or -1");
  const int quote = opt.quote < 0 ? -1 : opt.quote;
  // grammar level 2: canonical quoted fields are decoded, so the quote byte is no structural reason any more. The byte must be
  // ASCII (dropping one of a doubled pair then leaves a value's UTF-8 validity as it is)
  const int grammar = ctx->csv_grammar;
  if (grammar >= 2 && quote >= 0x80) fail(QHIP_UNSUPPORTED, "CSV needs the host path: the quote is not an ASCII byte");

  // ---- the projection: types are checked before anything is uploaded
  std::vector<int32_t> proj;
  if (columns && n_columns > 0) proj.assign(columns, columns + n_columns);
  else for (int64_t c = 0; c < nfields; ++c) proj.push_back((int32_t)c);
  if ((int)proj.size() > kCsvCols) fail(QHIP_UNSUPPORTED, "CSV needs the host path: more than " + std::to_string(kCsvCols) + " projected columns");
  std::vector<DType> types;
  for (int32_t c : proj) {
    if (c < 0 || c >= nfields) fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_csv: projected column " + std::to_string(c) + " is not in the schema");
    const DType t = dtype_from_format(schema->children[c]->format);   // (unknown formats: QHIP_UNSUPPORTED)
    if (!csv_decodable(t, grammar, ctx->float_parse)) fail(QHIP_UNSUPPORTED, "CSV needs the host path: column type " + dtype_name(t) + " is not decoded on the device");
    types.push_back(t);
  }

  // ---- what the host decides from the file's first bytes
  const uint64_t n = (uint64_t)n_bytes;
  if (n == 0) fail(QHIP_UNSUPPORTED, "CSV needs the host path: the file is empty");
  if (n >= 3 && bytes[0] == 0xEF && bytes[1] == 0xBB && bytes[2] == 0xBF) fail(QHIP_UNSUPPORTED, "CSV needs the host path: the file begins with a byte order mark");
  uint64_t d0 = 0;   // where the data records begin
  if (opt.has_header) {
    const uint8_t* nl = (const uint8_t*)memchr(bytes, '\n', (size_t)n);
    uint64_t hend = nl ? (uint64_t)(nl - bytes) : n;
    d0 = nl ? hend + 1 : n;
    if (hend > 0 && bytes[hend - 1] == '\r') --hend;
    // a name may stand in quotes (Arrow's CSV writer quotes the header even when it quotes no value): "name" is name when
    // there is no further quote inside; anything more involved differs from the schema's name and goes to the host
    uint64_t a = 0;
    int64_t f = 0;
    bool same = true;
    for (;;) {
      uint64_t b = a;
      while (b < hend && bytes[b] != (uint8_t)opt.delimiter) ++b;
      uint64_t na = a, nb = b;
      if (quote >= 0 && nb - na >= 2 && bytes[na] == (uint8_t)quote && bytes[nb - 1] == (uint8_t)quote) { ++na; --nb; }
      const char* want = f < nfields ? schema->children[f]->name : nullptr;
      if (!want || strlen(want) != (size_t)(nb - na) || memcmp(want, bytes + na, (size_t)(nb - na)) != 0 ||
          (quote >= 0 && memchr(bytes + na, quote, (size_t)(nb - na)))) { same = false; break; }
      ++f;
      if (b >= hend) break;
      a = b + 1;
    }
    if (!same || f != nfields) fail(QHIP_UNSUPPORTED, "CSV needs the host path: the header's names differ from the schema's");
  }
  const bool tail = n > d0 && bytes[n - 1] != '\n';   // a last record without a line end counts

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
  for (float& ms : ctx->csv_pass_ms) ms = 0;
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

  uint64_t R = 0;
  if (d0 < n) {
    // ---- 1. upload
    DevBuf file((size_t)n);
    const size_t kPiece = 64u << 20;
    for (uint64_t o = 0; o < n; o += kPiece)
      QHIP_HIP_CHECK(hipMemcpyAsync((uint8_t*)file.ptr + o, bytes + o, (size_t)std::min<uint64_t>(kPiece, n - o), hipMemcpyHostToDevice, ctx->stream));
    mark(1);
    // status words: [0] first offender (position or row << 8 | reason), [1] record ends, [2 .. 2 + 64) null counts, then Utf8 bytes
    std::vector<uint64_t> st_host(2 + 2 * kCsvCols, 0);
    st_host[0] = ~0ULL;
    DevBuf st(st_host.size() * 8);
    QHIP_HIP_CHECK(hipMemcpyAsync(st.ptr, st_host.data(), st.bytes, hipMemcpyHostToDevice, ctx->stream));
    uint64_t* st_dev = st.as<uint64_t>();
    // ---- 2. record ends
    const uint64_t nchunks = (n + kCsvChunk - 1) / kCsvChunk;
    DevBuf counts((size_t)(nchunks + 1) * 4);
    // (level 2: every '\n' still ends a record, a quote is no reason here; a line end inside quotes shows in the decode as a
    // record with an unterminated quote)
    launch_csv_scan(file.as<uint8_t>(), d0, n, grammar >= 2 ? -1 : quote, counts.as<uint32_t>(), st_dev, st_dev + 1, ctx->stream);
    mark(2);
    std::vector<uint64_t> back(st_host.size());
    copy_sync(ctx->stream, back.data(), st.ptr, 16, hipMemcpyDeviceToHost);   // host wait 1 (also: the upload has left `bytes`)
    if (back[0] != ~0ULL) {
      const uint64_t pos = back[0] >> 8;
      const uint64_t rec = (uint64_t)std::count(bytes + d0, bytes + pos, (uint8_t)'\n') + 1;
      fail(QHIP_UNSUPPORTED, needs_host((unsigned)(back[0] & 0xFF), rec));
    }
    R = back[1] + (tail ? 1 : 0);
    if (R >= 0xFFFFFFFFULL) fail(QHIP_UNSUPPORTED, "CSV needs the host path: 2^32 - 1 records or more");
    // ---- 3. record starts
    exclusive_scan_u32(counts.as<uint32_t>(), counts.as<uint32_t>(), nchunks, nullptr, ctx->stream);
    DevBuf starts((size_t)(R + 1) * 8);
    launch_csv_starts(file.as<uint8_t>(), d0, n, counts.as<uint32_t>(), starts.as<uint64_t>(), tail, ctx->stream);
    mark(3);
    // ---- 4. decode
    struct Out { DevColumn col; std::shared_ptr<DevBuf> strpos; };
    std::vector<Out> outs(proj.size());
    std::vector<int> order(proj.size());
    for (size_t k = 0; k < proj.size(); ++k) order[k] = (int)k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return proj[(size_t)a] < proj[(size_t)b]; });   // the kernel walks the fields in order
    CsvCols desc;
    memset(&desc, 0, sizeof desc);
    for (size_t j = 0; j < order.size(); ++j) {
      const size_t k = (size_t)order[j];
      const DType& ty = types[k];
      Out& o = outs[k];
      o.col.type = ty;
      o.col.length = (int64_t)R;
      o.col.validity = std::make_shared<DevBuf>((size_t)((R + 63) / 64) * 8);
      CsvCol& d = desc.c[j];
      d.field = (uint32_t)proj[k];
      d.valid = o.col.validity->as<uint64_t>();
      if (ty.id == QHIP_UTF8) {
        o.col.values = std::make_shared<DevBuf>((size_t)(R + 1) * 4);
        o.strpos = std::make_shared<DevBuf>((size_t)R * 8);
        d.kind = QH_CSV_K_UTF8; d.width = 4;
        d.strpos = o.strpos->as<uint64_t>();
      } else if (ty.id == QHIP_BOOL) {
        o.col.values = std::make_shared<DevBuf>((size_t)((R + 63) / 64) * 8);   // bit-packed; the kernel writes whole 64-row words
        d.kind = QH_CSV_K_BOOL;
      } else {
        const int w = dtype_width(ty);
        o.col.values = std::make_shared<DevBuf>((size_t)R * (size_t)w);
        d.width = (uint8_t)w;
        if (dtype_is_integer(ty)) { d.kind = QH_CSV_K_INT; d.a = dtype_is_signed(ty) ? 1 : 0; }
        else if (ty.id == QHIP_DATE32) d.kind = QH_CSV_K_DATE32;
        else if (ty.id == QHIP_FLOAT64) d.kind = ctx->float_parse >= 2 ? QH_CSV_K_FLOAT64_FULL : QH_CSV_K_FLOAT64;   // (qhip_ctx_set_float_parse)
        else if (ty.id == QHIP_FLOAT32) d.kind = QH_CSV_K_FLOAT32;
        else if (is_timestamp(ty)) { d.kind = QH_CSV_K_TIMESTAMP; d.a = (uint8_t)(3 * (ty.id - QHIP_TIMESTAMP_S)); }
        else { d.kind = QH_CSV_K_DECIMAL128; d.a = (uint8_t)ty.precision; d.b = (uint8_t)ty.scale; }
      }
      d.values = o.col.values->ptr;
    }
    time_mark(ctx, 2);
    if (grammar >= 2)
      launch_csv_decode_q(file.as<uint8_t>(), n, starts.as<uint64_t>(), R, desc, (int)order.size(), (uint32_t)nfields, opt.delimiter, quote, st_dev, st_dev + 2,
                          st_dev + 2 + kCsvCols, ctx->stream);
    else
      launch_csv_decode(file.as<uint8_t>(), n, starts.as<uint64_t>(), R, desc, (int)order.size(), (uint32_t)nfields, opt.delimiter, st_dev, st_dev + 2,
                        st_dev + 2 + kCsvCols, ctx->stream);
    time_mark(ctx, 3);
    mark(4);
    copy_sync(ctx->stream, back.data(), st.ptr, st.bytes, hipMemcpyDeviceToHost);   // host wait 2
    if (back[0] != ~0ULL) fail(QHIP_UNSUPPORTED, needs_host((unsigned)(back[0] & 0xFF), (back[0] >> 8) + 1));
    // ---- 5. Utf8 bytes; null counts
    for (size_t j = 0; j < order.size(); ++j) {
      Out& o = outs[(size_t)order[j]];
      o.col.null_count = (int64_t)back[2 + j];
      if (o.col.null_count == 0) o.col.validity.reset();   // as upload_column: no NULLs, no bitmap
      if (o.col.type.id != QHIP_UTF8) continue;
      const uint64_t total = back[2 + kCsvCols + j];
      if (total > 0x7fffffffULL) fail(QHIP_UNSUPPORTED, "Utf8 column larger than 2 GiB (needs LargeUtf8 offsets)");
      o.col.data = std::make_shared<DevBuf>((size_t)total);
      o.col.data_bytes = (int64_t)total;
      uint32_t* off = o.col.values->as<uint32_t>();
      exclusive_scan_u32(off, off, R, off + R, ctx->stream);
      if (grammar >= 2 && quote >= 0) launch_csv_copy_utf8_q(file.as<uint8_t>(), o.strpos->as<uint64_t>(), off, R, o.col.data->as<uint8_t>(), quote, ctx->stream);
      else launch_csv_copy_utf8(file.as<uint8_t>(), o.strpos->as<uint64_t>(), off, R, o.col.data->as<uint8_t>(), ctx->stream);
    }
    mark(5);
    for (auto& o : outs) t->cols.push_back(std::move(o.col));
    // (the file, the starts and the string positions go back to the pool here: its reuse is ordered on the one stream)
    if (ctx->timing) {
      QHIP_HIP_CHECK(sync_event(ev[5]));
      for (int k = 0; k < 5; ++k) (void)hipEventElapsedTime(&ctx->csv_pass_ms[k], ev[k], ev[k + 1]);
    }
  } else {
    // a header and nothing else: zero rows, zero batches
    for (size_t k = 0; k < proj.size(); ++k) {
      DevColumn col;
      col.type = types[k];
      col.values = std::make_shared<DevBuf>(col.type.id == QHIP_UTF8 ? 4 : 0);   // (Utf8: the one offset of an empty column)
      if (col.type.id == QHIP_UTF8) {
        QHIP_HIP_CHECK(hipMemsetAsync(col.values->ptr, 0, 4, ctx->stream));
        col.data = std::make_shared<DevBuf>(0);
      }
      t->cols.push_back(std::move(col));
    }
    time_mark(ctx, 2);
    time_mark(ctx, 3);
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
  ctx->stats.bytes_per_row_read = R ? (double)(n - d0) / (double)R : 0.0;
  snprintf(ctx->stats.main_kernel_name, sizeof ctx->stats.main_kernel_name, "k_csv_decode");
  return t.release();
}

}  // namespace qhip

using namespace qhip;

extern "C" {

int qhip_table_from_csv(qhip_ctx* ctx, const struct ArrowSchema* schema, const void* bytes, int64_t n_bytes, const qhip_csv_options* options,
                        const int32_t* columns, int32_t n_columns, int64_t batch_rows, qhip_table** out) {
  if (!ctx || !out || n_bytes < 0 || (n_bytes > 0 && !bytes) || n_columns < 0) return QHIP_INVALID_ARGUMENT;
  *out = nullptr;
  return guarded(ctx, [&] { *out = table_from_csv(ctx, schema, (const uint8_t*)bytes, n_bytes, options, columns, n_columns, batch_rows); });
}

int qhip_ctx_csv_pass_ms(const qhip_ctx* ctx, double* out, int32_t n_out) {
  if (!ctx || !out || n_out != 5) return QHIP_INVALID_ARGUMENT;
  for (int k = 0; k < 5; ++k) out[k] = (double)ctx->csv_pass_ms[k];
  return QHIP_OK;
}

}  // extern "C"
