// parquet.cpp — qhip_table_from_parquet: a Parquet file's bytes -> an HBM-resident table, decoded on the device.
//
// The reference reads Parquet on the host (datasource/file/parquet.rs) and so did this project (pyarrow, then an upload of the
// decoded columns). Here the host reads the footer and one header per page of the projected chunks (parquet_meta.hpp: a Thrift
// compact reader and the page walk, plain C++), uploads the bytes of those chunks alone — an unprojected column never crosses
// PCIe — and the device turns pages into columns. Format level 1: uncompressed chunks, data pages V1, PLAIN and dictionary
// encodings, RLE definition levels, flat columns. Whatever lies outside makes the whole call answer QHIP_UNSUPPORTED with nothing
// created, and the caller takes the host path, which then produces every error message.
//
// Passes, all on the context's stream:
//   1 upload        the projected chunks, one behind the other, into one device buffer; the page table and column descriptors
//   2 k_pq_levels   definition levels -> validity words, non-NULL count per page, NULL count per column
//   3 k_pq_strings  Utf8: the length chains of dictionary pages and PLAIN data pages -> (length, position) entries
//   4 k_pq_values   values: bit-unpack, dictionary gather, scatter over NULLs; Utf8 rows get (length, position)
//                   -> the ONE host wait: first offender, NULL counts, Utf8 byte totals (they size the data buffers)
//   5 Utf8          lengths scanned in place into offsets, k_csv_copy_utf8 moves the bytes (no wait: stream-ordered)
#include <hip/hip_runtime_api.h>
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "kernels_parquet.hpp"
#include "parquet_meta.hpp"

namespace qhip {

static_assert(sizeof(qh_pq_page) == 56 && sizeof(qh_pq_col) == 48 && sizeof(qh_pq_ent) == 16, "the Parquet descriptors have the layout both compilers agree on");

qhip_table* table_from_parquet(Ctx* ctx, const ArrowSchema* schema, const uint8_t* bytes, int64_t n_bytes, const int32_t* columns, int32_t n_columns,
                               int64_t batch_rows) {
  if (!schema || !schema->format || strcmp(schema->format, "+s") != 0)
    fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_parquet: schema must be a struct ('+s') naming every field of the file");
  const int64_t nfields = schema->n_children;
  if (nfields < 1) fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_parquet: the schema has no fields");

  // ---- the Arrow types: one the C ABI does not carry (a zoned Timestamp, LargeUtf8, a dictionary, a list ...) is no error
  // here, it needs the host when it is projected
  std::vector<qhip_pq::ArrowType> types((size_t)nfields);
  std::vector<std::string> names((size_t)nfields);
  std::vector<DType> dtypes((size_t)nfields);
  for (int64_t c = 0; c < nfields; ++c) {
    const ArrowSchema* cs = schema->children[c];
    names[(size_t)c] = cs->name ? cs->name : "";
    if (cs->dictionary || cs->n_children > 0) continue;
    try {
      const DType t = dtype_from_format(cs->format);
      dtypes[(size_t)c] = t;
      types[(size_t)c].id = t.id; types[(size_t)c].precision = t.precision; types[(size_t)c].scale = t.scale;
    } catch (const Error& e) {
      if (e.code != QHIP_UNSUPPORTED) throw;
    }
  }
  std::vector<int32_t> proj;
  if (columns && n_columns > 0) proj.assign(columns, columns + n_columns);
  else for (int64_t c = 0; c < nfields; ++c) proj.push_back((int32_t)c);
  for (int32_t c : proj)
    if (c < 0 || c >= nfields) fail(QHIP_INVALID_ARGUMENT, "qhip_table_from_parquet: projected column " + std::to_string(c) + " is not in the schema");

  // ---- footer and page walk (host, one header per page)
  qhip_pq::Plan plan;
  try {
    plan = qhip_pq::plan_file(bytes, (uint64_t)n_bytes, &names, types, proj);
  } catch (const qhip_pq::PqNeedsHost& e) {
    fail(QHIP_UNSUPPORTED, qhip_pq::needs_host_text(e));
  }
  const uint64_t R = plan.num_rows;
  const uint32_t npages = (uint32_t)plan.pages.size();
  const size_t ncols = proj.size();

  std::unique_ptr<qhip_table> t(new qhip_table());
  t->ctx = ctx;
  for (size_t k = 0; k < ncols; ++k) {
    const ArrowSchema* cs = schema->children[proj[k]];
    t->names.push_back(names[(size_t)proj[k]]);
    t->nullable.push_back((cs->flags & ARROW_FLAG_NULLABLE) != 0);
  }
  QHIP_HIP_CHECK(hipSetDevice(ctx->device));
  memset(&ctx->stats, 0, sizeof(ctx->stats));
  ctx->stats_timing_pending = 0;
  ctx->wide_join_stage_ms = 0;
  for (float& ms : ctx->parquet_pass_ms) ms = 0;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int k = 0; k < 6; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
  auto mark = [&](int k) {
    if (!ctx->timing) return;
    if (!ev[k]) QHIP_HIP_CHECK(hipEventCreate(&ev[k]));
    QHIP_HIP_CHECK(hipEventRecord(ev[k], ctx->stream));
  };
  time_mark(ctx, 0);
  mark(0);

  // ---- 1. upload: the projected chunks only (the buffer keeps the 64 bytes of slack DevBuf::alloc gives)
  DevBuf file((size_t)plan.upload_bytes);
  const size_t kPiece = 64u << 20;
  for (const qhip_pq::Range& r : plan.ranges)
    for (uint64_t o = 0; o < r.bytes; o += kPiece)
      QHIP_HIP_CHECK(hipMemcpyAsync((uint8_t*)file.ptr + r.buf_off + o, bytes + r.file_off + o, (size_t)std::min<uint64_t>(kPiece, r.bytes - o), hipMemcpyHostToDevice,
                                    ctx->stream));
  DevBuf pages_d((size_t)npages * sizeof(qh_pq_page)), state_d((size_t)npages * sizeof(qh_pq_state)), cols_d(ncols * sizeof(qh_pq_col));
  QHIP_HIP_CHECK(hipMemcpyAsync(pages_d.ptr, plan.pages.data(), (size_t)npages * sizeof(qh_pq_page), hipMemcpyHostToDevice, ctx->stream));
  // status words: [0] first offender (page << 8 | reason), [1 .. 1 + 64) NULL counts, then Utf8 byte totals
  std::vector<uint64_t> st_host(1 + 2 * QH_PQ_MAX_COLS, 0);
  st_host[0] = ~0ULL;
  DevBuf st(st_host.size() * 8);
  QHIP_HIP_CHECK(hipMemcpyAsync(st.ptr, st_host.data(), st.bytes, hipMemcpyHostToDevice, ctx->stream));
  uint64_t* st_dev = st.as<uint64_t>();

  struct Out { DevColumn col; std::shared_ptr<DevBuf> strpos, ent; };
  std::vector<Out> outs(ncols);
  std::vector<qh_pq_col> desc(ncols);
  const size_t words = (size_t)((R + 63) / 64);
  for (size_t k = 0; k < ncols; ++k) {
    const qhip_pq::ColPlan& cp = plan.cols[k];
    Out& o = outs[k];
    qh_pq_col& d = desc[k];
    memset(&d, 0, sizeof d);
    o.col.type = dtypes[(size_t)proj[k]];
    o.col.length = (int64_t)R;
    if (cp.optional) {
      o.col.validity = std::make_shared<DevBuf>(words * 8);
      QHIP_HIP_CHECK(hipMemsetAsync(o.col.validity->ptr, 0, words * 8, ctx->stream));   // (shared words are OR-ed in)
      d.valid = o.col.validity->as<pq_u64>();
    }
    if (cp.utf8) {
      o.col.values = std::make_shared<DevBuf>((size_t)(R + 1) * 4);
      o.strpos = std::make_shared<DevBuf>((size_t)R * 8);
      o.ent = std::make_shared<DevBuf>((size_t)(R + cp.dict_entries) * sizeof(qh_pq_ent));
      d.strpos = o.strpos->as<pq_u64>();
      d.ent = o.ent->as<qh_pq_ent>();
    } else if (cp.boolean) {
      o.col.values = std::make_shared<DevBuf>(words * 8);   // bit-packed, whole 64-row words
      QHIP_HIP_CHECK(hipMemsetAsync(o.col.values->ptr, 0, words * 8, ctx->stream));
    } else {
      o.col.values = std::make_shared<DevBuf>((size_t)R * cp.width);
    }
    d.values = o.col.values->ptr;
    d.phys = cp.phys; d.flba = cp.flba; d.width = cp.width; d.narrow = cp.narrow;
  }
  QHIP_HIP_CHECK(hipMemcpyAsync(cols_d.ptr, desc.data(), ncols * sizeof(qh_pq_col), hipMemcpyHostToDevice, ctx->stream));
  mark(1);

  // ---- 2 .. 4: levels, string walk, values
  time_mark(ctx, 2);
  launch_pq_levels(file.as<uint8_t>(), pages_d.as<qh_pq_page>(), npages, cols_d.as<qh_pq_col>(), state_d.as<qh_pq_state>(), st_dev, st_dev + 1, ctx->stream);
  mark(2);
  launch_pq_strings(file.as<uint8_t>(), plan.upload_bytes, pages_d.as<qh_pq_page>(), npages, cols_d.as<qh_pq_col>(), state_d.as<qh_pq_state>(), st_dev, ctx->stream);
  mark(3);
  launch_pq_values(file.as<uint8_t>(), pages_d.as<qh_pq_page>(), npages, cols_d.as<qh_pq_col>(), state_d.as<qh_pq_state>(), st_dev, st_dev + 1 + QH_PQ_MAX_COLS, ctx->stream);
  time_mark(ctx, 3);
  mark(4);
  std::vector<uint64_t> back(st_host.size());
  copy_sync(ctx->stream, back.data(), st.ptr, st.bytes, hipMemcpyDeviceToHost);   // the host wait (also: the upload has left `bytes`)
  if (back[0] != ~0ULL) {
    const uint64_t pg = back[0] >> 8;
    qhip_pq::PqNeedsHost e{(int)(back[0] & 0xFF), -1, -1, -1};
    if (pg < plan.where.size()) { e.row_group = plan.where[pg].row_group; e.column = plan.where[pg].column; e.page = plan.where[pg].page; }
    fail(QHIP_UNSUPPORTED, qhip_pq::needs_host_text(e));
  }

  // ---- 5. NULL counts; Utf8 bytes
  for (size_t k = 0; k < ncols; ++k) {
    Out& o = outs[k];
    o.col.null_count = (int64_t)back[1 + k];
    if (o.col.null_count == 0) o.col.validity.reset();   // as upload_column: no NULLs, no bitmap
    if (o.col.type.id != QHIP_UTF8) continue;
    const uint64_t total = back[1 + QH_PQ_MAX_COLS + k];
    if (total > 0x7fffffffULL) fail(QHIP_UNSUPPORTED, qhip_pq::needs_host_text(qhip_pq::PqNeedsHost{QH_PQ_R_UTF8_LONG, -1, proj[k], -1}));
    o.col.data = std::make_shared<DevBuf>((size_t)total);
    o.col.data_bytes = (int64_t)total;
    uint32_t* off = o.col.values->as<uint32_t>();
    exclusive_scan_u32(off, off, R, off + R, ctx->stream);
    launch_csv_copy_utf8(file.as<uint8_t>(), o.strpos->as<uint64_t>(), off, R, o.col.data->as<uint8_t>(), ctx->stream);
  }
  mark(5);
  for (auto& o : outs) t->cols.push_back(std::move(o.col));
  // (the uploaded chunks, the page table, the entries and the string positions go back to the pool here: its reuse is ordered
  // on the one stream)
  if (ctx->timing) {
    QHIP_HIP_CHECK(sync_event(ev[5]));
    for (int k = 0; k < 5; ++k) (void)hipEventElapsedTime(&ctx->parquet_pass_ms[k], ev[k], ev[k + 1]);
  }
  time_mark(ctx, 1);
  t->num_rows = (int64_t)R;
  // batches as the host path cuts them (read_table, combine_chunks, to_batches): every batch_rows rows of the whole table
  t->batch_offsets.push_back(0);
  const uint64_t step = batch_rows > 0 ? (uint64_t)batch_rows : R;
  for (uint64_t r = step; r < R; r += step) t->batch_offsets.push_back((int64_t)r);
  t->batch_offsets.push_back((int64_t)R);
  ctx->stats_timing_pending = ctx->timing ? 2 : 0;
  ctx->stats.rows_in = (int64_t)R;
  ctx->stats.rows_out = (int64_t)R;
  ctx->stats.bytes_per_row_read = (double)plan.upload_bytes / (double)R;
  snprintf(ctx->stats.main_kernel_name, sizeof ctx->stats.main_kernel_name, "k_pq_values");
  return t.release();
}

}  // namespace qhip

using namespace qhip;

extern "C" {

int qhip_table_from_parquet(qhip_ctx* ctx, const struct ArrowSchema* schema, const void* bytes, int64_t n_bytes, const int32_t* columns, int32_t n_columns,
                            int64_t batch_rows, qhip_table** out) {
  if (!ctx || !out || n_bytes < 0 || (n_bytes > 0 && !bytes) || n_columns < 0) return QHIP_INVALID_ARGUMENT;
  *out = nullptr;
  return guarded(ctx, [&] { *out = table_from_parquet(ctx, schema, (const uint8_t*)bytes, n_bytes, columns, n_columns, batch_rows); });
}

int qhip_ctx_parquet_pass_ms(const qhip_ctx* ctx, double* out, int32_t n_out) {
  if (!ctx || !out || n_out != 5) return QHIP_INVALID_ARGUMENT;
  for (int k = 0; k < 5; ++k) out[k] = (double)ctx->parquet_pass_ms[k];
  return QHIP_OK;
}

}  // extern "C"
