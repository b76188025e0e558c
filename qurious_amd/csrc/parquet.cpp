// parquet.cpp — qhip_table_from_parquet: a Parquet file's bytes -> an HBM-resident table, decoded on the device.
//
// The reference reads Parquet on the host (datasource/file/parquet.rs) and so did this project (pyarrow, then an upload of the
// decoded columns). Here the host reads the footer and one header per page of the projected chunks (parquet_meta.hpp: a Thrift
// compact reader and the page walk, plain C++), uploads the bytes of those chunks alone — an unprojected column never crosses
// PCIe — and the device turns pages into columns. Format level 1: uncompressed chunks, data pages V1, PLAIN and dictionary
// encodings, RLE definition levels, flat columns. Format level 2 (qhip_ctx_set_parquet_format) adds SNAPPY chunks: their pages
// are uploaded compressed and unpacked on the device into an unpack area behind the uploaded chunks in the same buffer, where
// the passes below read them as they read any page. Encoding set 2 (qhip_ctx_set_parquet_encodings), independent of the level,
// adds data pages V2, RLE Boolean values, BYTE_STREAM_SPLIT, DELTA_BINARY_PACKED and DELTA_LENGTH_BYTE_ARRAY: a pass in front
// (k_pq_delta) leaves a delta page's values dense in a decoded area behind the unpack area. Codec set 2
// (qhip_ctx_set_parquet_codecs), independent of both, adds ZSTD chunks: their pages get slots in the same unpack area and a
// kernel of their own (k_pq_unzstd, a whole Zstandard frame decoder; the content checksum is not verified). The gzip switch
// (qhip_ctx_set_parquet_gzip), a fourth independent one, adds GZIP chunks the same way (k_pq_ungzip, an inflate kernel; the
// CRC32 is not verified). The lz4 switch (qhip_ctx_set_parquet_lz4), a fifth, adds LZ4_RAW and legacy LZ4 chunks (k_pq_unlz4,
// one wavefront per bare block; Hadoop's frames are split on the host). The DELTA_BYTE_ARRAY switch
// (qhip_ctx_set_parquet_delta_byte_array), a sixth, adds data pages of that encoding in Utf8 columns and FIXED_LEN_BYTE_ARRAY
// decimals: k_pq_delta_dba decodes their prefix and suffix lengths, k_pq_dba_fill reconstructs the prefixes 64 rows at a time.
// Whatever lies outside makes the whole call answer QHIP_UNSUPPORTED with nothing
// created, and the caller takes the host path, which then produces every error message.
//
// Passes, all on the context's stream:
//   1 upload        the projected chunks, one behind the other, into one device buffer; the page table and column descriptors
//  (k_pq_unsnap    level 2, a file with Snappy pages only: one wavefront per page, into the unpack area)
//  (k_pq_unzstd    codec set 2, a file with ZSTD pages only: one wavefront per page, into the unpack area)
//  (k_pq_ungzip    the gzip switch, a file with GZIP pages only: one wavefront per page, into the unpack area)
//  (k_pq_unlz4     the lz4 switch, a file with LZ4 pages only: one wavefront per block, into the unpack area)
//   2 k_pq_levels   definition levels -> validity words, non-NULL count per page, NULL count per column
//  (k_pq_delta     set 2, a file with DELTA_* pages only: one wavefront per page, into the decoded area or the column's entries)
//  (k_pq_delta_dba the DELTA_BYTE_ARRAY switch, a file with such pages only: both length streams of a page -> its entries)
//  (k_pq_dba_fill  the DELTA_BYTE_ARRAY switch, FIXED_LEN_BYTE_ARRAY pages of that encoding only: value space, into the decoded area)
//   3 k_pq_strings  Utf8: the length chains of dictionary pages and PLAIN data pages -> (length, position) entries
//   4 k_pq_values   values: bit-unpack, dictionary gather, scatter over NULLs; Utf8 rows get (length, position)
//  (k_pq_values_ext set 2, a file with RLE Boolean, BYTE_STREAM_SPLIT or DELTA_* pages only: the same body for those pages)
//                   -> the ONE host wait: first offender, NULL counts, Utf8 byte totals (they size the data buffers)
//   5 Utf8          lengths scanned in place into offsets, k_csv_copy_utf8 moves the bytes (no wait: stream-ordered)
//  (k_pq_dba_copy / k_pq_dba_fill  the DELTA_BYTE_ARRAY switch, Utf8 columns with such a page only: k_pq_dba_copy in
//                   k_csv_copy_utf8's place moves the suffixes, k_pq_dba_fill, row space, fills in the prefixes; no wait)
#include <hip/hip_runtime_api.h>
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "kernels_parquet.hpp"
#include "parquet_meta.hpp"

namespace qhip {

static_assert(sizeof(qh_pq_dstream) == 32, "the delta-table entry has the layout both compilers agree on");
static_assert(sizeof(qh_pq_fill) == 32, "the fill-table entry has the layout both compilers agree on");
static_assert(sizeof(qh_pq_page) == 80 && sizeof(qh_pq_col) == 56 && sizeof(qh_pq_ent) == 16, "the Parquet descriptors have the layout both compilers agree on");
static_assert(sizeof(qh_pq_unpack) == 32, "the unpack-table entry has the layout both compilers agree on");

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
    plan = qhip_pq::plan_file(bytes, (uint64_t)n_bytes, &names, types, proj, ctx->parquet_format, ctx->parquet_encodings, ctx->parquet_codecs, ctx->parquet_gzip, ctx->parquet_lz4,
                              ctx->parquet_dba);
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
  ctx->parquet_unpack_ms = 0;
  ctx->parquet_delta_ms = 0;
  ctx->parquet_fill_ms = 0;
  // ([6]: behind the unpack pass, [7]: behind the delta pass, [8]: behind the fill of the FIXED_LEN_BYTE_ARRAY pages, [9]: in front of the fill of the Utf8 columns)
  hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int k = 0; k < 10; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
  auto mark = [&](int k) {
    if (!ctx->timing) return;
    if (!ev[k]) QHIP_HIP_CHECK(hipEventCreate(&ev[k]));
    QHIP_HIP_CHECK(hipEventRecord(ev[k], ctx->stream));
  };
  time_mark(ctx, 0);
  mark(0);

  // ---- 1. upload: the projected chunks only (the buffer keeps the 64 bytes of slack DevBuf::alloc gives); behind them the
  // unpack area of a file with Snappy pages and the decoded area of one with DELTA_BINARY_PACKED pages, which nothing uploads
  const uint64_t buf_bytes = plan.buffer_bytes();
  const uint32_t nunpack = (uint32_t)plan.unpack.size();
  DevBuf file((size_t)buf_bytes);
  const size_t kPiece = 64u << 20;
  for (const qhip_pq::Range& r : plan.ranges)
    for (uint64_t o = 0; o < r.bytes; o += kPiece)
      QHIP_HIP_CHECK(hipMemcpyAsync((uint8_t*)file.ptr + r.buf_off + o, bytes + r.file_off + o, (size_t)std::min<uint64_t>(kPiece, r.bytes - o), hipMemcpyHostToDevice,
                                    ctx->stream));
  DevBuf pages_d((size_t)npages * sizeof(qh_pq_page)), state_d((size_t)npages * sizeof(qh_pq_state)), cols_d(ncols * sizeof(qh_pq_col));
  QHIP_HIP_CHECK(hipMemcpyAsync(pages_d.ptr, plan.pages.data(), (size_t)npages * sizeof(qh_pq_page), hipMemcpyHostToDevice, ctx->stream));
  // status words: [0] first offender (page << 8 | reason), [1 .. 1 + 64) NULL counts, then Utf8 byte totals, then the unpack
  // pass's own first offender
  const size_t kUnpackWord = 1 + 2 * QH_PQ_MAX_COLS;
  std::vector<uint64_t> st_host(kUnpackWord + 1, 0);
  st_host[0] = st_host[kUnpackWord] = ~0ULL;
  DevBuf st(st_host.size() * 8);
  QHIP_HIP_CHECK(hipMemcpyAsync(st.ptr, st_host.data(), st.bytes, hipMemcpyHostToDevice, ctx->stream));
  uint64_t* st_dev = st.as<uint64_t>();

  struct Out { DevColumn col; std::shared_ptr<DevBuf> strpos, ent, prefix; };
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
      if (cp.dba) {   // (rows of the column's other pages keep prefix 0)
        o.prefix = std::make_shared<DevBuf>((size_t)R * 4);
        QHIP_HIP_CHECK(hipMemsetAsync(o.prefix->ptr, 0, (size_t)R * 4, ctx->stream));
        d.prefix = o.prefix->as<pq_u32>();
      }
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
  DevBuf unpack_d;
  if (nunpack) unpack_d.alloc((size_t)nunpack * sizeof(qh_pq_unpack));
  if (nunpack) QHIP_HIP_CHECK(hipMemcpyAsync(unpack_d.ptr, plan.unpack.data(), (size_t)nunpack * sizeof(qh_pq_unpack), hipMemcpyHostToDevice, ctx->stream));
  const uint32_t nunzstd = (uint32_t)plan.unzstd.size();
  DevBuf unzstd_d;
  if (nunzstd) unzstd_d.alloc((size_t)nunzstd * sizeof(qh_pq_unpack));
  if (nunzstd) QHIP_HIP_CHECK(hipMemcpyAsync(unzstd_d.ptr, plan.unzstd.data(), (size_t)nunzstd * sizeof(qh_pq_unpack), hipMemcpyHostToDevice, ctx->stream));
  const uint32_t nungzip = (uint32_t)plan.ungzip.size();
  DevBuf ungzip_d;
  if (nungzip) ungzip_d.alloc((size_t)nungzip * sizeof(qh_pq_unpack));
  if (nungzip) QHIP_HIP_CHECK(hipMemcpyAsync(ungzip_d.ptr, plan.ungzip.data(), (size_t)nungzip * sizeof(qh_pq_unpack), hipMemcpyHostToDevice, ctx->stream));
  const uint32_t nunlz4 = (uint32_t)plan.unlz4.size();
  DevBuf unlz4_d;
  if (nunlz4) unlz4_d.alloc((size_t)nunlz4 * sizeof(qh_pq_unpack));
  if (nunlz4) QHIP_HIP_CHECK(hipMemcpyAsync(unlz4_d.ptr, plan.unlz4.data(), (size_t)nunlz4 * sizeof(qh_pq_unpack), hipMemcpyHostToDevice, ctx->stream));
  const uint32_t ndelta = (uint32_t)plan.delta.size();
  DevBuf delta_d;
  if (ndelta) delta_d.alloc((size_t)ndelta * sizeof(qh_pq_dstream));
  if (ndelta) QHIP_HIP_CHECK(hipMemcpyAsync(delta_d.ptr, plan.delta.data(), (size_t)ndelta * sizeof(qh_pq_dstream), hipMemcpyHostToDevice, ctx->stream));
  // the DELTA_BYTE_ARRAY switch: the fill jobs of the FIXED_LEN_BYTE_ARRAY pages, behind them those of the Utf8 pages by column
  std::stable_sort(plan.fill_rows.begin(), plan.fill_rows.end(), [](const qh_pq_fill& a, const qh_pq_fill& b) { return a.col < b.col; });
  const uint32_t nfillv = (uint32_t)plan.fill_values.size(), nfillr = (uint32_t)plan.fill_rows.size(), ndba = nfillv + nfillr;
  std::vector<qh_pq_fill> fill_host(plan.fill_values);
  fill_host.insert(fill_host.end(), plan.fill_rows.begin(), plan.fill_rows.end());
  DevBuf fill_d;
  if (!fill_host.empty()) fill_d.alloc(fill_host.size() * sizeof(qh_pq_fill));
  if (!fill_host.empty()) QHIP_HIP_CHECK(hipMemcpyAsync(fill_d.ptr, fill_host.data(), fill_host.size() * sizeof(qh_pq_fill), hipMemcpyHostToDevice, ctx->stream));
  mark(1);

  // ---- level 2: the Snappy pages into their slots; codec set 2: the ZSTD pages into theirs; the gzip switch: the GZIP pages; the lz4
  // switch: the LZ4 blocks
  time_mark(ctx, 2);
  if (nunpack) launch_pq_unsnap(file.as<uint8_t>(), buf_bytes, unpack_d.as<qh_pq_unpack>(), nunpack, st_dev + kUnpackWord, nullptr, ctx->stream);
  if (nunzstd) launch_pq_unzstd(file.as<uint8_t>(), unzstd_d.as<qh_pq_unpack>(), nunzstd, st_dev + kUnpackWord, nullptr, ctx->stream);
  if (nungzip) launch_pq_ungzip(file.as<uint8_t>(), ungzip_d.as<qh_pq_unpack>(), nungzip, st_dev + kUnpackWord, nullptr, ctx->stream);
  if (nunlz4) launch_pq_unlz4(file.as<uint8_t>(), unlz4_d.as<qh_pq_unpack>(), nunlz4, st_dev + kUnpackWord, nullptr, ctx->stream);
  if (nunpack || nunzstd || nungzip || nunlz4) mark(6);

  // ---- 2 .. 4: levels, string walk, values
  launch_pq_levels(file.as<uint8_t>(), pages_d.as<qh_pq_page>(), npages, cols_d.as<qh_pq_col>(), state_d.as<qh_pq_state>(), st_dev, st_dev + 1, ctx->stream);
  mark(2);
  if (ndelta) {   // (behind the levels: a page's stream begins where they end and holds its non-NULL rows)
    launch_pq_delta(file.as<uint8_t>(), delta_d.as<qh_pq_dstream>(), ndelta, pages_d.as<qh_pq_page>(), cols_d.as<qh_pq_col>(), state_d.as<qh_pq_state>(), st_dev, nullptr,
                    nullptr, (ndelta > ndba ? 1u : 0u) | (ndba ? 2u : 0u), ctx->stream);
    mark(7);
    if (nfillv) {   // (the FIXED_LEN_BYTE_ARRAY pages of DELTA_BYTE_ARRAY: dense into their slots, from where k_pq_values_ext reads them as PLAIN)
      launch_pq_dba_fill(file.as<uint8_t>(), fill_d.as<qh_pq_fill>(), nfillv, nullptr, nullptr, nullptr, state_d.as<qh_pq_state>(), st_dev, ctx->stream);
      mark(8);
    }
  }
  launch_pq_strings(file.as<uint8_t>(), buf_bytes, pages_d.as<qh_pq_page>(), npages, cols_d.as<qh_pq_col>(), state_d.as<qh_pq_state>(), st_dev, ctx->stream);
  mark(3);
  launch_pq_values(file.as<uint8_t>(), pages_d.as<qh_pq_page>(), npages, cols_d.as<qh_pq_col>(), state_d.as<qh_pq_state>(), st_dev, st_dev + 1 + QH_PQ_MAX_COLS, ctx->stream);
  if (plan.has_ext)
    launch_pq_values_ext(file.as<uint8_t>(), pages_d.as<qh_pq_page>(), npages, cols_d.as<qh_pq_col>(), state_d.as<qh_pq_state>(), st_dev, st_dev + 1 + QH_PQ_MAX_COLS,
                         ctx->stream);
  time_mark(ctx, 3);
  mark(4);
  std::vector<uint64_t> back(st_host.size());
  copy_sync(ctx->stream, back.data(), st.ptr, st.bytes, hipMemcpyDeviceToHost);   // the host wait (also: the upload has left `bytes`)
  // (a page whose unpacking failed holds whatever its slot held: what the later passes say of it does not count)
  const uint64_t offender = back[kUnpackWord] != ~0ULL ? back[kUnpackWord] : back[0];
  if (offender != ~0ULL) {
    const uint64_t pg = offender >> 8;
    qhip_pq::PqNeedsHost e{(int)(offender & 0xFF), -1, -1, -1};
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
    if (o.prefix) launch_pq_dba_copy(file.as<uint8_t>(), o.strpos->as<uint64_t>(), off, o.prefix->as<uint32_t>(), R, o.col.data->as<uint8_t>(), ctx->stream);
    else launch_csv_copy_utf8(file.as<uint8_t>(), o.strpos->as<uint64_t>(), off, R, o.col.data->as<uint8_t>(), ctx->stream);
  }
  if (nfillr) {   // the Utf8 columns with DELTA_BYTE_ARRAY pages: their prefixes, in row space, straight into the column's data
    mark(9);
    for (uint32_t a = 0; a < nfillr;) {
      uint32_t b = a;
      while (b < nfillr && plan.fill_rows[b].col == plan.fill_rows[a].col) ++b;
      Out& o = outs[plan.fill_rows[a].col];
      launch_pq_dba_fill(o.col.data->as<uint8_t>(), fill_d.as<qh_pq_fill>() + nfillv + a, b - a, o.col.values->as<uint32_t>(), o.prefix->as<uint32_t>(),
                         o.col.validity ? o.col.validity->as<uint64_t>() : nullptr, nullptr, nullptr, ctx->stream);
      a = b;
    }
  }
  mark(5);
  for (auto& o : outs) t->cols.push_back(std::move(o.col));
  // (the uploaded chunks, the page table, the entries and the string positions go back to the pool here: its reuse is ordered
  // on the one stream)
  if (ctx->timing) {
    QHIP_HIP_CHECK(sync_event(ev[5]));
    for (int k = 0; k < 5; ++k) (void)hipEventElapsedTime(&ctx->parquet_pass_ms[k], ev[k], ev[k + 1]);
    if (ev[6]) {   // "levels" begins behind the unpack passes, "upload" stays the upload
      (void)hipEventElapsedTime(&ctx->parquet_unpack_ms, ev[1], ev[6]);
      (void)hipEventElapsedTime(&ctx->parquet_pass_ms[1], ev[6], ev[2]);
    }
    if (ev[7]) {   // ... and the "string walk" behind the delta pass
      (void)hipEventElapsedTime(&ctx->parquet_delta_ms, ev[2], ev[7]);
      (void)hipEventElapsedTime(&ctx->parquet_pass_ms[2], ev[7], ev[3]);
    }
    if (ev[8]) {   // ... behind the fill of the FIXED_LEN_BYTE_ARRAY pages, where there is one
      (void)hipEventElapsedTime(&ctx->parquet_fill_ms, ev[7], ev[8]);
      (void)hipEventElapsedTime(&ctx->parquet_pass_ms[2], ev[8], ev[3]);
    }
    if (ev[9]) {   // ... and "Utf8" ends in front of the fill of the Utf8 columns
      float rows_ms = 0;
      (void)hipEventElapsedTime(&rows_ms, ev[9], ev[5]);
      (void)hipEventElapsedTime(&ctx->parquet_pass_ms[4], ev[4], ev[9]);
      ctx->parquet_fill_ms += rows_ms;
    }
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

// qhip_snappy_decode / qhip_zstd_decode / qhip_gzip_decode / qhip_lz4_decode: k_pq_unsnap / k_pq_unzstd / k_pq_ungzip /
// k_pq_unlz4 over raw streams, with the checks the page walk makes of a page's sizes (of a ZSTD page: its frame header and block
// headers; of a GZIP page: its member header and ISIZE; of an LZ4 block: the 255x bound). A refused stream is an answer (status),
// not an error.
enum UnpackCodec { kSnappy, kZstd, kGzip, kLz4 };
static void unpack_decode(Ctx* ctx, UnpackCodec codec, const uint8_t* bytes, int64_t n_bytes, const int64_t* src_offsets, const int64_t* dst_sizes, int64_t n_streams,
                          uint8_t* out, int64_t out_bytes, int32_t* status) {
  const bool zstd = codec == kZstd, gz = codec == kGzip, lz = codec == kLz4;
  const std::string fn = lz ? "qhip_lz4_decode" : gz ? "qhip_gzip_decode" : zstd ? "qhip_zstd_decode" : "qhip_snappy_decode";
  const int reason_base = lz ? QH_PQ_R_LZ4_BASE : gz ? QH_PQ_R_GZIP_BASE : zstd ? QH_PQ_R_ZSTD_BASE : QH_PQ_R_SNAPPY_BASE;
  uint64_t total_out = 0;
  for (int64_t k = 0; k < n_streams; ++k) {
    const int64_t a = src_offsets[k], b = src_offsets[k + 1];
    if (a < 0 || b < a || b > n_bytes || b - a > 0x7FFFFFFF || dst_sizes[k] < 0 || dst_sizes[k] > 0x7FFFFFFF)
      fail(QHIP_INVALID_ARGUMENT, fn + ": stream " + std::to_string(k) + " lies outside the bytes, or a size is negative or above 2^31 - 1");
    total_out += (uint64_t)dst_sizes[k];
  }
  if (total_out > (uint64_t)out_bytes) fail(QHIP_INVALID_ARGUMENT, fn + ": out is smaller than the sum of dst_sizes");
  const uint64_t base = ((uint64_t)n_bytes + 15) & ~(uint64_t)15;
  uint64_t area = 0;
  std::vector<qh_pq_unpack> tab;
  for (int64_t k = 0; k < n_streams; ++k) {
    qh_pq_unpack u;
    memset(&u, 0, sizeof u);
    const uint64_t len = (uint64_t)(src_offsets[k + 1] - src_offsets[k]);
    const int bad = lz     ? qh_lz4_check_sizes(len, (uint64_t)dst_sizes[k])
                    : gz   ? qh_gzip_check_member(bytes + src_offsets[k], len, (uint64_t)dst_sizes[k], &u.start)
                    : zstd ? qh_zstd_check_frame(bytes + src_offsets[k], len, (uint64_t)dst_sizes[k], &u.start)
                           : qh_snap_check_sizes(bytes + src_offsets[k], len, (uint64_t)dst_sizes[k], &u.start);
    status[k] = bad ? reason_base + bad : QH_PQ_OK;
    if (bad) continue;
    u.src = (uint64_t)src_offsets[k]; u.src_size = (uint32_t)(src_offsets[k + 1] - src_offsets[k]);
    u.dst = base + area; u.dst_size = (uint32_t)dst_sizes[k];
    u.page = (uint32_t)k;
    tab.push_back(u);
    area += ((uint64_t)u.dst_size + 15) & ~(uint64_t)15;
  }
  ctx->parquet_unpack_ms = 0;
  if (tab.empty()) return;
  QHIP_HIP_CHECK(hipSetDevice(ctx->device));
  const uint32_t nt = (uint32_t)tab.size();
  DevBuf buf((size_t)(base + area)), tab_d((size_t)nt * sizeof(qh_pq_unpack)), st_d((size_t)nt * 4);
  if (n_bytes) QHIP_HIP_CHECK(hipMemcpyAsync(buf.ptr, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, ctx->stream));
  QHIP_HIP_CHECK(hipMemcpyAsync(tab_d.ptr, tab.data(), (size_t)nt * sizeof(qh_pq_unpack), hipMemcpyHostToDevice, ctx->stream));
  hipEvent_t ev[2] = {nullptr, nullptr};
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
  if (ctx->timing) { QHIP_HIP_CHECK(hipEventCreate(&ev[0])); QHIP_HIP_CHECK(hipEventCreate(&ev[1])); QHIP_HIP_CHECK(hipEventRecord(ev[0], ctx->stream)); }
  if (lz) launch_pq_unlz4(buf.as<uint8_t>(), tab_d.as<qh_pq_unpack>(), nt, nullptr, st_d.as<uint32_t>(), ctx->stream);
  else if (gz) launch_pq_ungzip(buf.as<uint8_t>(), tab_d.as<qh_pq_unpack>(), nt, nullptr, st_d.as<uint32_t>(), ctx->stream);
  else if (zstd) launch_pq_unzstd(buf.as<uint8_t>(), tab_d.as<qh_pq_unpack>(), nt, nullptr, st_d.as<uint32_t>(), ctx->stream);
  else launch_pq_unsnap(buf.as<uint8_t>(), base + area, tab_d.as<qh_pq_unpack>(), nt, nullptr, st_d.as<uint32_t>(), ctx->stream);
  if (ctx->timing) QHIP_HIP_CHECK(hipEventRecord(ev[1], ctx->stream));
  std::vector<uint8_t> unpacked((size_t)area);
  std::vector<uint32_t> st(nt);
  if (area) QHIP_HIP_CHECK(hipMemcpyAsync(unpacked.data(), (const uint8_t*)buf.ptr + base, (size_t)area, hipMemcpyDeviceToHost, ctx->stream));
  copy_sync(ctx->stream, st.data(), st_d.ptr, (size_t)nt * 4, hipMemcpyDeviceToHost);
  if (ctx->timing) (void)hipEventElapsedTime(&ctx->parquet_unpack_ms, ev[0], ev[1]);
  std::vector<uint64_t> out_at((size_t)n_streams);
  uint64_t at = 0;
  for (int64_t k = 0; k < n_streams; ++k) { out_at[(size_t)k] = at; at += (uint64_t)dst_sizes[k]; }
  for (uint32_t i = 0; i < nt; ++i) {
    const qh_pq_unpack& u = tab[i];
    status[u.page] = st[i] ? (int32_t)(reason_base + st[i]) : QH_PQ_OK;
    if (!st[i] && u.dst_size) memcpy(out + out_at[u.page], unpacked.data() + (u.dst - base), u.dst_size);
  }
}
void snappy_decode(Ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const int64_t* src_offsets, const int64_t* dst_sizes, int64_t n_streams, uint8_t* out,
                   int64_t out_bytes, int32_t* status) {
  unpack_decode(ctx, kSnappy, bytes, n_bytes, src_offsets, dst_sizes, n_streams, out, out_bytes, status);
}
void zstd_decode(Ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const int64_t* src_offsets, const int64_t* dst_sizes, int64_t n_streams, uint8_t* out,
                 int64_t out_bytes, int32_t* status) {
  unpack_decode(ctx, kZstd, bytes, n_bytes, src_offsets, dst_sizes, n_streams, out, out_bytes, status);
}
void gzip_decode(Ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const int64_t* src_offsets, const int64_t* dst_sizes, int64_t n_streams, uint8_t* out,
                 int64_t out_bytes, int32_t* status) {
  unpack_decode(ctx, kGzip, bytes, n_bytes, src_offsets, dst_sizes, n_streams, out, out_bytes, status);
}
void lz4_decode(Ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const int64_t* src_offsets, const int64_t* dst_sizes, int64_t n_streams, uint8_t* out,
                int64_t out_bytes, int32_t* status) {
  unpack_decode(ctx, kLz4, bytes, n_bytes, src_offsets, dst_sizes, n_streams, out, out_bytes, status);
}

// qhip_parquet_delta_decode: k_pq_delta over raw DELTA_BINARY_PACKED streams. A refused stream is an answer (status), not an error.
void delta_decode(Ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const int64_t* src_offsets, const int32_t* widths, const int64_t* counts, int64_t n_streams,
                  uint8_t* out, int64_t out_bytes, int64_t* end_pos, int32_t* status) {
  uint64_t total_out = 0;
  for (int64_t k = 0; k < n_streams; ++k) {
    const int64_t a = src_offsets[k], b = src_offsets[k + 1];
    if (a < 0 || b < a || b > n_bytes || b - a > 0x7FFFFFFF || counts[k] < 0 || counts[k] > 0x0FFFFFFF || (widths[k] != 4 && widths[k] != 8))
      fail(QHIP_INVALID_ARGUMENT, "qhip_parquet_delta_decode: stream " + std::to_string(k) + " lies outside the bytes, its count is negative or above 2^28 - 1, or its width is not 4 or 8");
    total_out += (uint64_t)counts[k] * (uint64_t)widths[k];
  }
  if (total_out > (uint64_t)out_bytes) fail(QHIP_INVALID_ARGUMENT, "qhip_parquet_delta_decode: out is smaller than the sum of counts times widths");
  ctx->parquet_delta_ms = 0;
  if (!n_streams) return;
  const uint64_t base = ((uint64_t)n_bytes + 15) & ~(uint64_t)15;
  uint64_t area = 0;
  std::vector<qh_pq_dstream> tab((size_t)n_streams);
  for (int64_t k = 0; k < n_streams; ++k) {
    qh_pq_dstream& d = tab[(size_t)k];
    memset(&d, 0, sizeof d);
    d.src = (uint64_t)src_offsets[k]; d.src_size = (uint32_t)(src_offsets[k + 1] - src_offsets[k]);
    d.dst = base + area; d.count = (uint32_t)counts[k]; d.page = (uint32_t)k; d.width = (uint32_t)widths[k];
    area += ((uint64_t)d.count * d.width + 15) & ~(uint64_t)15;
  }
  QHIP_HIP_CHECK(hipSetDevice(ctx->device));
  const uint32_t nt = (uint32_t)n_streams;
  DevBuf buf((size_t)(base + area)), tab_d((size_t)nt * sizeof(qh_pq_dstream)), st_d((size_t)nt * 4), end_d((size_t)nt * 8);
  if (n_bytes) QHIP_HIP_CHECK(hipMemcpyAsync(buf.ptr, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, ctx->stream));
  QHIP_HIP_CHECK(hipMemcpyAsync(tab_d.ptr, tab.data(), (size_t)nt * sizeof(qh_pq_dstream), hipMemcpyHostToDevice, ctx->stream));
  hipEvent_t ev[2] = {nullptr, nullptr};
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
  if (ctx->timing) { QHIP_HIP_CHECK(hipEventCreate(&ev[0])); QHIP_HIP_CHECK(hipEventCreate(&ev[1])); QHIP_HIP_CHECK(hipEventRecord(ev[0], ctx->stream)); }
  launch_pq_delta(buf.as<uint8_t>(), tab_d.as<qh_pq_dstream>(), nt, nullptr, nullptr, nullptr, nullptr, st_d.as<uint32_t>(), end_d.as<uint64_t>(), 1u, ctx->stream);
  if (ctx->timing) QHIP_HIP_CHECK(hipEventRecord(ev[1], ctx->stream));
  std::vector<uint8_t> dense((size_t)area);
  std::vector<uint32_t> st(nt);
  std::vector<uint64_t> ends(nt);
  if (area) QHIP_HIP_CHECK(hipMemcpyAsync(dense.data(), (const uint8_t*)buf.ptr + base, (size_t)area, hipMemcpyDeviceToHost, ctx->stream));
  QHIP_HIP_CHECK(hipMemcpyAsync(ends.data(), end_d.ptr, (size_t)nt * 8, hipMemcpyDeviceToHost, ctx->stream));
  copy_sync(ctx->stream, st.data(), st_d.ptr, (size_t)nt * 4, hipMemcpyDeviceToHost);
  if (ctx->timing) (void)hipEventElapsedTime(&ctx->parquet_delta_ms, ev[0], ev[1]);
  uint64_t at = 0;
  for (uint32_t i = 0; i < nt; ++i) {
    const qh_pq_dstream& d = tab[i];
    const uint64_t nb = (uint64_t)d.count * d.width;
    status[i] = (int32_t)st[i];
    end_pos[i] = st[i] ? -1 : (int64_t)ends[i];
    if (!st[i] && nb) memcpy(out + at, dense.data() + (d.dst - base), (size_t)nb);
    at += nb;
  }
}

// qhip_parquet_dba_decode: raw DELTA_BYTE_ARRAY value streams through the kernels a file's pages go through: k_pq_delta_dba (both
// length streams -> entries), then, behind a wait of its own that a file does not need (there the column's one wait serves), the
// scan of the lengths on the host, k_pq_dba_copy and k_pq_dba_fill in row space, the values of the good streams one behind the
// other as the rows of one column without NULLs. A refused stream is an answer (status), not an error.
void dba_decode(Ctx* ctx, const uint8_t* bytes, int64_t n_bytes, const int64_t* src_offsets, const int32_t* widths, const int64_t* counts, int64_t n_streams,
                uint8_t* out, int64_t out_bytes, int64_t* value_offsets, int64_t* total_bytes, int32_t* status) {
  uint64_t nvalues = 0;
  for (int64_t k = 0; k < n_streams; ++k) {
    const int64_t a = src_offsets[k], b = src_offsets[k + 1];
    if (a < 0 || b < a || b > n_bytes || b - a > 0x7FFFFFFF || counts[k] < 0 || counts[k] > 0x0FFFFFFF || widths[k] < 0 || widths[k] > 16)
      fail(QHIP_INVALID_ARGUMENT, "qhip_parquet_dba_decode: stream " + std::to_string(k) + " lies outside the bytes, its count is negative or above 2^28 - 1, or its width is not 0 .. 16");
    nvalues += (uint64_t)counts[k];
  }
  if (nvalues > 0x0FFFFFFFull) fail(QHIP_INVALID_ARGUMENT, "qhip_parquet_dba_decode: more than 2^28 - 1 values in all");
  ctx->parquet_delta_ms = 0;
  ctx->parquet_fill_ms = 0;
  *total_bytes = 0;
  if (!n_streams) return;
  const uint64_t base = ((uint64_t)n_bytes + 15) & ~(uint64_t)15;
  uint64_t area = 0;
  std::vector<qh_pq_dstream> tab((size_t)n_streams);
  for (int64_t k = 0; k < n_streams; ++k) {
    qh_pq_dstream& d = tab[(size_t)k];
    memset(&d, 0, sizeof d);
    d.src = (uint64_t)src_offsets[k]; d.src_size = (uint32_t)(src_offsets[k + 1] - src_offsets[k]);
    d.dst = base + area; d.count = (uint32_t)counts[k]; d.page = (uint32_t)k; d.width = (uint32_t)widths[k] | QH_PQ_DS_DBA;
    area += (uint64_t)d.count * sizeof(qh_pq_ent);
  }
  QHIP_HIP_CHECK(hipSetDevice(ctx->device));
  const uint32_t nt = (uint32_t)n_streams;
  DevBuf buf((size_t)(base + area)), tab_d((size_t)nt * sizeof(qh_pq_dstream)), st_d((size_t)nt * 4);
  if (n_bytes) QHIP_HIP_CHECK(hipMemcpyAsync(buf.ptr, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, ctx->stream));
  QHIP_HIP_CHECK(hipMemcpyAsync(tab_d.ptr, tab.data(), (size_t)nt * sizeof(qh_pq_dstream), hipMemcpyHostToDevice, ctx->stream));
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int k = 0; k < 4; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
  if (ctx->timing) for (int k = 0; k < 4; ++k) QHIP_HIP_CHECK(hipEventCreate(&ev[k]));
  if (ctx->timing) QHIP_HIP_CHECK(hipEventRecord(ev[0], ctx->stream));
  launch_pq_delta(buf.as<uint8_t>(), tab_d.as<qh_pq_dstream>(), nt, nullptr, nullptr, nullptr, nullptr, st_d.as<uint32_t>(), nullptr, 2u, ctx->stream);
  if (ctx->timing) QHIP_HIP_CHECK(hipEventRecord(ev[1], ctx->stream));
  std::vector<qh_pq_ent> ents((size_t)(area / sizeof(qh_pq_ent)));
  std::vector<uint32_t> st(nt);
  if (area) QHIP_HIP_CHECK(hipMemcpyAsync(ents.data(), (const uint8_t*)buf.ptr + base, (size_t)area, hipMemcpyDeviceToHost, ctx->stream));
  copy_sync(ctx->stream, st.data(), st_d.ptr, (size_t)nt * 4, hipMemcpyDeviceToHost);
  if (ctx->timing) (void)hipEventElapsedTime(&ctx->parquet_delta_ms, ev[0], ev[1]);

  // the good streams' values as rows: lengths into offsets, where the suffixes lie, the prefix lengths, a fill job per stream
  std::vector<uint64_t> strpos;
  std::vector<uint32_t> off(1, 0), prefix;
  std::vector<qh_pq_fill> jobs;
  uint64_t total = 0;
  int64_t* vo = value_offsets;
  for (uint32_t i = 0; i < nt; ++i) {
    status[i] = (int32_t)st[i];
    const qh_pq_ent* e = ents.data() + (tab[i].dst - base) / sizeof(qh_pq_ent);
    const uint32_t c = st[i] ? 0u : tab[i].count;
    if (c) {
      qh_pq_fill fj;
      memset(&fj, 0, sizeof fj);
      fj.first = strpos.size(); fj.n = c; fj.page = i;
      jobs.push_back(fj);
    }
    for (uint32_t v = 0; v <= tab[i].count; ++v) {
      *vo++ = (int64_t)total;
      if (v < c) {
        total += e[v].len;
        if (total > 0x7fffffffULL) fail(QHIP_INVALID_ARGUMENT, "qhip_parquet_dba_decode: the values exceed 2^31 - 1 bytes");
        strpos.push_back(e[v].pos); prefix.push_back(e[v].pad); off.push_back((uint32_t)total);
      }
    }
  }
  *total_bytes = (int64_t)total;
  const uint64_t rows = strpos.size();
  if (!rows || !total || total > (uint64_t)out_bytes) return;
  DevBuf pos_d((size_t)rows * 8), off_d((size_t)(rows + 1) * 4), pre_d((size_t)rows * 4), jobs_d(jobs.size() * sizeof(qh_pq_fill)), data_d((size_t)total);
  QHIP_HIP_CHECK(hipMemcpyAsync(pos_d.ptr, strpos.data(), (size_t)rows * 8, hipMemcpyHostToDevice, ctx->stream));
  QHIP_HIP_CHECK(hipMemcpyAsync(off_d.ptr, off.data(), (size_t)(rows + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  QHIP_HIP_CHECK(hipMemcpyAsync(pre_d.ptr, prefix.data(), (size_t)rows * 4, hipMemcpyHostToDevice, ctx->stream));
  QHIP_HIP_CHECK(hipMemcpyAsync(jobs_d.ptr, jobs.data(), jobs.size() * sizeof(qh_pq_fill), hipMemcpyHostToDevice, ctx->stream));
  launch_pq_dba_copy(buf.as<uint8_t>(), pos_d.as<uint64_t>(), off_d.as<uint32_t>(), pre_d.as<uint32_t>(), rows, data_d.as<uint8_t>(), ctx->stream);
  if (ctx->timing) QHIP_HIP_CHECK(hipEventRecord(ev[2], ctx->stream));
  launch_pq_dba_fill(data_d.as<uint8_t>(), jobs_d.as<qh_pq_fill>(), (uint32_t)jobs.size(), off_d.as<uint32_t>(), pre_d.as<uint32_t>(), nullptr, nullptr, nullptr, ctx->stream);
  if (ctx->timing) QHIP_HIP_CHECK(hipEventRecord(ev[3], ctx->stream));
  copy_sync(ctx->stream, out, data_d.ptr, (size_t)total, hipMemcpyDeviceToHost);
  if (ctx->timing) (void)hipEventElapsedTime(&ctx->parquet_fill_ms, ev[2], ev[3]);
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

int qhip_ctx_parquet_unpack_ms(const qhip_ctx* ctx, double* out) {
  if (!ctx || !out) return QHIP_INVALID_ARGUMENT;
  *out = (double)ctx->parquet_unpack_ms;
  return QHIP_OK;
}

int qhip_ctx_parquet_delta_ms(const qhip_ctx* ctx, double* out) {
  if (!ctx || !out) return QHIP_INVALID_ARGUMENT;
  *out = (double)ctx->parquet_delta_ms;
  return QHIP_OK;
}

int qhip_ctx_parquet_fill_ms(const qhip_ctx* ctx, double* out) {
  if (!ctx || !out) return QHIP_INVALID_ARGUMENT;
  *out = (double)ctx->parquet_fill_ms;
  return QHIP_OK;
}

int qhip_parquet_dba_decode(qhip_ctx* ctx, const void* bytes, int64_t n_bytes, const int64_t* src_offsets, const int32_t* widths, const int64_t* counts,
                            int64_t n_streams, void* out, int64_t out_bytes, int64_t* value_offsets, int64_t* total_bytes, int32_t* status) {
  if (!ctx || n_bytes < 0 || (n_bytes > 0 && !bytes) || n_streams < 0 || out_bytes < 0 || (out_bytes > 0 && !out) || !total_bytes) return QHIP_INVALID_ARGUMENT;
  if (n_streams > 0 && (!src_offsets || !widths || !counts || !value_offsets || !status)) return QHIP_INVALID_ARGUMENT;
  if (n_streams >= (1 << 24)) return QHIP_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    dba_decode(ctx, (const uint8_t*)bytes, n_bytes, src_offsets, widths, counts, n_streams, (uint8_t*)out, out_bytes, value_offsets, total_bytes, status);
  });
}

int qhip_parquet_delta_decode(qhip_ctx* ctx, const void* bytes, int64_t n_bytes, const int64_t* src_offsets, const int32_t* widths, const int64_t* counts,
                              int64_t n_streams, void* out, int64_t out_bytes, int64_t* end_pos, int32_t* status) {
  if (!ctx || n_bytes < 0 || (n_bytes > 0 && !bytes) || n_streams < 0 || out_bytes < 0 || (out_bytes > 0 && !out)) return QHIP_INVALID_ARGUMENT;
  if (n_streams > 0 && (!src_offsets || !widths || !counts || !end_pos || !status)) return QHIP_INVALID_ARGUMENT;
  if (n_streams >= (1 << 24)) return QHIP_INVALID_ARGUMENT;
  return guarded(ctx, [&] { delta_decode(ctx, (const uint8_t*)bytes, n_bytes, src_offsets, widths, counts, n_streams, (uint8_t*)out, out_bytes, end_pos, status); });
}

int qhip_snappy_decode(qhip_ctx* ctx, const void* bytes, int64_t n_bytes, const int64_t* src_offsets, const int64_t* dst_sizes, int64_t n_streams, void* out,
                       int64_t out_bytes, int32_t* status) {
  if (!ctx || n_bytes < 0 || (n_bytes > 0 && !bytes) || n_streams < 0 || out_bytes < 0 || (out_bytes > 0 && !out)) return QHIP_INVALID_ARGUMENT;
  if (n_streams > 0 && (!src_offsets || !dst_sizes || !status)) return QHIP_INVALID_ARGUMENT;
  if (n_streams >= (1 << 24)) return QHIP_INVALID_ARGUMENT;
  return guarded(ctx, [&] { snappy_decode(ctx, (const uint8_t*)bytes, n_bytes, src_offsets, dst_sizes, n_streams, (uint8_t*)out, out_bytes, status); });
}

int qhip_zstd_decode(qhip_ctx* ctx, const void* bytes, int64_t n_bytes, const int64_t* src_offsets, const int64_t* dst_sizes, int64_t n_streams, void* out,
                     int64_t out_bytes, int32_t* status) {
  if (!ctx || n_bytes < 0 || (n_bytes > 0 && !bytes) || n_streams < 0 || out_bytes < 0 || (out_bytes > 0 && !out)) return QHIP_INVALID_ARGUMENT;
  if (n_streams > 0 && (!src_offsets || !dst_sizes || !status)) return QHIP_INVALID_ARGUMENT;
  if (n_streams >= (1 << 24)) return QHIP_INVALID_ARGUMENT;
  return guarded(ctx, [&] { zstd_decode(ctx, (const uint8_t*)bytes, n_bytes, src_offsets, dst_sizes, n_streams, (uint8_t*)out, out_bytes, status); });
}

int qhip_gzip_decode(qhip_ctx* ctx, const void* bytes, int64_t n_bytes, const int64_t* src_offsets, const int64_t* dst_sizes, int64_t n_streams, void* out,
                     int64_t out_bytes, int32_t* status) {
  if (!ctx || n_bytes < 0 || (n_bytes > 0 && !bytes) || n_streams < 0 || out_bytes < 0 || (out_bytes > 0 && !out)) return QHIP_INVALID_ARGUMENT;
  if (n_streams > 0 && (!src_offsets || !dst_sizes || !status)) return QHIP_INVALID_ARGUMENT;
  if (n_streams >= (1 << 24)) return QHIP_INVALID_ARGUMENT;
  return guarded(ctx, [&] { gzip_decode(ctx, (const uint8_t*)bytes, n_bytes, src_offsets, dst_sizes, n_streams, (uint8_t*)out, out_bytes, status); });
}

int qhip_lz4_decode(qhip_ctx* ctx, const void* bytes, int64_t n_bytes, const int64_t* src_offsets, const int64_t* dst_sizes, int64_t n_streams, void* out,
                    int64_t out_bytes, int32_t* status) {
  if (!ctx || n_bytes < 0 || (n_bytes > 0 && !bytes) || n_streams < 0 || out_bytes < 0 || (out_bytes > 0 && !out)) return QHIP_INVALID_ARGUMENT;
  if (n_streams > 0 && (!src_offsets || !dst_sizes || !status)) return QHIP_INVALID_ARGUMENT;
  if (n_streams >= (1 << 24)) return QHIP_INVALID_ARGUMENT;
  return guarded(ctx, [&] { lz4_decode(ctx, (const uint8_t*)bytes, n_bytes, src_offsets, dst_sizes, n_streams, (uint8_t*)out, out_bytes, status); });
}

}  // extern "C"
