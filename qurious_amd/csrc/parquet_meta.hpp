// parquet_meta.hpp — the host half of the device Parquet decoder that needs no device (parquet.cpp includes it; so does
// tests/cpp/parquet_tests.cpp, which runs it under the sanitizers): a bounds-checked Thrift compact-protocol reader, the footer
// (FileMetaData) and page headers decoded as far as they are used, the match of a column's physical type and annotation against
// its Arrow type, and the page walk that turns the projected chunks into a page table and, at format level 2, the pages of Snappy
// chunks into an unpack table with their slots in the unpack area and, at encoding set 2, data pages V2 and the DELTA_* pages into
// a delta table with their slots in the decoded area and, at codec set 2, the pages of ZSTD chunks into a second unpack table
// with slots in the same unpack area and, with the gzip switch on, the pages of GZIP chunks into a third and, with the lz4
// switch on, the blocks of LZ4_RAW and legacy LZ4 pages into a fourth and, with the DELTA_BYTE_ARRAY switch on, the pages of
// that encoding into the delta table and a fill table. Plain C++, no Arrow, no HIP.
// A ZSTD page's frame header and block headers are checked here (qh_zstd_check_frame) before anything is reserved; its content
// checksum, where it has one, is skipped and not verified. A GZIP page's member header and ISIZE are checked here
// (qh_gzip_check_member); its CRC32 is skipped and not verified either. An LZ4 page's size is checked against the 255x bound
// (qh_lz4_check_sizes); a page of the legacy id is split into Hadoop's frames where they tile it (qh_lz4_hadoop_scan).
// Every offset, length and count comes from the file and is checked before it is followed: a violation throws PqNeedsHost.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "qhip.h"
#include "device/qhip_parquet.inc"
#include "device/qhip_snappy.inc"
#include "device/qhip_delta.inc"
#include "device/qhip_dba.inc"
#include "device/qhip_zstd.inc"
#include "device/qhip_inflate.inc"
#include "device/qhip_lz4.inc"

static_assert(QH_PQ_R_SNAPPY_PREAMBLE == QH_PQ_R_SNAPPY_BASE + QH_SNAP_E_PREAMBLE && QH_PQ_R_SNAPPY_OFFSET == QH_PQ_R_SNAPPY_BASE + QH_SNAP_E_OFFSET &&
                  QH_PQ_R_V2_UNCOMPRESSED == QH_PQ_R_SNAPPY_BASE + QH_SNAP_E_COUNT,
              "the Snappy reasons follow the decoder's error codes, the reasons of encoding set 2 follow them");

static_assert(QH_PQ_R_ZSTD_BASE == QH_PQ_R_DELTA_LENGTH && QH_PQ_R_ZSTD_FRAME == QH_PQ_R_ZSTD_BASE + QH_ZSTD_E_FRAME &&
                  QH_PQ_R_ZSTD_OFFSET == QH_PQ_R_ZSTD_BASE + QH_ZSTD_E_OFFSET && QH_PQ_R_GZIP_MEMBER == QH_PQ_R_ZSTD_BASE + QH_ZSTD_E_COUNT,
              "the Zstd reasons follow the reasons of encoding set 2 and the decoder's error codes");

static_assert(QH_PQ_R_GZIP_BASE == QH_PQ_R_ZSTD_OFFSET && QH_PQ_R_GZIP_MEMBER == QH_PQ_R_GZIP_BASE + QH_INFL_E_MEMBER &&
                  QH_PQ_R_GZIP_TRAILER == QH_PQ_R_GZIP_BASE + QH_INFL_E_TRAILER && QH_PQ_R_LZ4_SIZE == QH_PQ_R_GZIP_BASE + QH_INFL_E_COUNT,
              "the Gzip reasons follow the Zstd reasons and the decoder's error codes");

static_assert(QH_PQ_R_LZ4_BASE == QH_PQ_R_GZIP_TRAILER && QH_PQ_R_LZ4_SIZE == QH_PQ_R_LZ4_BASE + QH_LZ4_E_SIZE &&
                  QH_PQ_R_LZ4_END == QH_PQ_R_LZ4_BASE + QH_LZ4_E_END && QH_PQ_R_DBA_PREFIX == QH_PQ_R_LZ4_BASE + QH_LZ4_E_COUNT,
              "the LZ4 reasons follow the Gzip reasons and the decoder's error codes");
static_assert(QH_PQ_R_DBA_WIDTH == QH_PQ_R_DBA_PREFIX + 2 && QH_PQ_R_COUNT == QH_PQ_R_DBA_WIDTH + 1, "the DELTA_BYTE_ARRAY reasons follow the LZ4 reasons");

namespace qhip_pq {

struct PqNeedsHost {
  int reason;
  int64_t row_group, column, page;   // -1: does not apply
};
[[noreturn]] inline void needs_host(int reason, int64_t rg = -1, int64_t col = -1, int64_t page = -1) { throw PqNeedsHost{reason, rg, col, page}; }

inline std::string needs_host_text(const PqNeedsHost& e) {
  std::string s = std::string("Parquet needs the host path: ") + qh_pq_reason_text((unsigned)e.reason);
  if (e.row_group >= 0) s += ", row group " + std::to_string(e.row_group);
  if (e.column >= 0) s += ", column " + std::to_string(e.column);
  if (e.page >= 0) s += ", page " + std::to_string(e.page);
  return s;
}

// ---------------------------------------------------------------- Thrift compact protocol
enum { T_STOP = 0, T_TRUE = 1, T_FALSE = 2, T_BYTE = 3, T_I16 = 4, T_I32 = 5, T_I64 = 6, T_DOUBLE = 7, T_BINARY = 8, T_LIST = 9, T_SET = 10, T_MAP = 11, T_STRUCT = 12 };

struct Thrift {
  const uint8_t* p;
  uint64_t n, pos = 0;
  Thrift(const uint8_t* bytes, uint64_t len) : p(bytes), n(len) {}
  [[noreturn]] static void bad() { needs_host(QH_PQ_R_CORRUPT); }
  uint8_t byte() { if (pos >= n) bad(); return p[pos++]; }
  uint64_t varint() {
    uint64_t v = 0;
    for (int shift = 0; shift < 70; shift += 7) {
      const uint8_t b = byte();
      v |= (uint64_t)(b & 0x7F) << (shift < 64 ? shift : 63);
      if (!(b & 0x80)) return v;
    }
    bad();
  }
  int64_t zigzag() { const uint64_t v = varint(); return (int64_t)(v >> 1) ^ -(int64_t)(v & 1); }
  // the next field of a struct: false at the stop byte. `last` carries the previous field id (deltas).
  bool field(int& last, int& id, int& type) {
    const uint8_t b = byte();
    if (b == 0) return false;
    type = b & 0x0F;
    const int delta = b >> 4;
    id = delta ? last + delta : (int)zigzag();
    last = id;
    return true;
  }
  void binary(const uint8_t*& s, uint64_t& len) {
    len = varint();
    if (len > n - pos) bad();
    s = p + pos;
    pos += len;
  }
  std::string string() { const uint8_t* s; uint64_t len; binary(s, len); return std::string((const char*)s, (size_t)len); }
  // a list's element type and size; every element takes at least one byte, so a size beyond the rest of the bytes is refused
  // before anything is reserved for it
  void list(int& elem, uint64_t& size) {
    const uint8_t b = byte();
    elem = b & 0x0F;
    size = b >> 4;
    if (size == 15) size = varint();
    if (size > n - pos) bad();
  }
  void skip(int type, int depth, bool in_container = false) {
    if (depth > 24) bad();
    switch (type) {
      case T_TRUE: case T_FALSE: if (in_container) (void)byte(); break;   // (a struct field carries its Boolean in the type)
      case T_BYTE: (void)byte(); break;
      case T_I16: case T_I32: case T_I64: (void)varint(); break;
      case T_DOUBLE: if (n - pos < 8) bad(); pos += 8; break;
      case T_BINARY: { const uint8_t* s; uint64_t len; binary(s, len); break; }
      case T_LIST: case T_SET: {
        int elem; uint64_t size;
        list(elem, size);
        for (uint64_t i = 0; i < size; ++i) skip(elem, depth + 1, true);
        break;
      }
      case T_MAP: {
        const uint64_t size = varint();
        if (size > n - pos) bad();
        if (size) {
          const uint8_t kv = byte();
          for (uint64_t i = 0; i < size; ++i) { skip(kv >> 4, depth + 1, true); skip(kv & 0x0F, depth + 1, true); }
        }
        break;
      }
      case T_STRUCT: {
        int last = 0, id, t;
        while (field(last, id, t)) skip(t, depth + 1);
        break;
      }
      default: bad();
    }
  }
  int64_t integer(int type) { if (type != T_I16 && type != T_I32 && type != T_I64 && type != T_BYTE) bad(); return type == T_BYTE ? (int64_t)(int8_t)byte() : zigzag(); }
  bool boolean(int type) { if (type != T_TRUE && type != T_FALSE) bad(); return type == T_TRUE; }
};

// ---------------------------------------------------------------- the parts of the metadata that are used
enum { PT_BOOLEAN = 0, PT_INT32 = 1, PT_INT64 = 2, PT_INT96 = 3, PT_FLOAT = 4, PT_DOUBLE = 5, PT_BYTE_ARRAY = 6, PT_FLBA = 7 };
enum { ENC_PLAIN = 0, ENC_PLAIN_DICTIONARY = 2, ENC_RLE = 3, ENC_BIT_PACKED = 4, ENC_DELTA_BINARY_PACKED = 5, ENC_DELTA_LENGTH_BYTE_ARRAY = 6, ENC_DELTA_BYTE_ARRAY = 7,
       ENC_RLE_DICTIONARY = 8, ENC_BYTE_STREAM_SPLIT = 9 };
enum { PAGE_DATA = 0, PAGE_INDEX = 1, PAGE_DICTIONARY = 2, PAGE_DATA_V2 = 3 };
enum { CODEC_UNCOMPRESSED = 0, CODEC_SNAPPY = 1, CODEC_GZIP = 2, CODEC_LZ4 = 5, CODEC_ZSTD = 6, CODEC_LZ4_RAW = 7 };
enum { L_NONE = 0, L_STRING, L_DECIMAL, L_DATE, L_TIMESTAMP, L_INT, L_OTHER };

struct SchemaElem {
  int type = -1, type_length = 0, repetition = -1, num_children = 0, converted = -1, scale = 0, precision = 0;
  std::string name;
  int logical = L_NONE;             // the annotation, from logicalType where present, else from converted_type
  int bits = 0, is_signed = 0;      // L_INT
  int unit = 0, utc = 0;            // L_TIMESTAMP: 1 ms, 2 us, 3 ns
};
struct Chunk {
  bool has_file_path = false, has_meta = false;
  int type = -1, codec = -1;
  int64_t num_values = -1, total_compressed = -1, data_off = -1, dict_off = -1;
};
struct RowGroup { std::vector<Chunk> cols; int64_t num_rows = -1; };
struct Footer { std::vector<SchemaElem> schema; int64_t num_rows = -1; std::vector<RowGroup> groups; };
struct PageHeader {
  int type = -1;
  int64_t uncompressed = -1, compressed = -1;
  bool has_data = false, has_dict = false;
  int64_t num_values = -1, encoding = -1, def_encoding = -1;   // of the data or dictionary page header
  // DataPageHeaderV2 (read at encoding set 2 only): its num_values and encoding stand above where the page's type is DATA_PAGE_V2
  bool has_v2 = false, is_compressed = true;
  int64_t num_nulls = -1, num_rows = -1, def_bytes = -1, rep_bytes = -1;
  uint64_t header_bytes = 0;
};

inline void read_logical_type(Thrift& t, SchemaElem& e) {
  int last = 0, id, ty;
  while (t.field(last, id, ty)) {
    if (ty != T_STRUCT) { t.skip(ty, 1); continue; }
    int l2 = 0, id2, ty2;
    switch (id) {
      case 1: e.logical = L_STRING; break;
      case 5: e.logical = L_DECIMAL; break;
      case 6: e.logical = L_DATE; break;
      case 8: e.logical = L_TIMESTAMP; e.utc = 1; e.unit = 0; break;
      case 10: e.logical = L_INT; break;
      default: e.logical = L_OTHER; break;
    }
    while (t.field(l2, id2, ty2)) {
      if (id == 5 && id2 == 1) e.scale = (int)t.integer(ty2);
      else if (id == 5 && id2 == 2) e.precision = (int)t.integer(ty2);
      else if (id == 8 && id2 == 1) e.utc = t.boolean(ty2) ? 1 : 0;
      else if (id == 8 && id2 == 2 && ty2 == T_STRUCT) {
        int l3 = 0, id3, ty3;
        while (t.field(l3, id3, ty3)) { e.unit = id3; t.skip(ty3, 3); }
      } else if (id == 10 && id2 == 1) e.bits = (int)t.integer(ty2);
      else if (id == 10 && id2 == 2) e.is_signed = t.boolean(ty2) ? 1 : 0;
      else t.skip(ty2, 2);
    }
  }
}

inline SchemaElem read_schema_elem(Thrift& t) {
  SchemaElem e;
  bool has_logical = false;
  int last = 0, id, ty;
  while (t.field(last, id, ty)) {
    switch (id) {
      case 1: e.type = (int)t.integer(ty); break;
      case 2: e.type_length = (int)t.integer(ty); break;
      case 3: e.repetition = (int)t.integer(ty); break;
      case 4: if (ty != T_BINARY) Thrift::bad(); e.name = t.string(); break;
      case 5: e.num_children = (int)t.integer(ty); break;
      case 6: e.converted = (int)t.integer(ty); break;
      case 7: if (!has_logical) e.scale = (int)t.integer(ty); else (void)t.integer(ty); break;
      case 8: if (!has_logical) e.precision = (int)t.integer(ty); else (void)t.integer(ty); break;
      case 10: if (ty != T_STRUCT) Thrift::bad(); read_logical_type(t, e); has_logical = true; break;
      default: t.skip(ty, 1); break;
    }
  }
  if (!has_logical && e.converted >= 0) {
    const int c = e.converted;
    if (c == 0) e.logical = L_STRING;
    else if (c == 5) e.logical = L_DECIMAL;
    else if (c == 6) e.logical = L_DATE;
    else if (c == 9 || c == 10) { e.logical = L_TIMESTAMP; e.utc = 1; e.unit = c - 8; }   // (legacy annotation: Arrow reads these as UTC)
    else if (c >= 11 && c <= 14) { e.logical = L_INT; e.is_signed = 0; e.bits = 8 << (c - 11); }
    else if (c >= 15 && c <= 18) { e.logical = L_INT; e.is_signed = 1; e.bits = 8 << (c - 15); }
    else e.logical = L_OTHER;
  }
  return e;
}

inline Chunk read_chunk(Thrift& t) {
  Chunk c;
  int last = 0, id, ty;
  while (t.field(last, id, ty)) {
    if (id == 1 && ty == T_BINARY) { (void)t.string(); c.has_file_path = true; }
    else if (id == 3 && ty == T_STRUCT) {
      c.has_meta = true;
      int l2 = 0, id2, ty2;
      while (t.field(l2, id2, ty2)) {
        switch (id2) {
          case 1: c.type = (int)t.integer(ty2); break;
          case 4: c.codec = (int)t.integer(ty2); break;
          case 5: c.num_values = t.integer(ty2); break;
          case 7: c.total_compressed = t.integer(ty2); break;
          case 9: c.data_off = t.integer(ty2); break;
          case 11: c.dict_off = t.integer(ty2); break;
          default: t.skip(ty2, 2); break;   // (encodings, path_in_schema, key_value_metadata, Statistics, ...)
        }
      }
    } else t.skip(ty, 1);
  }
  return c;
}

inline Footer read_footer(const uint8_t* bytes, uint64_t len) {
  Thrift t(bytes, len);
  Footer f;
  int last = 0, id, ty;
  while (t.field(last, id, ty)) {
    if (id == 2 && ty == T_LIST) {
      int elem; uint64_t size;
      t.list(elem, size);
      if (elem != T_STRUCT) Thrift::bad();
      for (uint64_t i = 0; i < size; ++i) f.schema.push_back(read_schema_elem(t));
    } else if (id == 3) f.num_rows = t.integer(ty);
    else if (id == 4 && ty == T_LIST) {
      int elem; uint64_t size;
      t.list(elem, size);
      if (elem != T_STRUCT) Thrift::bad();
      for (uint64_t i = 0; i < size; ++i) {
        RowGroup g;
        int l2 = 0, id2, ty2;
        while (t.field(l2, id2, ty2)) {
          if (id2 == 1 && ty2 == T_LIST) {
            int e2; uint64_t s2;
            t.list(e2, s2);
            if (e2 != T_STRUCT) Thrift::bad();
            for (uint64_t k = 0; k < s2; ++k) g.cols.push_back(read_chunk(t));
          } else if (id2 == 3) g.num_rows = t.integer(ty2);
          else t.skip(ty2, 2);
        }
        f.groups.push_back(std::move(g));
      }
    } else t.skip(ty, 1);
  }
  return f;
}

// one page header in bytes[0 .. len): nothing behind len is read. v2: decode DataPageHeaderV2 as well (else it is skipped); a
// page of another type that carries one too is answered as without it
inline PageHeader read_page_header(const uint8_t* bytes, uint64_t len, bool v2 = false) {
  Thrift t(bytes, len);
  PageHeader h;
  int64_t v2_num_values = -1, v2_encoding = -1;
  int last = 0, id, ty;
  while (t.field(last, id, ty)) {
    if (id == 1) h.type = (int)t.integer(ty);
    else if (id == 2) h.uncompressed = t.integer(ty);
    else if (id == 3) h.compressed = t.integer(ty);
    else if ((id == 5 || id == 7) && ty == T_STRUCT) {
      (id == 5 ? h.has_data : h.has_dict) = true;
      int l2 = 0, id2, ty2;
      while (t.field(l2, id2, ty2)) {
        if (id2 == 1) h.num_values = t.integer(ty2);
        else if (id2 == 2) h.encoding = t.integer(ty2);
        else if (id2 == 3 && id == 5) h.def_encoding = t.integer(ty2);
        else t.skip(ty2, 2);   // (Statistics, is_sorted, the repetition level encoding: a flat column has none)
      }
    } else if (v2 && id == 8 && ty == T_STRUCT) {
      h.has_v2 = true;
      int l2 = 0, id2, ty2;
      while (t.field(l2, id2, ty2)) {
        switch (id2) {
          case 1: v2_num_values = t.integer(ty2); break;
          case 2: h.num_nulls = t.integer(ty2); break;
          case 3: h.num_rows = t.integer(ty2); break;
          case 4: v2_encoding = t.integer(ty2); break;
          case 5: h.def_bytes = t.integer(ty2); break;
          case 6: h.rep_bytes = t.integer(ty2); break;
          case 7: h.is_compressed = t.boolean(ty2); break;
          default: t.skip(ty2, 2); break;   // (Statistics)
        }
      }
    } else t.skip(ty, 1);
  }
  if (h.has_v2 && h.type == PAGE_DATA_V2) { h.num_values = v2_num_values; h.encoding = v2_encoding; }
  h.header_bytes = t.pos;
  return h;
}

// ---------------------------------------------------------------- types
struct ArrowType { int id = -1; int precision = 0, scale = 0; };   // id: a QHIP_* dtype id; -1: a type the C ABI does not carry

struct ColPlan {
  uint32_t phys = 0, flba = 0, width = 0, narrow = 0;
  bool optional = true, utf8 = false, boolean = false;
  uint64_t dict_entries = 0;   // Utf8: entries of all its dictionary pages
  bool dba = false;            // Utf8: a DELTA_BYTE_ARRAY page among its pages (the column gets a per-row prefix array)
};

// does the file store Arrow type `a` in this leaf the way the device decodes? Fills the column's physical description.
inline bool match_type(const SchemaElem& e, const ArrowType& a, ColPlan& c) {
  const int L = e.logical;
  auto is_int = [&](int bits, int sg) { return L == L_INT && e.bits == bits && e.is_signed == sg; };
  switch (a.id) {
    case QHIP_BOOL: c.phys = QH_PQ_P_BOOL; c.boolean = true; return e.type == PT_BOOLEAN && L == L_NONE;
    case QHIP_INT8: c.phys = QH_PQ_P_32; c.width = 1; c.narrow = 1; return e.type == PT_INT32 && is_int(8, 1);
    case QHIP_INT16: c.phys = QH_PQ_P_32; c.width = 2; c.narrow = 1; return e.type == PT_INT32 && is_int(16, 1);
    case QHIP_UINT8: c.phys = QH_PQ_P_32; c.width = 1; c.narrow = 2; return e.type == PT_INT32 && is_int(8, 0);
    case QHIP_UINT16: c.phys = QH_PQ_P_32; c.width = 2; c.narrow = 2; return e.type == PT_INT32 && is_int(16, 0);
    case QHIP_INT32: c.phys = QH_PQ_P_32; c.width = 4; return e.type == PT_INT32 && (L == L_NONE || is_int(32, 1));
    case QHIP_UINT32: c.phys = QH_PQ_P_32; c.width = 4; return e.type == PT_INT32 && is_int(32, 0);
    case QHIP_DATE32: c.phys = QH_PQ_P_32; c.width = 4; return e.type == PT_INT32 && L == L_DATE;
    case QHIP_FLOAT32: c.phys = QH_PQ_P_32; c.width = 4; return e.type == PT_FLOAT && L == L_NONE;
    case QHIP_INT64: c.phys = QH_PQ_P_64; c.width = 8; return e.type == PT_INT64 && (L == L_NONE || is_int(64, 1));
    case QHIP_UINT64: c.phys = QH_PQ_P_64; c.width = 8; return e.type == PT_INT64 && is_int(64, 0);
    case QHIP_FLOAT64: c.phys = QH_PQ_P_64; c.width = 8; return e.type == PT_DOUBLE && L == L_NONE;
    case QHIP_TIMESTAMP_MS: case QHIP_TIMESTAMP_US: case QHIP_TIMESTAMP_NS:
      c.phys = QH_PQ_P_64; c.width = 8;
      return e.type == PT_INT64 && L == L_TIMESTAMP && !e.utc && e.unit == a.id - QHIP_TIMESTAMP_MS + 1;
    case QHIP_UTF8: c.phys = QH_PQ_P_BYTES; c.utf8 = true; return e.type == PT_BYTE_ARRAY && L == L_STRING;
    case QHIP_DECIMAL128:
      c.width = 16;
      if (L != L_DECIMAL || e.precision != a.precision || e.scale != a.scale || a.precision < 1 || a.precision > 38) return false;
      if (e.type == PT_INT32) { c.phys = QH_PQ_P_32; return a.precision <= 9; }
      if (e.type == PT_INT64) { c.phys = QH_PQ_P_64; return a.precision <= 18; }
      c.phys = QH_PQ_P_FLBA; c.flba = (uint32_t)e.type_length;
      return e.type == PT_FLBA && e.type_length >= 1 && e.type_length <= 16;
    default: return false;
  }
}

// ---------------------------------------------------------------- the plan: which bytes to upload, which pages they hold
struct Range { uint64_t file_off, bytes, buf_off; };
struct PageWhere { int64_t row_group, column, page; };

struct Plan {
  uint64_t num_rows = 0;
  uint64_t upload_bytes = 0;
  std::vector<ColPlan> cols;          // in output order
  std::vector<Range> ranges;          // the projected chunks, one behind the other in the upload buffer
  std::vector<qh_pq_page> pages;      // (`col`: index into cols; positions in the upload buffer)
  std::vector<PageWhere> where;       // for the message: what pages[k] is in the file
  // format level 2: the pages of the Snappy chunks. The device buffer is the uploaded chunks, then (16-byte aligned, at
  // unpack_base) the unpack area: one 16-byte aligned slot of uncompressed_page_size bytes per entry. Empty at level 1.
  std::vector<qh_pq_unpack> unpack;
  uint64_t unpack_base = 0, unpack_bytes = 0;
  // codec set 2: the pages of the ZSTD chunks (k_pq_unzstd), a table of their own with slots in the same unpack area, in the
  // order of the pages. `start`: where the frame's first block header lies. Empty at codec set 1.
  std::vector<qh_pq_unpack> unzstd;
  // the gzip switch: the pages of the GZIP chunks (k_pq_ungzip), a third table with slots in the same unpack area. `start`:
  // where the member's first DEFLATE block lies. Empty with the switch off.
  std::vector<qh_pq_unpack> ungzip;
  // the lz4 switch: the blocks of the LZ4_RAW and legacy LZ4 chunks (k_pq_unlz4), a fourth table. A page is one bare block and
  // one entry, or, under the legacy id where Hadoop's frames tile it, one entry per frame: each with its own source range and
  // its own slice of the page's one slot in the same unpack area. Empty with the switch off.
  std::vector<qh_pq_unpack> unlz4;
  // encoding set 2: the DELTA_BINARY_PACKED pages (k_pq_delta). The dense values of one get a 16-byte aligned slot of
  // num_values x width bytes in the decoded area, which lies behind the unpack area (at decoded_base) in the same buffer;
  // DELTA_LENGTH_BYTE_ARRAY lengths become entries of their column and need no slot. has_ext: some page is for k_pq_values_ext.
  std::vector<qh_pq_dstream> delta;
  uint64_t decoded_base = 0, decoded_bytes = 0;
  bool has_ext = false;
  // the DELTA_BYTE_ARRAY switch: such a page is an entry of `delta` marked QH_PQ_DS_DBA and a job for k_pq_dba_fill. A
  // FIXED_LEN_BYTE_ARRAY page (fill_values, value space, before the host wait) gets a slot in the decoded area: num_values x
  // width bytes for its dense values, where k_pq_values_ext reads it as PLAIN (its enc is QH_PQ_ENC_DELTA), and behind them,
  // 16-byte aligned, num_values x 16 bytes for its entries. A Utf8 page (fill_rows, row space, after the wait) needs no slot.
  std::vector<qh_pq_fill> fill_values, fill_rows;
  uint64_t packed_bytes() const { return unpack.empty() && unzstd.empty() && ungzip.empty() && unlz4.empty() ? upload_bytes : unpack_base + unpack_bytes; }
  uint64_t buffer_bytes() const { return decoded_bytes ? decoded_base + decoded_bytes : packed_bytes(); }
};

// names: the schema's field names (checked against the file's when given). types: the Arrow type of EVERY field. proj: the
// fields to decode, in output order. level: the format level (qhip_ctx_set_parquet_format); 2 admits SNAPPY chunks. encodings:
// the encoding set (qhip_ctx_set_parquet_encodings); 2 admits data pages V2, RLE Boolean values, BYTE_STREAM_SPLIT,
// DELTA_BINARY_PACKED and DELTA_LENGTH_BYTE_ARRAY. At set 1 nothing below differs from what it was before the set existed.
// codecs: the codec set (qhip_ctx_set_parquet_codecs); 2 admits ZSTD chunks, whatever the level, which goes on governing SNAPPY.
// At set 1 nothing below differs from what it was before the set existed either. gzip: the gzip switch
// (qhip_ctx_set_parquet_gzip); 1 admits GZIP chunks, whatever the other three say; at 0 nothing below differs. lz4: the lz4
// switch (qhip_ctx_set_parquet_lz4); 1 admits LZ4_RAW chunks (codec 7: a page is one bare LZ4 block) and chunks of the legacy id
// (codec 5: Hadoop's frames where they tile the page, one bare block otherwise), whatever the other four say; at 0 nothing differs.
// dba: the DELTA_BYTE_ARRAY switch (qhip_ctx_set_parquet_delta_byte_array); 1 admits data pages of that encoding in Utf8 columns
// and in the FIXED_LEN_BYTE_ARRAY decimals, whatever the other five say (a V2 page still needs encoding set 2, a compressed chunk
// its codec's switch); at 0 nothing differs.
inline Plan plan_file(const uint8_t* file, uint64_t n, const std::vector<std::string>* names, const std::vector<ArrowType>& types, const std::vector<int32_t>& proj,
                      int level = 1, int encodings = 1, int codecs = 1, int gzip = 0, int lz4 = 0, int dba = 0) {
  const bool set2 = encodings >= 2;
  if (n >= 4 && memcmp(file, "PARE", 4) == 0) needs_host(QH_PQ_R_ENCRYPTED);
  if (n >= 4 && memcmp(file + n - 4, "PARE", 4) == 0) needs_host(QH_PQ_R_ENCRYPTED);
  if (n < 12 || memcmp(file, "PAR1", 4) != 0 || memcmp(file + n - 4, "PAR1", 4) != 0) needs_host(QH_PQ_R_MAGIC);
  const uint64_t flen = qh_pq_le32(file + n - 8);
  if (flen > n - 12) needs_host(QH_PQ_R_CORRUPT);
  const uint64_t fstart = n - 8 - flen;   // data lies in [4, fstart)
  const Footer f = read_footer(file + fstart, flen);

  // ---- the schema: a root and leaves, nothing else
  if (f.schema.empty()) needs_host(QH_PQ_R_CORRUPT);
  for (size_t k = 1; k < f.schema.size(); ++k) {
    const SchemaElem& e = f.schema[k];
    if (e.num_children > 0 || e.type < 0) needs_host(QH_PQ_R_NESTED);
    if (e.repetition == 2) needs_host(QH_PQ_R_REPEATED);
    if (e.repetition != 0 && e.repetition != 1) needs_host(QH_PQ_R_CORRUPT);
  }
  const size_t nfields = f.schema.size() - 1;
  if ((size_t)f.schema[0].num_children != nfields) needs_host(QH_PQ_R_NESTED);
  if (nfields != types.size()) needs_host(QH_PQ_R_SCHEMA);
  if (names) for (size_t k = 0; k < nfields; ++k) if (f.schema[k + 1].name != (*names)[k]) needs_host(QH_PQ_R_SCHEMA);
  if (proj.size() > QH_PQ_MAX_COLS) needs_host(QH_PQ_R_TOO_MANY_COLUMNS);

  Plan plan;
  for (size_t k = 0; k < proj.size(); ++k) {
    ColPlan c;
    const SchemaElem& e = f.schema[(size_t)proj[k] + 1];
    if (e.type == PT_INT96 || !match_type(e, types[(size_t)proj[k]], c)) needs_host(QH_PQ_R_TYPE, -1, proj[k]);
    c.optional = e.repetition == 1;
    plan.cols.push_back(c);
  }

  // ---- rows
  uint64_t rows = 0;
  for (const RowGroup& g : f.groups) {
    if (g.num_rows < 0 || (uint64_t)g.num_rows > 0xFFFFFFFFull) needs_host(g.num_rows < 0 ? QH_PQ_R_CORRUPT : QH_PQ_R_TOO_MANY_ROWS);
    rows += (uint64_t)g.num_rows;
    if (rows >= 0xFFFFFFFFull) needs_host(QH_PQ_R_TOO_MANY_ROWS);
  }
  if (f.num_rows < 0 || (uint64_t)f.num_rows != rows) needs_host(QH_PQ_R_CORRUPT);
  if (rows == 0) needs_host(QH_PQ_R_NO_ROWS);
  plan.num_rows = rows;

  // ---- the page walk: one header per page of every projected chunk
  std::vector<uint8_t> in_unpack;   // per page: 1 its pos, 2 its dict_pos is relative to the unpack area
  uint64_t first_row = 0;
  for (size_t gi = 0; gi < f.groups.size(); ++gi) {
    const RowGroup& g = f.groups[gi];
    if (g.num_rows == 0) continue;
    if (g.cols.size() != nfields) needs_host(QH_PQ_R_CORRUPT, (int64_t)gi);
    for (size_t k = 0; k < proj.size(); ++k) {
      const Chunk& ch = g.cols[(size_t)proj[k]];
      ColPlan& cp = plan.cols[k];
      const int64_t G = (int64_t)gi, C = proj[k];
      if (ch.has_file_path) needs_host(QH_PQ_R_FILE_PATH, G, C);
      if (!ch.has_meta || ch.type != f.schema[(size_t)proj[k] + 1].type) needs_host(QH_PQ_R_CORRUPT, G, C);
      const bool snappy = level >= 2 && ch.codec == CODEC_SNAPPY;
      const bool zstd = codecs >= 2 && ch.codec == CODEC_ZSTD;
      const bool gz = gzip >= 1 && ch.codec == CODEC_GZIP;
      const bool lz = lz4 >= 1 && (ch.codec == CODEC_LZ4_RAW || ch.codec == CODEC_LZ4);
      const bool packed = snappy || zstd || gz || lz;
      if (ch.codec != CODEC_UNCOMPRESSED && !packed) needs_host(QH_PQ_R_CODEC, G, C);
      const int64_t start = ch.dict_off > 0 ? ch.dict_off : ch.data_off;
      if (start < 4 || ch.total_compressed < 0 || (uint64_t)start > fstart || (uint64_t)ch.total_compressed > fstart - (uint64_t)start) needs_host(QH_PQ_R_CORRUPT, G, C);
      const uint64_t cbytes = (uint64_t)ch.total_compressed, cbuf = plan.upload_bytes;
      plan.ranges.push_back(Range{(uint64_t)start, cbytes, cbuf});
      plan.upload_bytes += cbytes;
      const uint8_t* chunk = file + start;
      const uint32_t pw = qh_pq_phys_bytes(cp.phys, cp.flba);
      const int ptype = ch.type;   // (the physical type: INT32 and FLOAT share a layout, DELTA_BINARY_PACKED is for integers)
      uint64_t pos = 0, got = 0, dict_pos = 0, dict_ent = 0;
      uint32_t dict_size = 0, dict_n = 0;
      bool have_dict = false, seen_data = false;
      for (int64_t pageno = 0; got < (uint64_t)g.num_rows; ++pageno) {
        if (pos >= cbytes) needs_host(QH_PQ_R_NUM_VALUES, G, C, pageno);
        PageHeader h;
        try { h = read_page_header(chunk + pos, cbytes - pos, set2); } catch (const PqNeedsHost& e) { needs_host(e.reason, G, C, pageno); }
        const uint64_t payload = pos + h.header_bytes;
        if (h.compressed < 0 || (!packed && h.compressed != h.uncompressed) || (uint64_t)h.compressed > cbytes - payload || h.compressed > 0x7FFFFFFF)
          needs_host(QH_PQ_R_CORRUPT, G, C, pageno);
        uint32_t size = (uint32_t)h.compressed;   // of the page as the device's passes see it
        qh_pq_page pg;
        memset(&pg, 0, sizeof pg);
        pg.pos = cbuf + payload; pg.col = (uint32_t)k;
        // encoding set 2, a data page V2: its levels lie uncompressed in front of the values, which alone are the page's payload
        // for the codec and for the passes below. `lev`: the level bytes.
        const bool v2 = set2 && h.type == PAGE_DATA_V2;
        uint32_t lev = 0;
        bool unpacked = packed;
        if (v2) {
          if (!h.has_v2 || h.num_values < 0 || h.num_nulls < 0 || h.num_rows < 0 || h.def_bytes < 0 || h.rep_bytes < 0) needs_host(QH_PQ_R_CORRUPT, G, C, pageno);
          if (h.num_rows != h.num_values) needs_host(QH_PQ_R_V2_ROWS, G, C, pageno);
          if (h.rep_bytes != 0) needs_host(QH_PQ_R_V2_REPETITION, G, C, pageno);
          if (!cp.optional && (h.def_bytes != 0 || h.num_nulls != 0)) needs_host(QH_PQ_R_V2_LEVELS, G, C, pageno);
          if (h.def_bytes > h.compressed || h.uncompressed < 0 || h.def_bytes > h.uncompressed) needs_host(QH_PQ_R_V2_LEVELS, G, C, pageno);
          if (h.num_nulls > h.num_values) needs_host(QH_PQ_R_V2_NULLS, G, C, pageno);
          // (a writer may leave a page's values uncompressed in a compressed chunk, as Arrow does where the codec does not help:
          // they are read where they lie in the upload, as in an uncompressed chunk)
          if (packed && !h.is_compressed) {
            if (h.compressed != h.uncompressed) needs_host(QH_PQ_R_V2_UNCOMPRESSED, G, C, pageno);
            unpacked = false;
          }
          lev = (uint32_t)h.def_bytes;
          pg.flags = QH_PQ_F_V2; pg.lev_pos = cbuf + payload; pg.lev_size = lev; pg.num_nulls = (uint32_t)(h.num_nulls > 0xFFFFFFFFll ? 0xFFFFFFFFll : h.num_nulls);
          pg.pos = cbuf + payload + lev;
          size -= lev;
          if (packed && h.compressed == (int64_t)lev && h.uncompressed == (int64_t)lev) unpacked = false;   // (an empty values part: nothing to unpack)
        }
        if (unpacked) {
          // the page is unpacked into a slot of the unpack area first: pos is relative to that area until the upload's size is
          // final (below). The sizes are the file's claims: nothing is reserved for a claim the stream cannot keep.
          if (h.type == PAGE_DATA_V2 && !v2) needs_host(QH_PQ_R_PAGE_V2, G, C, pageno);   // (its levels lie outside the compressed part)
          if (h.uncompressed < 0 || h.uncompressed > 0x7FFFFFFF) needs_host(QH_PQ_R_CORRUPT, G, C, pageno);
          qh_pq_unpack u;
          memset(&u, 0, sizeof u);
          const uint8_t* body = chunk + payload + lev;
          const uint64_t body_bytes = (uint64_t)h.compressed - lev, declared = (uint64_t)h.uncompressed - lev;
          u.page = (uint32_t)plan.pages.size();
          uint32_t frames = 0;
          int frame_bad = 0;
          if (lz && ch.codec == CODEC_LZ4 && qh_lz4_hadoop_scan(body, body_bytes, declared, &frames, &frame_bad)) {
            // the legacy id in Hadoop's framing: an entry per frame, the frames' outputs one behind the other in the page's slot,
            // so that the kernel knows no framing. A bare block whose first bytes happen to tile gets here too: the kernel
            // refuses what is then no block, and the page needs the host.
            if (frame_bad) needs_host(QH_PQ_R_LZ4_BASE + frame_bad, G, C, pageno);
            lz4_u64 at = 0, out = 0;
            lz4_u32 usize = 0, csize = 0;
            while (qh_lz4_hadoop_next(body, body_bytes, &at, &usize, &csize)) {
              u.src = cbuf + payload + lev + (at - csize); u.src_size = csize;
              u.dst = plan.unpack_bytes + out; u.dst_size = usize;
              plan.unlz4.push_back(u);
              out += usize;
            }
          } else {
            const int bad = lz     ? qh_lz4_check_sizes(body_bytes, declared)
                            : gz   ? qh_gzip_check_member(body, body_bytes, declared, &u.start)
                            : zstd ? qh_zstd_check_frame(body, body_bytes, declared, &u.start)
                                   : qh_snap_check_sizes(body, body_bytes, declared, &u.start);
            if (bad) needs_host((lz ? QH_PQ_R_LZ4_BASE : gz ? QH_PQ_R_GZIP_BASE : zstd ? QH_PQ_R_ZSTD_BASE : QH_PQ_R_SNAPPY_BASE) + bad, G, C, pageno);
            u.src = cbuf + payload + lev; u.src_size = (uint32_t)body_bytes;
            u.dst = plan.unpack_bytes; u.dst_size = (uint32_t)declared;
            (lz ? plan.unlz4 : gz ? plan.ungzip : zstd ? plan.unzstd : plan.unpack).push_back(u);
          }
          pg.pos = plan.unpack_bytes;
          size = (uint32_t)declared;
          plan.unpack_bytes += (declared + 15) & ~(uint64_t)15;
        }
        pg.size = size;
        if (h.type == PAGE_DICTIONARY) {
          if (have_dict || seen_data) needs_host(QH_PQ_R_PAGE_ORDER, G, C, pageno);
          if (!h.has_dict || h.num_values < 0 || h.num_values > 0x7FFFFFFF) needs_host(QH_PQ_R_CORRUPT, G, C, pageno);
          if ((h.encoding != ENC_PLAIN && h.encoding != ENC_PLAIN_DICTIONARY) || cp.boolean) needs_host(QH_PQ_R_ENCODING, G, C, pageno);
          // (fixed widths: every entry lies inside the page; BYTE_ARRAY: every entry has at least its 4 length bytes, which
          // bounds the entry array, and the string walk checks each length)
          if ((uint64_t)h.num_values * (cp.utf8 ? 4u : pw) > size) needs_host(QH_PQ_R_CORRUPT, G, C, pageno);
          have_dict = true;
          dict_pos = pg.pos; dict_size = size; dict_n = (uint32_t)h.num_values;
          dict_ent = plan.num_rows + cp.dict_entries;
          cp.dict_entries += dict_n;
          pg.enc = QH_PQ_ENC_DICTPAGE; pg.num_values = dict_n; pg.ent = dict_ent;
        } else if (h.type == PAGE_DATA || v2) {
          if (!v2 && (!h.has_data || h.num_values < 0)) needs_host(QH_PQ_R_CORRUPT, G, C, pageno);
          if ((uint64_t)h.num_values > (uint64_t)g.num_rows - got) needs_host(QH_PQ_R_NUM_VALUES, G, C, pageno);
          if (h.encoding == ENC_PLAIN) pg.enc = QH_PQ_ENC_PLAIN;
          else if ((h.encoding == ENC_RLE_DICTIONARY || h.encoding == ENC_PLAIN_DICTIONARY) && !cp.boolean) {
            if (!have_dict) needs_host(QH_PQ_R_CORRUPT, G, C, pageno);
            pg.enc = QH_PQ_ENC_DICT;
          } else if (set2 && h.encoding == ENC_RLE && cp.boolean) pg.enc = QH_PQ_ENC_RLE_BOOL;
          else if (set2 && h.encoding == ENC_BYTE_STREAM_SPLIT && pw) pg.enc = QH_PQ_ENC_BSS;
          else if (set2 && h.encoding == ENC_DELTA_BINARY_PACKED && (ptype == PT_INT32 || ptype == PT_INT64)) pg.enc = QH_PQ_ENC_DELTA;
          else if (set2 && h.encoding == ENC_DELTA_LENGTH_BYTE_ARRAY && cp.utf8) pg.enc = QH_PQ_ENC_DELTA_LEN;
          else if (dba >= 1 && h.encoding == ENC_DELTA_BYTE_ARRAY && cp.utf8) pg.enc = QH_PQ_ENC_DBA;
          else if (dba >= 1 && h.encoding == ENC_DELTA_BYTE_ARRAY && cp.phys == QH_PQ_P_FLBA) pg.enc = QH_PQ_ENC_DELTA;   // (dense in its slot behind k_pq_dba_fill)
          else needs_host(QH_PQ_R_ENCODING, G, C, pageno);
          if (pg.enc >= QH_PQ_ENC_RLE_BOOL) plan.has_ext = true;
          if (h.encoding == ENC_DELTA_BYTE_ARRAY) {
            qh_pq_dstream d;
            memset(&d, 0, sizeof d);
            qh_pq_fill fj;
            memset(&fj, 0, sizeof fj);
            d.page = fj.page = (uint32_t)plan.pages.size();
            d.width = cp.flba | QH_PQ_DS_DBA;
            fj.n = (uint32_t)h.num_values; fj.col = (uint32_t)k;
            if (cp.utf8) {
              cp.dba = true;
              fj.first = first_row + got;
              plan.fill_rows.push_back(fj);
            } else {
              // (sized by the page's claim, which the row group's rows bound, as they bound the output columns)
              fj.width = cp.flba;
              fj.out = plan.decoded_bytes;
              plan.decoded_bytes += ((uint64_t)h.num_values * cp.flba + 15) & ~(uint64_t)15;
              fj.first = d.dst = plan.decoded_bytes;
              plan.decoded_bytes += (uint64_t)h.num_values * sizeof(qh_pq_ent);
              plan.fill_values.push_back(fj);
            }
            plan.delta.push_back(d);
          } else if (pg.enc == QH_PQ_ENC_DELTA || pg.enc == QH_PQ_ENC_DELTA_LEN) {
            qh_pq_dstream d;
            memset(&d, 0, sizeof d);
            d.page = (uint32_t)plan.pages.size();
            d.width = pg.enc == QH_PQ_ENC_DELTA ? pw : (4u | QH_PQ_DS_LENGTHS);
            if (pg.enc == QH_PQ_ENC_DELTA) {
              // (the slot is sized by the page's claim, which the row group's rows bound, as they bound the output columns)
              d.dst = plan.decoded_bytes;
              plan.decoded_bytes += ((uint64_t)h.num_values * pw + 15) & ~(uint64_t)15;
            }
            plan.delta.push_back(d);
          }
          if (!v2 && cp.optional && h.def_encoding != ENC_RLE) needs_host(h.def_encoding == ENC_BIT_PACKED ? QH_PQ_R_LEVEL_ENCODING : QH_PQ_R_CORRUPT, G, C, pageno);
          seen_data = true;
          pg.num_values = (uint32_t)h.num_values; pg.first_row = first_row + got;
          pg.dict_pos = dict_pos; pg.dict_size = dict_size; pg.dict_n = dict_n;
          pg.ent = pg.enc == QH_PQ_ENC_DICT ? dict_ent : pg.first_row;
          got += (uint64_t)h.num_values;
        } else if (h.type == PAGE_DATA_V2) needs_host(QH_PQ_R_PAGE_V2, G, C, pageno);
        else if (h.type == PAGE_INDEX) needs_host(QH_PQ_R_INDEX_PAGE, G, C, pageno);
        else needs_host(QH_PQ_R_PAGE_ORDER, G, C, pageno);
        plan.pages.push_back(pg);
        in_unpack.push_back(packed ? (uint8_t)((unpacked ? 1 : 0) | ((h.type == PAGE_DATA || v2) && have_dict ? 2 : 0)) : (uint8_t)0);
        plan.where.push_back(PageWhere{G, C, pageno});
        if (plan.pages.size() >= (1u << 24)) needs_host(QH_PQ_R_CORRUPT, G, C, pageno);   // (the device's error word keeps 8 bits for the reason)
        pos = payload + (uint64_t)h.compressed;
      }
    }
    first_row += (uint64_t)g.num_rows;
  }
  // ---- the unpack area begins behind the last uploaded chunk: now its slots have their place in the buffer
  if (!plan.unpack.empty() || !plan.unzstd.empty() || !plan.ungzip.empty() || !plan.unlz4.empty()) {
    plan.unpack_base = (plan.upload_bytes + 15) & ~(uint64_t)15;
    for (qh_pq_unpack& u : plan.unpack) u.dst += plan.unpack_base;
    for (qh_pq_unpack& u : plan.unzstd) u.dst += plan.unpack_base;
    for (qh_pq_unpack& u : plan.ungzip) u.dst += plan.unpack_base;
    for (qh_pq_unpack& u : plan.unlz4) u.dst += plan.unpack_base;
    for (size_t p = 0; p < plan.pages.size(); ++p) {
      if (in_unpack[p] & 1) plan.pages[p].pos += plan.unpack_base;
      if (in_unpack[p] & 2) plan.pages[p].dict_pos += plan.unpack_base;
    }
  }
  // ---- ... and the decoded area behind that: a DELTA_BINARY_PACKED page's dict_pos is its slot
  if (plan.decoded_bytes) {
    plan.decoded_base = (plan.packed_bytes() + 15) & ~(uint64_t)15;
    for (qh_pq_dstream& d : plan.delta) {
      if (d.width & QH_PQ_DS_DBA) { if (d.width & 0xFFu) d.dst += plan.decoded_base; }   // (its entries; a Utf8 page has the column's)
      else if (!(d.width & QH_PQ_DS_LENGTHS)) { d.dst += plan.decoded_base; plan.pages[d.page].dict_pos = d.dst; }
    }
    for (qh_pq_fill& fj : plan.fill_values) { fj.first += plan.decoded_base; fj.out += plan.decoded_base; plan.pages[fj.page].dict_pos = fj.out; }
  }
  return plan;
}

}  // namespace qhip_pq
