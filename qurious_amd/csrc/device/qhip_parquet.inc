// qhip_parquet.inc — per-run and per-value code of the device Parquet decoder (parquet.cpp qhip_table_from_parquet,
// kernels_parquet.hip; DESIGN §3.9): the needs-host reasons, the page and column descriptors both sides share, the run headers
// of the RLE / bit-packed hybrid, bit extraction, the validity word a level run contributes, the physical value readers
// (little-endian INT32 / INT64, big-endian FIXED_LEN_BYTE_ARRAY decimals) and the checks of a BYTE_ARRAY length chain.
//
// One text for two compilers: included by kernels_parquet.hip for hipcc and, as plain host C++, by parquet.cpp and
// tests/cpp/parquet_tests.cpp, so the functions the kernels call are the functions the CPU tests check under the sanitizers.
// Self-contained: builtin integer types only, no #include. Every count, length and index in a page is untrusted: each function
// says which bytes it reads and the caller has checked them against the page before (no load assumes more than 1-byte alignment).
#ifndef QHIP_PARQUET_INC
#define QHIP_PARQUET_INC
#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define QH_PQ_HD __host__ __device__
#else
#define QH_PQ_HD
#endif

typedef unsigned char pq_u8;
typedef unsigned int pq_u32;
typedef unsigned long long pq_u64;
typedef long long pq_i64;

#define QH_PQ_MAX_COLS 64

// ---- why a file needs the host path (the smallest page << 8 | reason wins on the device, as for CSV)
#define QH_PQ_OK 0
#define QH_PQ_R_MAGIC 1            // no PAR1 at both ends, or too short for a footer
#define QH_PQ_R_ENCRYPTED 2        // PARE: an encrypted footer
#define QH_PQ_R_CORRUPT 3          // an offset, length or count that points outside the file, its chunk or its page
#define QH_PQ_R_NESTED 4           // a group, list or map field somewhere in the schema
#define QH_PQ_R_SCHEMA 5           // the file's fields are not the passed schema's
#define QH_PQ_R_TYPE 6             // a (physical type, annotation, Arrow type) triple outside the coverage list
#define QH_PQ_R_CODEC 7            // a projected chunk is compressed
#define QH_PQ_R_FILE_PATH 8        // a projected chunk lives in another file
#define QH_PQ_R_PAGE_V2 9
#define QH_PQ_R_INDEX_PAGE 10
#define QH_PQ_R_PAGE_ORDER 11      // a second dictionary page, one behind a data page, an unknown page type
#define QH_PQ_R_ENCODING 12        // a value encoding other than PLAIN / PLAIN_DICTIONARY / RLE_DICTIONARY
#define QH_PQ_R_LEVEL_ENCODING 13  // BIT_PACKED definition levels
#define QH_PQ_R_REPEATED 14        // a repeated field: repetition level above 0
#define QH_PQ_R_NO_ROWS 15
#define QH_PQ_R_TOO_MANY_COLUMNS 16
#define QH_PQ_R_TOO_MANY_ROWS 17
#define QH_PQ_R_NUM_VALUES 18      // a chunk's data pages do not add up to the row group's rows
#define QH_PQ_R_LEVELS_LENGTH 19   // the levels' length prefix points past the page
#define QH_PQ_R_RUN 20             // a run header or a run's bytes past the end of its stream, or a run of no values
#define QH_PQ_R_RUN_COUNT 21       // a level run that counts past num_values
#define QH_PQ_R_LEVEL_VALUE 22     // a definition level above 1
#define QH_PQ_R_BIT_WIDTH 23       // dictionary indices wider than 32 bits
#define QH_PQ_R_VALUES_SHORT 24    // the values region holds fewer values than the page has non-NULL rows
#define QH_PQ_R_DICT_INDEX 25      // a dictionary index >= the dictionary's entry count
#define QH_PQ_R_BYTE_ARRAY 26      // a BYTE_ARRAY length that points past its page
#define QH_PQ_R_RANGE 27           // a stored INT32 outside an Int8 / Int16 / UInt8 / UInt16 column's range
#define QH_PQ_R_UTF8_LONG 28       // a Utf8 column of more than 2^31 - 1 bytes
// (format level 2: a Snappy page, device/qhip_snappy.inc. QH_PQ_R_SNAPPY_BASE + QH_SNAP_E_*)
#define QH_PQ_R_SNAPPY_BASE 28
#define QH_PQ_R_SNAPPY_PREAMBLE 29 // the stream's preamble does not end, or is not the header's uncompressed_page_size
#define QH_PQ_R_SNAPPY_SIZE 30     // uncompressed_page_size above 64/3 times the compressed payload
#define QH_PQ_R_SNAPPY_INPUT 31    // an element past the end of its stream, or stream and page do not end together
#define QH_PQ_R_SNAPPY_OUTPUT 32   // an element past uncompressed_page_size
#define QH_PQ_R_SNAPPY_OFFSET 33   // a copy offset of 0 or beyond the bytes produced
// (encoding set 2, qhip_ctx_set_parquet_encodings: data pages V2, RLE Booleans, BYTE_STREAM_SPLIT, DELTA_*; device/qhip_delta.inc)
#define QH_PQ_R_V2_UNCOMPRESSED 34 // a data page V2 with is_compressed = false whose two sizes differ
#define QH_PQ_R_V2_LEVELS 35       // a data page V2 whose level lengths point past the page, or definition levels in a required column
#define QH_PQ_R_V2_REPETITION 36   // a data page V2 with repetition levels
#define QH_PQ_R_V2_ROWS 37         // a data page V2 whose num_rows is not its num_values
#define QH_PQ_R_V2_NULLS 38        // a data page V2 whose num_nulls is not what its levels say
#define QH_PQ_R_RLE_LENGTH 39      // RLE Boolean values whose length prefix points past the page, or a value above 1
#define QH_PQ_R_BSS_SIZE 40        // a BYTE_STREAM_SPLIT region that is not (non-NULL rows) x (value width) bytes
#define QH_PQ_R_DELTA_VARINT 41    // a DELTA_BINARY_PACKED varint of more than 64 bits
#define QH_PQ_R_DELTA_GEOMETRY 42  // block size 0 or no multiple of 128, miniblocks 0 or no divisor, values per miniblock no multiple of 32
#define QH_PQ_R_DELTA_LARGE 43     // a block of more than 65 536 values
#define QH_PQ_R_DELTA_COUNT 44     // the stream's total count is not the page's non-NULL rows
#define QH_PQ_R_DELTA_SHORT 45     // the stream ends inside its header, a block header, the width bytes or a miniblock
#define QH_PQ_R_DELTA_WIDTH 46     // a miniblock that holds a value has a bit width above the type's
#define QH_PQ_R_DELTA_LENGTH 47    // DELTA_LENGTH_BYTE_ARRAY: a negative length, or lengths that add up past the page
// (codec set 2, qhip_ctx_set_parquet_codecs: a ZSTD page, device/qhip_zstd.inc. QH_PQ_R_ZSTD_BASE + QH_ZSTD_E_*)
#define QH_PQ_R_ZSTD_BASE 47
#define QH_PQ_R_ZSTD_FRAME 48      // the frame header: magic, a dictionary id, the reserved bit, a skippable or second frame, stray bytes behind the last block
#define QH_PQ_R_ZSTD_SIZE 49       // Frame_Content_Size or the blocks' bound against uncompressed_page_size
#define QH_PQ_R_ZSTD_BLOCK 50      // a block header: cut off, the reserved type, above 128 KB, past the payload
#define QH_PQ_R_ZSTD_LITERALS 51   // a literals section that is cut off, above 128 KB, or whose stream sizes do not fit
#define QH_PQ_R_ZSTD_HUFFMAN 52    // a Huffman tree description outside the format's rules, or a treeless section without a tree
#define QH_PQ_R_ZSTD_FSE 53        // an FSE table description outside the format's rules
#define QH_PQ_R_ZSTD_SEQUENCES 54  // a sequences section that is cut off, has reserved bits, repeats a table that is not there, or wants more literals than there are
#define QH_PQ_R_ZSTD_BITS 55       // a backward bit stream that underflows or does not end exactly at its start
#define QH_PQ_R_ZSTD_OUTPUT 56     // output past uncompressed_page_size, or a frame that ends with output missing
#define QH_PQ_R_ZSTD_OFFSET 57     // a match offset of 0 or beyond the bytes produced
// (the gzip switch, qhip_ctx_set_parquet_gzip: a GZIP page, device/qhip_inflate.inc. QH_PQ_R_GZIP_BASE + QH_INFL_E_*)
#define QH_PQ_R_GZIP_BASE 57
#define QH_PQ_R_GZIP_MEMBER 58     // the member header: magic (a zlib wrapper among the rest), CM, a reserved FLG bit, an optional field cut off, no room for a body and the trailer
#define QH_PQ_R_GZIP_SIZE 59       // ISIZE against uncompressed_page_size mod 2^32, or a size above 1032 x the body's bytes
#define QH_PQ_R_GZIP_BLOCK 60      // a block header: BTYPE 3, a stored block whose LEN and NLEN do not match
#define QH_PQ_R_GZIP_LENGTHS 61    // a dynamic block's code lengths: HLIT, HDIST, the code-length code, a repeat with nothing before it or past the count
#define QH_PQ_R_GZIP_CODE 62       // a literal/length or distance code that is over-subscribed or incomplete, or has no end-of-block code
#define QH_PQ_R_GZIP_SYMBOL 63     // bits that are no code, literal/length symbol 286 / 287, distance symbol 30 / 31
#define QH_PQ_R_GZIP_DISTANCE 64   // a distance of 0 or beyond the bytes produced
#define QH_PQ_R_GZIP_OUTPUT 65     // output past uncompressed_page_size, or a final block that ends with output missing
#define QH_PQ_R_GZIP_INPUT 66      // the input ends inside a header, a code length, a symbol or a stored block
#define QH_PQ_R_GZIP_TRAILER 67    // bytes between the final block and the trailer: a second member among the rest
// (the lz4 switch, qhip_ctx_set_parquet_lz4: an LZ4_RAW or legacy LZ4 page, device/qhip_lz4.inc. QH_PQ_R_LZ4_BASE + QH_LZ4_E_*)
#define QH_PQ_R_LZ4_BASE 67
#define QH_PQ_R_LZ4_SIZE 68        // a size above 255 x the block's bytes
#define QH_PQ_R_LZ4_FRAME 69       // Hadoop framing: the frames tile the page, but one has no bytes for the output it declares
#define QH_PQ_R_LZ4_CUT 70         // the input ends inside a length's extension or an offset
#define QH_PQ_R_LZ4_LITERAL 71     // a literal run past the input
#define QH_PQ_R_LZ4_OUTPUT 72      // a literal run or a match past uncompressed_page_size
#define QH_PQ_R_LZ4_OFFSET 73      // a match offset of 0 or beyond the bytes produced
#define QH_PQ_R_LZ4_END 74         // input left behind a full output; input that ends with output missing, or behind a match
// (the DELTA_BYTE_ARRAY switch, qhip_ctx_set_parquet_delta_byte_array: device/qhip_dba.inc)
#define QH_PQ_R_DBA_PREFIX 75      // a negative prefix length, a first prefix of the page that is not 0, a prefix longer than the value before it
#define QH_PQ_R_DBA_SUFFIX 76      // a negative suffix length, suffix lengths that add up past the page, a value longer than 2^31 - 1
#define QH_PQ_R_DBA_WIDTH 77       // a FIXED_LEN_BYTE_ARRAY value whose length is not the column's width
#define QH_PQ_R_COUNT 78

QH_PQ_HD inline const char* qh_pq_reason_text(unsigned r) {
  switch (r) {
    case QH_PQ_R_MAGIC: return "no PAR1 magic at both ends";
    case QH_PQ_R_ENCRYPTED: return "an encrypted footer";
    case QH_PQ_R_CORRUPT: return "corrupt: an offset, length or count points outside the file, its chunk or its page";
    case QH_PQ_R_NESTED: return "a group, list or map field in the schema";
    case QH_PQ_R_SCHEMA: return "the file's fields differ from the schema's";
    case QH_PQ_R_TYPE: return "a column type that is not decoded on the device";
    case QH_PQ_R_CODEC: return "a compressed column chunk";
    case QH_PQ_R_FILE_PATH: return "a column chunk stored in another file";
    case QH_PQ_R_PAGE_V2: return "a data page V2";
    case QH_PQ_R_INDEX_PAGE: return "an index page";
    case QH_PQ_R_PAGE_ORDER: return "a dictionary page that is not the chunk's first page, or an unknown page type";
    case QH_PQ_R_ENCODING: return "a value encoding other than PLAIN and RLE_DICTIONARY";
    case QH_PQ_R_LEVEL_ENCODING: return "BIT_PACKED definition levels";
    case QH_PQ_R_REPEATED: return "a repeated field";
    case QH_PQ_R_NO_ROWS: return "a file of 0 rows";
    case QH_PQ_R_TOO_MANY_COLUMNS: return "more than 64 projected columns";
    case QH_PQ_R_TOO_MANY_ROWS: return "2^32 - 1 rows or more";
    case QH_PQ_R_NUM_VALUES: return "corrupt: the data pages' num_values do not add up to the row group's rows";
    case QH_PQ_R_LEVELS_LENGTH: return "corrupt: the levels' length points past the page";
    case QH_PQ_R_RUN: return "corrupt: a run past the end of its stream";
    case QH_PQ_R_RUN_COUNT: return "corrupt: a level run counts past num_values";
    case QH_PQ_R_LEVEL_VALUE: return "a definition level above 1";
    case QH_PQ_R_BIT_WIDTH: return "corrupt: a dictionary index width above 32 bits";
    case QH_PQ_R_VALUES_SHORT: return "corrupt: fewer values than non-NULL rows in the page";
    case QH_PQ_R_DICT_INDEX: return "corrupt: a dictionary index past the dictionary's entries";
    case QH_PQ_R_BYTE_ARRAY: return "corrupt: a BYTE_ARRAY length points past its page";
    case QH_PQ_R_RANGE: return "a stored value outside the column's integer range";
    case QH_PQ_R_UTF8_LONG: return "a Utf8 column larger than 2 GiB";
    case QH_PQ_R_SNAPPY_PREAMBLE: return "corrupt: a Snappy page whose preamble does not end or differs from uncompressed_page_size";
    case QH_PQ_R_SNAPPY_SIZE: return "corrupt: a Snappy page that claims more than 64/3 times its compressed size";
    case QH_PQ_R_SNAPPY_INPUT: return "corrupt: a Snappy element past the end of its page, or a page whose stream and size do not end together";
    case QH_PQ_R_SNAPPY_OUTPUT: return "corrupt: a Snappy element past uncompressed_page_size";
    case QH_PQ_R_SNAPPY_OFFSET: return "corrupt: a Snappy copy offset of 0 or beyond the bytes produced";
    case QH_PQ_R_V2_UNCOMPRESSED: return "corrupt: a data page V2 marked uncompressed whose compressed and uncompressed sizes differ";
    case QH_PQ_R_V2_LEVELS: return "corrupt: a data page V2 whose level lengths point past the page, or levels in a required column";
    case QH_PQ_R_V2_REPETITION: return "a data page V2 with repetition levels";
    case QH_PQ_R_V2_ROWS: return "a data page V2 whose num_rows differs from num_values";
    case QH_PQ_R_V2_NULLS: return "corrupt: a data page V2 whose num_nulls differs from its levels";
    case QH_PQ_R_RLE_LENGTH: return "corrupt: RLE Boolean values whose length points past the page, or a value above 1";
    case QH_PQ_R_BSS_SIZE: return "corrupt: a BYTE_STREAM_SPLIT region that is not non-NULL rows times the value width";
    case QH_PQ_R_DELTA_VARINT: return "corrupt: a DELTA_BINARY_PACKED varint of more than 64 bits";
    case QH_PQ_R_DELTA_GEOMETRY: return "corrupt: a DELTA_BINARY_PACKED block size or miniblock count outside the format's rules";
    case QH_PQ_R_DELTA_LARGE: return "a DELTA_BINARY_PACKED block of more than 65536 values";
    case QH_PQ_R_DELTA_COUNT: return "corrupt: a DELTA_BINARY_PACKED total count that differs from the page's non-NULL rows";
    case QH_PQ_R_DELTA_SHORT: return "corrupt: a DELTA_BINARY_PACKED stream that ends inside a header or a miniblock";
    case QH_PQ_R_DELTA_WIDTH: return "corrupt: a DELTA_BINARY_PACKED bit width above the type's bits";
    case QH_PQ_R_DELTA_LENGTH: return "corrupt: a DELTA_LENGTH_BYTE_ARRAY length that is negative or points past its page";
    case QH_PQ_R_ZSTD_FRAME: return "a Zstd page whose frame header is not one plain frame: magic, dictionary id, reserved bit, or bytes behind the last block";
    case QH_PQ_R_ZSTD_SIZE: return "corrupt: a Zstd page whose frame size or block sizes do not fit uncompressed_page_size";
    case QH_PQ_R_ZSTD_BLOCK: return "corrupt: a Zstd block header that is cut off, of the reserved type, above 128 KB or past its page";
    case QH_PQ_R_ZSTD_LITERALS: return "corrupt: a Zstd literals section that is cut off, above 128 KB, or whose streams do not fit";
    case QH_PQ_R_ZSTD_HUFFMAN: return "corrupt: a Zstd Huffman tree description outside the format's rules";
    case QH_PQ_R_ZSTD_FSE: return "corrupt: a Zstd FSE table description outside the format's rules";
    case QH_PQ_R_ZSTD_SEQUENCES: return "corrupt: a Zstd sequences section that is cut off or inconsistent with its literals and tables";
    case QH_PQ_R_ZSTD_BITS: return "corrupt: a Zstd bit stream that underflows or does not end exactly at its start";
    case QH_PQ_R_ZSTD_OUTPUT: return "corrupt: a Zstd page whose output passes or does not fill uncompressed_page_size";
    case QH_PQ_R_ZSTD_OFFSET: return "corrupt: a Zstd match offset of 0 or beyond the bytes produced";
    case QH_PQ_R_GZIP_MEMBER: return "a Gzip page whose member header is not one plain gzip member: magic, method, reserved flags, or a header cut off";
    case QH_PQ_R_GZIP_SIZE: return "corrupt: a Gzip page whose ISIZE or body size does not fit uncompressed_page_size";
    case QH_PQ_R_GZIP_BLOCK: return "corrupt: a Gzip block header of the reserved type, or a stored block whose lengths do not match";
    case QH_PQ_R_GZIP_LENGTHS: return "corrupt: Gzip code lengths outside the format's rules";
    case QH_PQ_R_GZIP_CODE: return "corrupt: a Gzip Huffman code that is over-subscribed, incomplete or without an end-of-block code";
    case QH_PQ_R_GZIP_SYMBOL: return "corrupt: a Gzip symbol that is no code or outside the alphabet";
    case QH_PQ_R_GZIP_DISTANCE: return "corrupt: a Gzip match distance of 0 or beyond the bytes produced";
    case QH_PQ_R_GZIP_OUTPUT: return "corrupt: a Gzip page whose output passes or does not fill uncompressed_page_size";
    case QH_PQ_R_GZIP_INPUT: return "corrupt: a Gzip page whose input ends inside a block";
    case QH_PQ_R_GZIP_TRAILER: return "a Gzip page with bytes between its final block and its trailer: a second member, or stray bytes";
    case QH_PQ_R_LZ4_SIZE: return "corrupt: an LZ4 page whose size exceeds 255 times its compressed bytes";
    case QH_PQ_R_LZ4_FRAME: return "corrupt: an LZ4 page whose Hadoop frames tile it, one of them without bytes for the output it declares";
    case QH_PQ_R_LZ4_CUT: return "corrupt: an LZ4 page whose input ends inside a length or an offset";
    case QH_PQ_R_LZ4_LITERAL: return "corrupt: an LZ4 literal run past the input";
    case QH_PQ_R_LZ4_OUTPUT: return "corrupt: an LZ4 literal run or match past uncompressed_page_size";
    case QH_PQ_R_LZ4_OFFSET: return "corrupt: an LZ4 match offset of 0 or beyond the bytes produced";
    case QH_PQ_R_LZ4_END: return "corrupt: an LZ4 page whose input and output do not end together behind a literal run";
    case QH_PQ_R_DBA_PREFIX: return "a DELTA_BYTE_ARRAY prefix length that is negative, not 0 at the head of its page, or longer than the value before it";
    case QH_PQ_R_DBA_SUFFIX: return "corrupt: a DELTA_BYTE_ARRAY suffix length that is negative or points past its page, or a value above 2 GiB";
    case QH_PQ_R_DBA_WIDTH: return "corrupt: a DELTA_BYTE_ARRAY value of a fixed-length column whose length is not the column's width";
    default: return "outside the device's Parquet coverage";
  }
}

// ---- descriptors (host: parquet.cpp fills them; device: the kernels read them from device memory)
#define QH_PQ_ENC_PLAIN 0u
#define QH_PQ_ENC_DICT 1u       // RLE_DICTIONARY / PLAIN_DICTIONARY indices over the chunk's dictionary page
#define QH_PQ_ENC_DICTPAGE 2u   // the dictionary page itself: only the string walk looks at it (Utf8)
// (encoding set 2: k_pq_values leaves these pages to k_pq_values_ext)
#define QH_PQ_ENC_RLE_BOOL 3u   // BOOLEAN values as the hybrid at width 1 behind a 4-byte length
#define QH_PQ_ENC_BSS 4u        // BYTE_STREAM_SPLIT: byte j of value idx at j * (non-NULL rows) + idx
#define QH_PQ_ENC_DELTA 5u      // DELTA_BINARY_PACKED: k_pq_delta leaves the values dense (PLAIN) in the page's slot at dict_pos
#define QH_PQ_ENC_DELTA_LEN 6u  // DELTA_LENGTH_BYTE_ARRAY: k_pq_delta writes the page's (length, position) entries
// (the DELTA_BYTE_ARRAY switch. A FIXED_LEN_BYTE_ARRAY page of that encoding is QH_PQ_ENC_DELTA: k_pq_dba_fill leaves its values dense)
#define QH_PQ_ENC_DBA 7u        // DELTA_BYTE_ARRAY, Utf8: k_pq_delta writes the page's (length, suffix position, prefix length) entries

#define QH_PQ_F_V2 1u           // a data page V2: its levels lie at lev_pos without a length prefix, its values begin at pos

// physical layout of a stored value
#define QH_PQ_P_BOOL 0u
#define QH_PQ_P_32 1u           // 4 bytes little-endian (INT32 sign-extended, FLOAT as its bits)
#define QH_PQ_P_64 2u           // 8 bytes little-endian
#define QH_PQ_P_FLBA 3u         // `flba` bytes big-endian two's complement (decimals)
#define QH_PQ_P_BYTES 4u        // BYTE_ARRAY: 4-byte length, then the bytes

// one page of a projected chunk, in file order within its chunk. Positions are byte offsets into the device buffer: the
// uploaded chunks and, behind them, the unpack area. A page of a Snappy chunk is described as it lies unpacked in its slot there.
typedef struct qh_pq_page {
  pq_u64 pos;         // the page's payload (behind its header)
  pq_u64 first_row;   // data page: its first row in the output column
  pq_u64 dict_pos;    // data page: the chunk's dictionary page payload (QH_PQ_ENC_DELTA: its slot in the decoded area); dictionary page: unused
  pq_u64 ent;         // Utf8: where this page's (length, position) entries begin in the column's entry array
  pq_u32 size;        // payload bytes
  pq_u32 num_values;  // data page: rows; dictionary page: entries
  pq_u32 col;         // index into the column descriptors
  pq_u32 enc;         // QH_PQ_ENC_*
  pq_u32 dict_size;   // data page: the dictionary payload's bytes
  pq_u32 dict_n;      // ... and its entry count (fixed widths: dict_n * width <= dict_size was checked on the host)
  pq_u64 lev_pos;     // data page V2: its definition levels, lev_size bytes in the uploaded chunks (never compressed)
  pq_u32 lev_size;
  pq_u32 flags;       // QH_PQ_F_*
  pq_u32 num_nulls;   // data page V2: what its header claims; the level pass counts
  pq_u32 pad;
} qh_pq_page;

// one DELTA_BINARY_PACKED stream for k_pq_delta (encoding set 2). Of a page: src, src_size and count come from the page and the
// level pass's state on the device. Of a raw stream (qhip_parquet_delta_decode): they stand here.
typedef struct qh_pq_dstream {
  pq_u64 src;         // raw: the stream in the buffer
  pq_u64 dst;         // the dense values' slot, 16-byte aligned, count * width bytes (unused for lengths)
  pq_u32 src_size;
  pq_u32 count;       // raw: the expected number of values
  pq_u32 page;        // index into the page table (the offender word), or the stream's number
  pq_u32 width;       // 4 or 8: the physical type's bytes; | QH_PQ_DS_LENGTHS for DELTA_LENGTH_BYTE_ARRAY; QH_PQ_DS_DBA, below
} qh_pq_dstream;
#define QH_PQ_DS_LENGTHS 0x100u
// DELTA_BYTE_ARRAY: the stream of prefix lengths, behind it the stream of suffix lengths, behind that the suffix bytes. The low
// byte of width is the FIXED_LEN_BYTE_ARRAY width every value must have, 0 for BYTE_ARRAY. The entries go to the column's entry
// array (a Utf8 page) or, 16 bytes each, to `dst` (a FIXED_LEN_BYTE_ARRAY page, a raw stream).
#define QH_PQ_DS_DBA 0x200u

// one DELTA_BYTE_ARRAY page for k_pq_dba_fill. Row space (a Utf8 column, after the host wait): the rows [first, first + n) of
// the column. Value space (a FIXED_LEN_BYTE_ARRAY page, before the wait): the page's entries lie at buffer[first ..), its dense
// values go to buffer[out ..), `width` bytes each; their count is the level pass's non-NULL count of page `page`.
typedef struct qh_pq_fill {
  pq_u64 first;
  pq_u64 out;
  pq_u32 n;
  pq_u32 page;
  pq_u32 width;
  pq_u32 col;         // row space: the column (host side only)
} qh_pq_fill;

// one compressed page (format level 2): k_pq_unsnap turns buffer[src .. src + src_size) into buffer[dst .. dst + dst_size).
// Codec set 2 keeps the ZSTD pages in a second table of the same entries for k_pq_unzstd: `start` is then where the frame's
// first block header lies, and dst_size what the frame header says where it says it. The gzip switch keeps the GZIP pages in
// a third table for k_pq_ungzip: `start` is where the member's first DEFLATE block lies. The lz4 switch keeps the LZ4 pages in
// a fourth for k_pq_unlz4, one entry per bare block: a page in Hadoop's framing has an entry per frame, each with its own source
// range and its own slice of the page's slot; `start` is 0.
typedef struct qh_pq_unpack {
  pq_u64 src;         // the compressed payload, in the uploaded chunks
  pq_u64 dst;         // the page's slot in the unpack area, 16-byte aligned
  pq_u32 src_size;
  pq_u32 dst_size;    // uncompressed_page_size: what the stream's preamble says (checked on the host)
  pq_u32 page;        // index into the page table (the offender word)
  pq_u32 start;       // bytes of the preamble: where the elements begin in the payload
} qh_pq_unpack;

// one BYTE_ARRAY value: its bytes in the buffer. Of a DELTA_BYTE_ARRAY page: len is prefix + suffix, pos where the suffix bytes
// lie, pad the prefix length; everywhere else pad is 0.
typedef struct qh_pq_ent { pq_u64 pos; pq_u32 len; pq_u32 pad; } qh_pq_ent;

typedef struct qh_pq_col {
  void* values;       // width-byte values | u32 lengths (Utf8, scanned into offsets afterwards) | Boolean bits (zeroed)
  pq_u64* valid;      // validity words, zeroed; NULL for a required column
  pq_u64* strpos;     // Utf8: where row k's bytes lie in the buffer
  qh_pq_ent* ent;     // Utf8: entries of the PLAIN data pages (at first_row) and of the dictionaries (behind the rows)
  pq_u32 phys;        // QH_PQ_P_*
  pq_u32 flba;        // FIXED_LEN_BYTE_ARRAY length 1..16
  pq_u32 width;       // bytes of an output value: 1, 2, 4, 8, 16 (0: Boolean, Utf8)
  pq_u32 narrow;      // 0: none; 1: signed, 2: unsigned range check of an INT32 stored for a 1- / 2-byte column
  pq_u32* prefix;     // Utf8 with a DELTA_BYTE_ARRAY page: row k's prefix length, zeroed; NULL for every other column
} qh_pq_col;

// what the level pass leaves for the value passes, per page
typedef struct qh_pq_state { pq_u32 nonnull; pq_u32 values_off; } qh_pq_state;

// ---- little-endian reads at any alignment
QH_PQ_HD inline pq_u32 qh_pq_le32(const pq_u8* p) { return (pq_u32)p[0] | ((pq_u32)p[1] << 8) | ((pq_u32)p[2] << 16) | ((pq_u32)p[3] << 24); }
QH_PQ_HD inline pq_u64 qh_pq_le64(const pq_u8* p) { return (pq_u64)qh_pq_le32(p) | ((pq_u64)qh_pq_le32(p + 4) << 32); }

// ULEB128 of a u32 at s[pos ..), nothing read at or behind s[len]. Returns the bytes consumed, 0 when it does not end in time.
QH_PQ_HD inline int qh_pq_varint(const pq_u8* s, pq_u64 len, pq_u64 pos, pq_u32* out) {
  pq_u32 v = 0;
  for (int i = 0; i < 5; ++i) {
    if (pos + (pq_u64)i >= len) return 0;
    const pq_u32 b = s[pos + (pq_u64)i];
    if (i == 4 && b > 0x0Fu) return 0;
    v |= (b & 0x7Fu) << (7 * i);
    if (!(b & 0x80u)) { *out = v; return i + 1; }
  }
  return 0;
}

// ---- the RLE / bit-packed hybrid. A run covers the value indices [start, start + count) of its stream.
typedef struct qh_pq_run {
  pq_u64 start, count;
  pq_u64 data;      // bit-packed: where its bytes begin in the stream (count / 8 * width of them, all inside the stream)
  pq_u32 value;     // RLE: the repeated value
  pq_u32 packed;
} qh_pq_run;

QH_PQ_HD inline void qh_pq_run_init(qh_pq_run* r) { r->start = 0; r->count = 0; r->data = 0; r->value = 0; r->packed = 0; }

// The run behind `r` in the stream s[0 .. len) of bit width w (0..32): parses the header at *cpos, checks that the run's bytes
// lie inside the stream, moves *cpos behind them. QH_PQ_OK or QH_PQ_R_RUN; a run of no values is refused (no progress).
QH_PQ_HD inline int qh_pq_next_run(const pq_u8* s, pq_u64 len, pq_u64* cpos, pq_u32 w, qh_pq_run* r) {
  pq_u32 h = 0;
  const int used = qh_pq_varint(s, len, *cpos, &h);
  if (!used) return QH_PQ_R_RUN;
  const pq_u64 pos = *cpos + (pq_u64)used;
  r->start += r->count;
  if (h & 1u) {
    const pq_u64 groups = h >> 1;
    const pq_u64 bytes = groups * w;
    if (!groups || bytes > len - pos) return QH_PQ_R_RUN;
    r->packed = 1; r->count = groups * 8; r->data = pos; r->value = 0;
    *cpos = pos + bytes;
  } else {
    const pq_u64 vb = (w + 7u) >> 3;
    if (!(h >> 1) || vb > len - pos) return QH_PQ_R_RUN;
    pq_u32 v = 0;
    for (pq_u64 i = 0; i < vb; ++i) v |= (pq_u32)s[pos + i] << (8 * i);
    r->packed = 0; r->count = h >> 1; r->data = pos; r->value = v;
    *cpos = pos + vb;
  }
  return QH_PQ_OK;
}

// value k (k < count) of a bit-packed run whose bytes begin at d: w bits at bit k * w. Reads only bytes of the run.
QH_PQ_HD inline pq_u32 qh_pq_extract(const pq_u8* d, pq_u64 k, pq_u32 w) {
  if (!w) return 0;
  const pq_u64 bit = k * w, b = bit >> 3;
  const pq_u32 sh = (pq_u32)(bit & 7u), nb = (sh + w + 7u) >> 3;   // at most 5 bytes
  pq_u64 v = 0;
  for (pq_u32 i = 0; i < nb; ++i) v |= (pq_u64)d[b + i] << (8 * i);
  return (pq_u32)((v >> sh) & (w == 32 ? 0xFFFFFFFFull : ((1ull << w) - 1ull)));
}

QH_PQ_HD inline pq_u32 qh_pq_run_value(const pq_u8* s, const qh_pq_run* r, pq_u64 idx, pq_u32 w) {
  return r->packed ? qh_pq_extract(s + r->data, idx - r->start, w) : r->value;
}

// The bits a level run (width 1) sets in validity word `word` of the column: the run's first `take` values stand for the rows
// [g0, g0 + take). 0 where the run does not touch the word. A bit-packed run reads at most 9 of its own bytes.
QH_PQ_HD inline pq_u64 qh_pq_level_word(const pq_u8* s, const qh_pq_run* r, pq_u64 g0, pq_u64 take, pq_u64 word) {
  const pq_u64 w0 = word * 64;
  const pq_u64 lo = w0 > g0 ? w0 : g0, hi = w0 + 64 < g0 + take ? w0 + 64 : g0 + take;
  if (lo >= hi) return 0;
  const pq_u32 n = (pq_u32)(hi - lo);
  pq_u64 bits;
  if (!r->packed) {
    bits = r->value ? ~0ull : 0ull;
  } else {
    const pq_u64 k = lo - g0, b = k >> 3;
    const pq_u32 sh = (pq_u32)(k & 7u), nb = (sh + n + 7u) >> 3;   // at most 9 bytes, all below count / 8
    const pq_u8* d = s + r->data + b;
    bits = 0;
    for (pq_u32 i = 0; i < nb && i < 8; ++i) bits |= (pq_u64)d[i] << (8 * i);
    bits >>= sh;
    if (nb == 9) bits |= (pq_u64)d[8] << (64 - sh);   // (nb == 9 only with sh > 0)
  }
  if (n < 64) bits &= (1ull << n) - 1ull;
  return bits << (lo & 63u);
}

// ---- stored values. A value is read as a sign-extended 128-bit integer (lo, hi) and its low `width` bytes are stored.
QH_PQ_HD inline void qh_pq_read_value(const pq_u8* src, pq_u32 phys, pq_u32 flba, pq_u64* lo, pq_u64* hi) {
  if (phys == QH_PQ_P_32) {
    const pq_i64 v = (pq_i64)(int)qh_pq_le32(src);
    *lo = (pq_u64)v; *hi = v < 0 ? ~0ull : 0ull;
  } else if (phys == QH_PQ_P_64) {
    *lo = qh_pq_le64(src); *hi = (*lo >> 63) ? ~0ull : 0ull;
  } else {
    // FIXED_LEN_BYTE_ARRAY decimal: flba (1..16) bytes, big-endian two's complement
    pq_u64 l = (src[0] & 0x80u) ? ~0ull : 0ull, h = l;
    for (pq_u32 i = 0; i < flba; ++i) { h = (h << 8) | (l >> 56); l = (l << 8) | src[i]; }
    *lo = l; *hi = h;
  }
}

// an INT32 stored for an Int8 / Int16 / UInt8 / UInt16 column must lie in the column's range
QH_PQ_HD inline bool qh_pq_in_range(pq_u64 lo, pq_u32 width, pq_u32 narrow) {
  const pq_i64 v = (pq_i64)lo;
  if (narrow == 1) return width == 1 ? (v >= -128 && v <= 127) : (v >= -32768 && v <= 32767);
  if (narrow == 2) return width == 1 ? (v >= 0 && v <= 255) : (v >= 0 && v <= 65535);
  return true;
}

QH_PQ_HD inline void qh_pq_store(void* values, pq_u64 row, pq_u32 width, pq_u64 lo, pq_u64 hi) {
  switch (width) {
    case 1: ((pq_u8*)values)[row] = (pq_u8)lo; break;
    case 2: ((unsigned short*)values)[row] = (unsigned short)lo; break;
    case 4: ((pq_u32*)values)[row] = (pq_u32)lo; break;
    case 8: ((pq_u64*)values)[row] = lo; break;
    default: ((pq_u64*)values)[2 * row] = lo; ((pq_u64*)values)[2 * row + 1] = hi; break;
  }
}

// the same value out of a BYTE_STREAM_SPLIT region v of nn values: byte j of value idx lies at v[j * nn + idx]
QH_PQ_HD inline void qh_pq_read_value_bss(const pq_u8* v, pq_u64 nn, pq_u64 idx, pq_u32 phys, pq_u32 flba, pq_u64* lo, pq_u64* hi) {
  if (phys == QH_PQ_P_32) {
    pq_u32 x = 0;
    for (pq_u32 j = 0; j < 4; ++j) x |= (pq_u32)v[j * nn + idx] << (8 * j);
    const pq_i64 s = (pq_i64)(int)x;
    *lo = (pq_u64)s; *hi = s < 0 ? ~0ull : 0ull;
  } else if (phys == QH_PQ_P_64) {
    pq_u64 x = 0;
    for (pq_u32 j = 0; j < 8; ++j) x |= (pq_u64)v[j * nn + idx] << (8 * j);
    *lo = x; *hi = (x >> 63) ? ~0ull : 0ull;
  } else {
    pq_u64 l = (v[idx] & 0x80u) ? ~0ull : 0ull, h = l;
    for (pq_u32 i = 0; i < flba; ++i) { h = (h << 8) | (l >> 56); l = (l << 8) | v[i * nn + idx]; }
    *lo = l; *hi = h;
  }
}

QH_PQ_HD inline pq_u32 qh_pq_phys_bytes(pq_u32 phys, pq_u32 flba) { return phys == QH_PQ_P_32 ? 4u : phys == QH_PQ_P_64 ? 8u : phys == QH_PQ_P_FLBA ? flba : 0u; }

// ---- a BYTE_ARRAY length chain in a region of `size` bytes. Before the 4 length bytes at q are read: has_prefix. Before the
// length is followed (q becomes q + 4 + len): fits.
QH_PQ_HD inline bool qh_pq_chain_has_prefix(pq_u64 q, pq_u64 size) { return size >= 4 && q <= size - 4; }
QH_PQ_HD inline bool qh_pq_chain_fits(pq_u64 q, pq_u64 size, pq_u32 len) { return (pq_u64)len <= size - (q + 4); }

#endif  // QHIP_PARQUET_INC
