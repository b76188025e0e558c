"""File-backed tables (reference: datasource/file/{csv,parquet,json}.rs + provider/table.rs:32-41).

The reference's readers load the whole file into a host `MemoryTable` with arrow-rs' readers and every scan hands every
column to the operators (`Scan.projections` is always None, planner/mod.rs:251-256). Here the file is decoded on the host
with Arrow C++ (pyarrow) into the same `MemoryTable`, whose device copy is LAZY: a column is uploaded to HBM the first time
an operator or an export reads it (qhip_table_from_arrow_lazy), so the columns a query never touches never cross PCIe —
for TPC-H Q1 that is 7 of lineitem's 16 columns. Parquet additionally skips the untouched column chunks on disk when a
`columns=` subset is requested up front.

CSV files can instead be decoded ON THE DEVICE (`read_csv(device=True)` / QHIP_CSV_DEVICE=1, off by default): the
text crosses PCIe once and unread columns are never parsed; a file outside the device's strict grammar takes the host path.
So can Parquet files (`read_parquet(device=True)` / QHIP_PARQUET_DEVICE=1, off by default): only the projected
column chunks cross PCIe; format level 1 (uncompressed, data pages V1, flat columns), everything else takes the host path.
And newline-delimited JSON (`read_json(device=True)` / QHIP_JSON_DEVICE=1, off by default): flat objects of
scalar values; nested values, \\uXXXX escapes and every lenient spelling take the host path.

Divergence note: with `schema=None` the column types come from Arrow C++'s CSV / JSON type inference, which is close to
but not the same code as arrow-rs' `Format::infer_schema` (csv.rs:58); pass an explicit schema for exact control."""
from __future__ import annotations

from typing import Optional, Sequence

import pyarrow as pa

from ._ffi import DeviceTable
from .plan import MemoryTable


class CsvReadOptions:
    """datasource/file/csv.rs:15-31. Defaults: header row, ',' delimiter; quote / escape None = arrow-rs' Format defaults
    (csv.rs:42-51 only overrides them when given): fields may be quoted with '"', a quote inside is doubled, no escape
    character."""

    def __init__(self, has_header: bool = True, delimiter: str = ",", quote: Optional[str] = None, escape: Optional[str] = None):
        self.has_header, self.delimiter, self.quote, self.escape = has_header, delimiter, quote, escape


def _table_of(tbl: pa.Table, batch_rows: Optional[int]) -> MemoryTable:
    tbl = tbl.combine_chunks()
    batches = tbl.to_batches(max_chunksize=batch_rows) if batch_rows else tbl.to_batches()
    return MemoryTable(tbl.schema, batches, lazy_upload=True)


class DeviceDecodedTable(MemoryTable):
    """A file decoded on the device (qhip_table_from_csv, qhip_table_from_parquet, qhip_table_from_json): `device_table()` IS the decoded table, nothing
    was parsed on the host. `.data` — what the oracle, `insert` and `delete` work on — is downloaded the first time somebody asks for it;
    from then on MemoryTable's rule holds (the device copy is kept for as long as `data` holds the very batches it stands for)."""

    decoded_on_device = True

    def __init__(self, schema: pa.Schema, device: DeviceTable):
        self._schema = schema
        self._data = None
        self.lazy_upload = True
        self._device = device
        self._device_of = None

    @property
    def data(self):
        if self._data is None:
            self._data = self._device.to_batches()
            self._device_of = tuple(self._data)
        return self._data

    @data.setter
    def data(self, value):
        self._data = value

    def device_table(self) -> DeviceTable:
        if self._data is None:
            return self._device
        return super().device_table()


DeviceCsvTable = DeviceDecodedTable   # (the name it had when CSV was the only format decoded on the device)


def _host_read_csv(path, o, schema, batch_rows, columns) -> MemoryTable:
    import pyarrow.csv as pacsv
    names = [f.name for f in schema] if (schema is not None and not o.has_header) else None
    read = pacsv.ReadOptions(autogenerate_column_names=(not o.has_header and names is None), column_names=names)
    parse = pacsv.ParseOptions(delimiter=o.delimiter, quote_char=o.quote if o.quote else '"', escape_char=o.escape if o.escape else False)
    conv = pacsv.ConvertOptions(column_types=schema) if schema is not None else pacsv.ConvertOptions()
    if columns is not None:
        conv.include_columns = list(columns)
    return _table_of(pacsv.read_csv(path, read_options=read, parse_options=parse, convert_options=conv), batch_rows)


def _device_read_csv(path, o, schema, batch_rows, columns) -> Optional[MemoryTable]:
    """the device path, or None when the file needs the host path (QHIP_UNSUPPORTED)"""
    import mmap
    import os
    import pyarrow.csv as pacsv
    from ._ffi import UnsupportedError, get_context
    if schema is None:
        # the types the host path would infer: Arrow C++ infers them from the first block it reads
        read = pacsv.ReadOptions(autogenerate_column_names=not o.has_header)
        parse = pacsv.ParseOptions(delimiter=o.delimiter, quote_char=o.quote if o.quote else '"', escape_char=o.escape if o.escape else False)
        try:
            with pacsv.open_csv(path, read_options=read, parse_options=parse) as rd:
                schema = rd.schema
        except pa.ArrowInvalid:
            return None
    schema = pa.schema([pa.field(f.name, f.type) for f in schema])   # as the host parse returns it: every field nullable, no metadata
    idx = None
    if columns is not None:
        idx = [schema.get_field_index(c) for c in columns]
        if any(k < 0 for k in idx):
            return None
    if os.path.getsize(path) == 0:
        return None
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
        try:
            dev = DeviceTable.from_csv_bytes(get_context(), schema, m, has_header=o.has_header, delimiter=o.delimiter, quote=o.quote if o.quote else '"',
                                             escape=o.escape, columns=idx, batch_rows=batch_rows)
        except UnsupportedError:
            return None
    out_schema = schema if idx is None else pa.schema([schema.field(k) for k in idx])
    return DeviceCsvTable(out_schema, dev)


def read_csv(path: str, options: Optional[CsvReadOptions] = None, schema: Optional[pa.Schema] = None,
             batch_rows: Optional[int] = 1 << 20, device: Optional[bool] = None, columns: Optional[Sequence[str]] = None) -> MemoryTable:
    """read_csv (datasource/file/csv.rs:33-70): the whole file becomes one in-memory table. `columns`: the names of the
    columns to read, in output order (None = all).

    device=True (None: the environment's QHIP_CSV_DEVICE, default 0): the file's text is decoded on the device
    (qhip_table_from_csv) and the result's `decoded_on_device` is True; a file outside the device's strict
    grammar falls back silently to the host parse below, which also produces every error message. What that grammar holds is
    the context's level (`Context.set_csv_grammar` / QHIP_CSV_GRAMMAR): 1, the default, plain fields only; 2 also quoted fields,
    Boolean and Timestamp columns — with `schema=None` the types Arrow infers pass through as they are. Float columns have a
    level of their own (`Context.set_float_parse` / QHIP_FLOAT_PARSE): 1, the default, decodes a Float64 value only in Clinger's
    exact range, so a file with one 17-digit `repr` value takes the host parse, and so does a Float32 column; 2 converts every
    spelling -?[0-9]+(.[0-9]+)?([eE][-+]?[0-9]+)? on the device, correctly rounded, and admits Float32 columns."""
    import os
    o = options or CsvReadOptions()
    if device is None:
        device = os.environ.get("QHIP_CSV_DEVICE", "0") not in ("", "0")
    if device:
        t = _device_read_csv(path, o, schema, batch_rows, columns)
        if t is not None:
            return t
    t = _host_read_csv(path, o, schema, batch_rows, columns)
    t.decoded_on_device = False
    return t


def _device_read_parquet(path, columns, batch_rows) -> Optional[MemoryTable]:
    """the device path, or None when the file needs the host path (QHIP_UNSUPPORTED, or a file Arrow itself cannot open)"""
    import mmap
    import os
    import pyarrow.parquet as pq
    from ._ffi import UnsupportedError, get_context
    try:
        schema = pq.read_schema(path)
        if os.path.getsize(path) == 0:
            return None
    except (pa.ArrowException, OSError):
        return None
    idx = None
    if columns:
        idx = [schema.get_field_index(c) for c in columns]
        if any(k < 0 for k in idx):
            return None
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
        try:
            dev = DeviceTable.from_parquet_bytes(get_context(), schema.remove_metadata(), m, columns=idx, batch_rows=batch_rows)
        except UnsupportedError:
            return None
    # the schema as the host read returns it (its metadata included), cut to the projection
    out_schema = schema if idx is None else pa.schema([schema.field(k) for k in idx], metadata=schema.metadata)
    return DeviceDecodedTable(out_schema, dev)


def read_parquet(path: str, columns: Optional[Sequence[str]] = None, batch_rows: Optional[int] = 1 << 20, device: Optional[bool] = None) -> MemoryTable:
    """read_parquet (datasource/file/parquet.rs): `columns` (optional) is a projection applied while reading the file.

    device=True (None: the environment's QHIP_PARQUET_DEVICE, default 0): the footer and one header per page are read on the
    host, the bytes of the projected column chunks alone cross PCIe and the pages are decoded on the device
    (qhip_table_from_parquet); the result's `decoded_on_device` is True. What the device decodes is the context's
    format level (`Context.set_parquet_format` / QHIP_PARQUET_FORMAT). Level 1, the default: UNCOMPRESSED chunks — write with
    `compression="NONE"`; pyarrow's default, Snappy, takes the host path — data pages V1, PLAIN and dictionary encodings, flat
    columns. Level 2 also decodes SNAPPY chunks, unpacked on the device; brotli still takes the host path, and so
    does zstd unless the codec set (`Context.set_parquet_codecs` / QHIP_PARQUET_CODECS), a third independent switch, is 2: then
    ZSTD chunks are unpacked on the device as well (the frames' content checksums are not verified). So does gzip unless the
    gzip switch (`Context.set_parquet_gzip` / QHIP_PARQUET_GZIP), a fourth independent one, is on: then GZIP chunks are
    inflated on the device (the members' CRC32 is not verified; zlib-wrapped pages still take the host path). And so does lz4
    unless the lz4 switch (`Context.set_parquet_lz4` / QHIP_PARQUET_LZ4), a fifth independent one, is on: then LZ4_RAW chunks
    (`compression="lz4"`) and chunks of the legacy LZ4 id, Hadoop-framed or bare, are unpacked on the device.
    Which page kinds and encodings are decoded is a second, independent switch, the encoding set
    (`Context.set_parquet_encodings` / QHIP_PARQUET_ENCODINGS). Set 1, the default: data pages V1 with PLAIN or dictionary
    values. Set 2 also decodes data pages V2 (`data_page_version="2.0"`), RLE Boolean values, BYTE_STREAM_SPLIT,
    DELTA_BINARY_PACKED and DELTA_LENGTH_BYTE_ARRAY. DELTA_BYTE_ARRAY takes the host path unless the DELTA_BYTE_ARRAY switch
    (`Context.set_parquet_delta_byte_array` / QHIP_PARQUET_DBA), a sixth independent one, is on: then such pages of Utf8 columns
    and of FIXED_LEN_BYTE_ARRAY decimals are decoded on the device (a page whose first prefix length is not 0 still takes the
    host path).
    Every other file falls back silently to the host read below, which also produces every error message."""
    import os
    import pyarrow.parquet as pq
    if device is None:
        device = os.environ.get("QHIP_PARQUET_DEVICE", "0") not in ("", "0")
    if device:
        t = _device_read_parquet(path, columns, batch_rows)
        if t is not None:
            return t
    t = _table_of(pq.read_table(path, columns=list(columns) if columns else None), batch_rows)
    t.decoded_on_device = False
    return t


def _host_read_json(path, schema, batch_rows, columns) -> MemoryTable:
    import pyarrow.json as pajson
    tbl = pajson.read_json(path, parse_options=pajson.ParseOptions(explicit_schema=schema)) if schema is not None else pajson.read_json(path)
    if columns is not None:
        tbl = tbl.select(list(columns))
    return _table_of(tbl, batch_rows)


def _device_read_json(path, schema, batch_rows, columns) -> Optional[MemoryTable]:
    """the device path, or None when the file needs the host path (QHIP_UNSUPPORTED, or a file Arrow itself cannot open)"""
    import mmap
    import os
    import pyarrow.json as pajson
    from ._ffi import UnsupportedError, get_context
    try:
        if os.path.getsize(path) == 0:
            return None
        if schema is None:
            # the types the host path infers from the first block it reads; a later block that would change one of them, or add
            # a key, fails the strict decode and the file takes the host read
            with pajson.open_json(path) as rd:
                schema = rd.schema
    except (pa.ArrowException, OSError):
        return None
    if len(set(schema.names)) != len(schema.names) or not all(f.nullable for f in schema):
        return None   # (the host refuses a record in which a required field is absent or null: such a schema stays with it)
    schema = pa.schema([pa.field(f.name, f.type) for f in schema])   # as the host parse returns it: no metadata
    idx = None
    if columns is not None:
        idx = [schema.get_field_index(c) for c in columns]
        if any(k < 0 for k in idx) or len(set(idx)) != len(idx):
            return None
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
        try:
            dev = DeviceTable.from_json_bytes(get_context(), schema, m, columns=idx, batch_rows=batch_rows)
        except UnsupportedError:
            return None
    out_schema = schema if idx is None else pa.schema([schema.field(k) for k in idx])
    return DeviceDecodedTable(out_schema, dev)


def read_json(path: str, batch_rows: Optional[int] = 1 << 20, schema: Optional[pa.Schema] = None, columns: Optional[Sequence[str]] = None,
              device: Optional[bool] = None) -> MemoryTable:
    """read_json (datasource/file/json.rs): newline-delimited JSON, one object per line. `schema`: the keys and their types
    (Arrow's `explicit_schema`; None: Arrow infers them); `columns`: the names of the columns to keep, in output order.

    device=True (None: the environment's QHIP_JSON_DEVICE, default 0): the file's text is decoded on the device
    (qhip_table_from_json) and the result's `decoded_on_device` is True. With `schema=None` the device takes the
    types Arrow infers from the file's first block. A file outside the device's strict grammar — nested values, \\uXXXX escapes,
    unknown or repeated keys, lenient number spellings, ... — falls back silently to the host read below, which also produces
    every error message. Float64 numbers decode in Clinger's exact range only, and a Float32 field in the schema takes the host
    read, unless the context's float_parse level (`Context.set_float_parse` / QHIP_FLOAT_PARSE) is 2: then every JSON number is
    converted on the device, correctly rounded, to Float64 or Float32."""
    import os
    if device is None:
        device = os.environ.get("QHIP_JSON_DEVICE", "0") not in ("", "0")
    if device:
        t = _device_read_json(path, schema, batch_rows, columns)
        if t is not None:
            return t
    t = _host_read_json(path, schema, batch_rows, columns)
    t.decoded_on_device = False
    return t
