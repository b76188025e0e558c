"""What getting a Parquet table onto the device costs: about --gb GB of lineitem-shaped rows (synth.lineitem written
once with pyarrow.parquet, compression="NONE", row groups of 2^20 rows, into a temporary directory), and per measurement the
median of --runs calls after --warmup calls, each ending in a device synchronise:

  (a) host path    datasource.read_parquet(device=False) — Arrow C++ read with --threads threads — plus the eager upload of the
                   decoded columns
  (b) device path  datasource.read_parquet(device=True) as a whole call: read_schema, mmap, footer and page walk, upload of the
                   projected chunks, the kernels, the one host wait
  (c) floor        one plain host-to-device copy of as many bytes as the projected chunks have, out of the same mapping
                   (hipMemcpy, pageable source)
  (d) passes       HIP events around the device path's passes (timing on, calls of their own): upload, k_pq_levels, k_pq_strings,
                   k_pq_values, Utf8 (offset scans + k_csv_copy_utf8), with the GB/s of chunk bytes each pass amounts to

(a) .. (c) alternate in one process, --repeat times. --columns a,b,c reads a projection: the other columns' chunks stay on disk.

--compression snappy writes the same rows with pyarrow's defaults (Snappy) and sets format level 2 (Context.set_parquet_format),
without which such a file takes the host path. (d) then also has the unpack pass (k_pq_unsnap, between the upload and
k_pq_levels) with the GB/s of uncompressed bytes it produces, and the header line says how many bytes the projected chunks have
compressed and uncompressed; (c) copies the compressed bytes, which are what crosses PCIe. --compression zstd writes them with
ZSTD (the writer's default level) and sets codec set 2 (Context.set_parquet_codecs); the unpack pass is then k_pq_unzstd.
--compression gzip writes them with GZIP at level 6 — zlib's own default and what most writers use; pyarrow's default, 9, takes
minutes per GB to write — and sets the gzip switch (Context.set_parquet_gzip); the unpack pass is then k_pq_ungzip. While a
compressed file is written a progress line goes to stderr every 8 row groups. --compression lz4 writes them with LZ4_RAW, one
bare LZ4 block per page, and sets the lz4 switch (Context.set_parquet_lz4); the unpack pass is then k_pq_unlz4.

--page-version 2.0 writes data pages V2 and --encoding plain|delta|bss writes without dictionaries, with PLAIN values, with
DELTA_BINARY_PACKED integers and dates and DELTA_LENGTH_BYTE_ARRAY strings, or with BYTE_STREAM_SPLIT numbers; either sets
encoding set 2 (Context.set_parquet_encodings). (d) then also has the delta pass (k_pq_delta, between k_pq_levels and
k_pq_strings); the time of k_pq_values includes k_pq_values_ext, which runs right behind it.

--encoding dba writes without dictionaries, data pages V2 whatever --page-version says, DELTA_BYTE_ARRAY for the Utf8 and decimal
columns (what arrow-rs falls back to at writer version 2) and PLAIN for the rest, and sets the DELTA_BYTE_ARRAY switch
(Context.set_parquet_delta_byte_array) and encoding set 2. (d) then has the delta pass (k_pq_delta_dba: both length streams of
every such page) and, on a line of its own, the fill pass (k_pq_dba_fill: the decimal pages in front of the host wait, the Utf8
columns behind it); "Utf8" is then the offset scans and k_pq_dba_copy.

    python tools/parquet_decode_timing.py [--gb 1.0] [--runs 10] [--warmup 2] [--repeat 2] [--threads 16] [--columns l_quantity,l_shipdate]
                                          [--compression none|snappy|zstd|gzip|lz4] [--page-version 1.0|2.0] [--encoding plain|delta|bss|dba]
"""
import argparse
import ctypes as C
import mmap
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pyarrow as pa  # noqa: E402
import pyarrow.parquet as pq  # noqa: E402

import qurious_amd as q  # noqa: E402
from qurious_amd import datasource, synth  # noqa: E402
from qurious_amd._ffi import DeviceTable  # noqa: E402

PASSES = ["upload", "k_pq_levels", "k_pq_strings", "k_pq_values", "Utf8 offsets + k_csv_copy_utf8"]


def writer_options(schema, page_version, encoding):
    kw = {"data_page_version": page_version}
    if encoding:
        kw["use_dictionary"] = False
    if encoding == "delta":
        kw["column_encoding"] = {f.name: "DELTA_LENGTH_BYTE_ARRAY" if pa.types.is_string(f.type) else "DELTA_BINARY_PACKED" for f in schema
                                 if pa.types.is_string(f.type) or pa.types.is_integer(f.type) or pa.types.is_date32(f.type)}
    if encoding == "dba":
        kw["data_page_version"] = "2.0"
        kw["column_encoding"] = {f.name: "DELTA_BYTE_ARRAY" for f in schema if pa.types.is_string(f.type) or pa.types.is_decimal(f.type)}
    if encoding == "bss":
        kw["column_encoding"] = {f.name: "BYTE_STREAM_SPLIT" for f in schema
                                 if pa.types.is_integer(f.type) or pa.types.is_floating(f.type) or pa.types.is_decimal(f.type) or pa.types.is_date32(f.type)}
    return kw


def write_file(path, target_bytes, compression="none", page_version="1.0", encoding=None):
    """lineitem rows, one row group per 2^20 of them, until the file has about target_bytes; returns the row count.
    compression="snappy" / "zstd" / "gzip" / "lz4": the rows the uncompressed file would have, written with pyarrow's defaults /
    with ZSTD / with GZIP at level 6 / with LZ4_RAW"""
    step, rows = 1 << 20, 0
    schema = pa.schema([pa.field(f.name, f.type) for f in synth.LINEITEM_SCHEMA])
    group = lambda first: pa.Table.from_batches([synth.lineitem_batch(first, step)]).cast(schema)   # noqa: E731
    kw = writer_options(schema, page_version, encoding)
    if compression != "none":
        pq.write_table(group(0), path + ".one", compression="NONE", row_group_size=step)
        groups = -(-target_bytes // os.path.getsize(path + ".one"))
        os.remove(path + ".one")
        if compression == "gzip":
            kw["compression_level"] = 6
        with pq.ParquetWriter(path, schema, compression=compression, **kw) as w:
            for g in range(groups):
                w.write_table(group(g * step), row_group_size=step)
                if g % 8 == 7:
                    print(f"written {g + 1} of {groups} row groups", file=sys.stderr, flush=True)
        return groups * step
    with pq.ParquetWriter(path, schema, compression="NONE", **kw) as w:
        while True:
            w.write_table(group(rows), row_group_size=step)
            rows += step
            if os.path.getsize(path) >= target_bytes:
                return rows


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--columns", type=str, default="", help="comma-separated projection (default: every column)")
    ap.add_argument("--compression", choices=["none", "snappy", "zstd", "gzip", "lz4"], default="none",
                    help="snappy: pyarrow's defaults, decoded at format level 2; zstd: decoded at codec set 2; gzip / lz4: decoded with the gzip / lz4 switch on")
    ap.add_argument("--page-version", choices=["1.0", "2.0"], default="1.0", help="2.0: data pages V2, decoded at encoding set 2")
    ap.add_argument("--encoding", choices=["plain", "delta", "bss", "dba"], default=None,
                    help="no dictionaries; delta and bss are decoded at encoding set 2, dba (data pages V2) with the DELTA_BYTE_ARRAY switch on as well")
    args = ap.parse_args()
    pa.set_cpu_count(args.threads)
    columns = [c for c in args.columns.split(",") if c] or None
    ctx = q.get_context()
    if args.compression == "snappy":
        ctx.set_parquet_format(2)
    if args.compression == "zstd":
        ctx.set_parquet_codecs(2)
    if args.compression == "gzip":
        ctx.set_parquet_gzip(1)
    if args.compression == "lz4":
        ctx.set_parquet_lz4(1)
    if args.encoding == "dba":
        args.page_version = "2.0"
        ctx.set_parquet_delta_byte_array(1)
    if args.page_version == "2.0" or args.encoding in ("delta", "bss"):
        ctx.set_parquet_encodings(2)
    hip = C.CDLL(None)   # (libqhip.so is loaded globally and brings the HIP runtime with it)
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "lineitem.parquet")
        rows = write_file(path, int(args.gb * 1e9), args.compression, args.page_version, args.encoding)
        nbytes = os.path.getsize(path)
        md = pq.ParquetFile(path).metadata
        names = md.schema.names
        want = set(columns) if columns else set(names)
        chunk_bytes = sum(md.row_group(g).column(c).total_compressed_size for g in range(md.num_row_groups) for c in range(md.num_columns) if names[c] in want)
        plain_bytes = sum(md.row_group(g).column(c).total_uncompressed_size for g in range(md.num_row_groups) for c in range(md.num_columns) if names[c] in want)
        values = args.encoding or "writer's default"
        print(f"device {ctx.device_name()}; {path}: {nbytes} bytes, {rows} rows in {md.num_row_groups} row groups, columns {sorted(want)}: {chunk_bytes} bytes of "
              f"projected chunks ({args.compression}, pages V{args.page_version[0]}, {values} values; {plain_bytes} bytes uncompressed); median (min) of {args.runs} calls after {args.warmup} warm-up calls; host read with {args.threads} threads", flush=True)

        def host_path():
            t = datasource.read_parquet(path, columns, device=False)
            dev = DeviceTable.from_batches(ctx, t.schema(), t.data, lazy=False)
            ctx.synchronize()
            return dev

        def device_path():
            t = datasource.read_parquet(path, columns, device=True)
            assert t.decoded_on_device
            ctx.synchronize()
            return t.device_table()

        dst = C.c_void_p()
        assert hip.hipMalloc(C.byref(dst), chunk_bytes + 64) == 0
        f = open(path, "rb")
        m = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        src = pa.py_buffer(m)

        def floor():
            assert hip.hipMemcpy(dst, C.c_void_p(src.address), chunk_bytes, 1) == 0   # (hipMemcpyHostToDevice; returns when the copy is done)

        assert host_path().num_rows == device_path().num_rows == rows
        for rep in range(args.repeat):
            for name, fn in (("(a) host read + upload", host_path), ("(b) device path, whole call", device_path), ("(c) plain copy of the chunks", floor)):
                med, low = median_ms(fn, args.runs, args.warmup)
                print(f"run {rep + 1} {name:30s} {med:9.2f} ms (min {low:9.2f})  {chunk_bytes / med / 1e6:8.2f} GB/s of chunk bytes", flush=True)
        ctx.set_timing(True)
        per = []
        for _ in range(args.warmup + args.runs):
            device_path()
            per.append(ctx.parquet_pass_ms() + [ctx.parquet_unpack_ms(), ctx.parquet_delta_ms(), ctx.parquet_fill_ms()])
        ctx.set_timing(False)
        per = per[args.warmup:]
        kernels = 0.0
        for k, name in enumerate(PASSES):
            med = statistics.median(p[k] for p in per)
            kernels += med if k else 0.0
            print(f"(d) {name:32s} {med:9.3f} ms  {chunk_bytes / max(med, 1e-6) / 1e6:9.1f} GB/s of chunk bytes", flush=True)
            if k == 0 and args.compression != "none":
                med = statistics.median(p[5] for p in per)
                kernels += med
                print(f"(d) { {'snappy': 'k_pq_unsnap', 'zstd': 'k_pq_unzstd', 'gzip': 'k_pq_ungzip', 'lz4': 'k_pq_unlz4'}[args.compression] + ' (unpack)':32s} {med:9.3f} ms  {plain_bytes / max(med, 1e-6) / 1e6:9.1f} GB/s of uncompressed bytes", flush=True)
            if k == 1 and args.encoding in ("delta", "dba"):
                med = statistics.median(p[6] for p in per)
                kernels += med
                print(f"(d) {'k_pq_delta_dba' if args.encoding == 'dba' else 'k_pq_delta':32s} {med:9.3f} ms  {chunk_bytes / max(med, 1e-6) / 1e6:9.1f} GB/s of chunk bytes", flush=True)
            if k == 4 and args.encoding == "dba":
                med = statistics.median(p[7] for p in per)
                kernels += med
                print(f"(d) {'k_pq_dba_fill (both places)':32s} {med:9.3f} ms  {chunk_bytes / max(med, 1e-6) / 1e6:9.1f} GB/s of chunk bytes", flush=True)
        print(f"(d) kernels together (all but the upload) {kernels:9.3f} ms  {chunk_bytes / max(kernels, 1e-6) / 1e6:9.1f} GB/s of chunk bytes", flush=True)
        del src
        m.close()
        f.close()
        hip.hipFree(dst)


if __name__ == "__main__":
    main()
