"""What getting a CSV table onto the device costs: about --gb GB of lineitem-shaped text (synth.lineitem written
once with pyarrow.csv.write_csv, quoting_style="none", into a temporary directory), and per measurement the median of --runs
calls after --warmup calls, each ending in a device synchronise:

  (a) host path    datasource.read_csv(device=False) — Arrow C++ parse with --threads threads — plus the eager upload of the
                   columns Q1 reads (all seven of this table)
  (b) device path  datasource.read_csv(device=True) as a whole call: mmap, upload of the text, the kernels, both host waits
  (c) floor        one plain host-to-device copy of the file's bytes out of the same mapping (hipMemcpy, pageable source)
  (d) passes       HIP events around the device path's passes (timing on, calls of their own): upload, k_csv_scan, record starts
                   (scan of the chunk counts + k_csv_scan<true>), k_csv_decode, Utf8 (offset scans + k_csv_copy_utf8), with the
                   GB/s of file bytes each pass amounts to

(a) .. (c) alternate in one process, --repeat times.

--quoted: the same table written with Arrow's default quoting (every string value in quotes) plus a comment column l_comment
whose values hold commas and, in a few percent of the rows, a doubled quote; the context decodes at grammar level 2
(qhip_ctx_set_csv_grammar), without which such a file takes the host path.

--floats repr: two more columns, Float64, written as the shortest round-trip text of random doubles (17 digits, what `repr` and
every writer emit); the context decodes at float_parse level 2 (qhip_ctx_set_float_parse), without which the file's first such
value sends it to the host. --floats round6: the same values rounded to 6 decimals, which level 1 decodes too; (a) .. (c) run at
--float-parse (default 1) and (d) is taken at level 1, 2, 1, 2 on the one file: what the level-2 kinds cost a file that did
not need them.

    python tools/csv_decode_timing.py [--gb 1.0] [--runs 10] [--warmup 2] [--repeat 2] [--threads 16] [--quoted]
                                      [--floats repr|round6] [--float-parse 1|2]
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

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import pyarrow.csv as pacsv  # noqa: E402

import qurious_amd as q  # noqa: E402
from qurious_amd import datasource, synth  # noqa: E402
from qurious_amd._ffi import DeviceTable  # noqa: E402

PASSES = ["upload", "k_csv_scan", "record starts", "k_csv_decode", "Utf8 offsets + k_csv_copy_utf8"]


COMMENT_WORDS = ["carefully", "final deposits", "blithely ironic", "requests, packages", "slyly even", "accounts sleep, furiously", "pending", "quickly"]


def comment_column(first_row, n):
    """TPC-H-like comments of 16 to 80 bytes out of a pool of 4096: every one holds a comma, one in 32 (3 %) a word in quotes"""
    pool = []
    for k in range(4096):
        first = COMMENT_WORDS[k % 8]
        if k % 32 == 5:
            first = '"' + first + '"'
        pool.append(first + ", " + COMMENT_WORDS[(k // 8) % 8] + (" " + COMMENT_WORDS[(k // 64) % 8] if k % 3 else ""))
    idx = (np.arange(first_row, first_row + n, dtype=np.int64) * 2654435761 >> 7) % len(pool)
    return pa.array(pool, pa.string()).take(pa.array(idx))


FLOAT_NAMES = ["f_reading", "f_ratio"]


def float_columns(first_row, n, mode):
    """two Float64 columns of measurement-like values over ten decades, both signs. mode "repr": random doubles, which Arrow's
    writer spells with their shortest round-trip digits (17, or 16 about as often); "round6": the same values rounded to 6
    decimals, at most 13 digits: Clinger's range, what float_parse level 1 decodes"""
    rng = np.random.default_rng(first_row + 1)
    cols = []
    for _ in FLOAT_NAMES:
        v = rng.standard_normal(n) * np.power(10.0, rng.integers(-3, 7, n))
        cols.append(pa.array(np.round(v, 6) if mode == "round6" else v))
    return cols


def write_file(path, target_bytes, quoted=False, floats=None):
    """lineitem rows until the file has about target_bytes; returns the row count"""
    step, rows = 1 << 20, 0
    with open(path, "wb") as f:
        while f.tell() < target_bytes:
            tbl = pa.Table.from_batches([synth.lineitem_batch(rows, step)])
            if floats:
                for name, col in zip(FLOAT_NAMES, float_columns(rows, step, floats)):
                    tbl = tbl.append_column(name, col)
            if quoted:
                tbl = tbl.append_column("l_comment", comment_column(rows, step))
            opts = pacsv.WriteOptions(include_header=rows == 0) if quoted else pacsv.WriteOptions(include_header=rows == 0, quoting_style="none")
            pacsv.write_csv(tbl, f, write_options=opts)
            rows += step
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
    ap.add_argument("--quoted", action="store_true", help="Arrow's default quoting and a comment column with commas and doubled quotes; grammar level 2")
    ap.add_argument("--floats", choices=["repr", "round6"], help="two Float64 columns: shortest round-trip spellings of random doubles / the same rounded to 6 decimals")
    ap.add_argument("--float-parse", type=int, choices=[1, 2], help="the context's float_parse level (default: 2 with --floats repr, else 1)")
    args = ap.parse_args()
    pa.set_cpu_count(args.threads)
    ctx = q.get_context()
    schema = pa.schema([pa.field(f.name, f.type) for f in synth.LINEITEM_SCHEMA])
    float_parse = args.float_parse or (2 if args.floats == "repr" else 1)
    ctx.set_float_parse(float_parse)
    if args.floats:
        for name in FLOAT_NAMES:
            schema = schema.append(pa.field(name, pa.float64()))
    if args.quoted:
        schema = schema.append(pa.field("l_comment", pa.string()))
        ctx.set_csv_grammar(2)
    hip = C.CDLL(None)   # (libqhip.so is loaded globally and brings the HIP runtime with it)
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "lineitem.csv")
        rows = write_file(path, int(args.gb * 1e9), args.quoted, args.floats)
        nbytes = os.path.getsize(path)
        kind = ", default quoting, grammar 2" if args.quoted else ""
        if args.floats:
            kind += f", two Float64 columns ({args.floats}), float_parse {float_parse}"
        print(f"device {ctx.device_name()}; {path}: {nbytes} bytes, {rows} rows, {nbytes / rows:.1f} bytes per record{kind}; median (min) of {args.runs} calls "
              f"after {args.warmup} warm-up calls; host parse with {args.threads} threads", flush=True)

        def host_path():
            t = datasource.read_csv(path, schema=schema, device=False)
            dev = DeviceTable.from_batches(ctx, t.schema(), t.data, lazy=False)
            ctx.synchronize()
            return dev

        def device_path():
            t = datasource.read_csv(path, schema=schema, device=True)
            assert t.decoded_on_device
            ctx.synchronize()
            return t.device_table()

        dst = C.c_void_p()
        assert hip.hipMalloc(C.byref(dst), nbytes + 64) == 0
        f = open(path, "rb")
        m = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        src = pa.py_buffer(m)

        def floor():
            assert hip.hipMemcpy(dst, C.c_void_p(src.address), nbytes, 1) == 0   # (hipMemcpyHostToDevice; returns when the copy is done)

        assert host_path().num_rows == device_path().num_rows == rows
        for rep in range(args.repeat):
            for name, fn in (("(a) host parse + upload", host_path), ("(b) device path, whole call", device_path), ("(c) plain copy of the file", floor)):
                med, low = median_ms(fn, args.runs, args.warmup)
                print(f"run {rep + 1} {name:30s} {med:9.2f} ms (min {low:9.2f})  {nbytes / med / 1e6:8.2f} GB/s of file bytes", flush=True)
        ctx.set_timing(True)
        # (a round6 file is inside both levels' grammar: the passes at either level, alternating, are what the level-2 kinds cost
        # a file that did not need them)
        levels = [1, 2, 1, 2] if args.floats == "round6" else [float_parse]
        for level in levels:
            ctx.set_float_parse(level)
            per = []
            for _ in range(args.warmup + args.runs):
                device_path()
                per.append(ctx.csv_pass_ms())
            per = per[args.warmup:]
            kernels = 0.0
            tag = f"(d) float_parse {level} " if args.floats else "(d) "
            for k, name in enumerate(PASSES):
                med = statistics.median(p[k] for p in per)
                kernels += med if k else 0.0
                print(f"{tag}{name:32s} {med:9.3f} ms  {nbytes / max(med, 1e-6) / 1e6:9.1f} GB/s of file bytes", flush=True)
            print(f"{tag}kernels together (all but the upload) {kernels:9.3f} ms  {nbytes / max(kernels, 1e-6) / 1e6:9.1f} GB/s of file bytes", flush=True)
        ctx.set_timing(False)
        del src
        m.close()
        f.close()
        hip.hipFree(dst)


if __name__ == "__main__":
    main()
