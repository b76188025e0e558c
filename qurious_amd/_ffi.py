"""ctypes binding of libqhip.so (include/qhip.h) — the only way Python reaches the HIP backend.

There is deliberately no fallback: if the shared library is missing this module raises at import
of the symbol table, and if no gfx950 device is visible ``get_context()`` raises. Nothing under
``oracle/`` is ever imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import List, Optional, Sequence

import pyarrow as pa

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libqhip.so")

# status codes (include/qhip.h)
QHIP_OK, QHIP_INVALID_ARGUMENT, QHIP_UNSUPPORTED, QHIP_HIP_ERROR, QHIP_OUT_OF_MEMORY, QHIP_EXEC_ERROR, QHIP_RCCL_ERROR, QHIP_RETRY = range(8)


class QuriousError(Exception):
    """Mirror of qurious::error::Error (error.rs:5-31); ``code`` is the qhip_status."""

    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


class InternalError(QuriousError):
    pass


class ArrowError(QuriousError):
    pass


class UnsupportedError(QuriousError):
    """QHIP_UNSUPPORTED: a valid plan the HIP backend does not accelerate (a Rust shim would fall back to the CPU node)."""


class HipError(QuriousError):
    pass


class RetryInput(QuriousError):
    """QHIP_RETRY: a hash join below ran without waiting for its output size and its room did not hold — the operator
    that reports it re-executes its input (plan.py: `_retrying`); never reaches a caller of ``execute()``."""


def _raise(code: int, msg: str):
    if code == QHIP_RETRY:
        raise RetryInput(code, msg)
    if code == QHIP_UNSUPPORTED:
        raise UnsupportedError(code, msg)
    if code in (QHIP_HIP_ERROR, QHIP_OUT_OF_MEMORY, QHIP_RCCL_ERROR):
        raise HipError(code, msg)
    if code == QHIP_EXEC_ERROR or msg.startswith("Arrow error") or msg.startswith("Invalid argument error"):
        raise ArrowError(code, msg)
    raise InternalError(code, msg)


class qhip_dtype(C.Structure):
    _fields_ = [("id", C.c_int32), ("precision", C.c_int32), ("scale", C.c_int32)]


class qhip_expr(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("op", C.c_int32), ("column", C.c_int32), ("left", C.c_int32), ("right", C.c_int32),
        ("third", C.c_int32), ("dtype", qhip_dtype), ("lit_is_null", C.c_int32),
        ("lit_lo", C.c_uint64), ("lit_hi", C.c_int64), ("lit_f64", C.c_double),
        ("lit_str", C.c_char_p), ("lit_len", C.c_int64),
    ]


class qhip_agg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("expr", C.c_int32), ("return_type", qhip_dtype)]


class qhip_exec_stats(C.Structure):
    _fields_ = [
        ("main_kernel_ms", C.c_double), ("total_device_ms", C.c_double), ("jit_ms", C.c_double),
        ("rows_in", C.c_int64), ("rows_out", C.c_int64), ("groups", C.c_int64), ("table_capacity", C.c_int64),
        ("retries", C.c_int32), ("lds_table_slots", C.c_int32), ("main_kernel_name", C.c_char * 64),
        ("lds_occupancy", C.c_double), ("hbm_table_load", C.c_double), ("lds_spilled", C.c_int32), ("workgroups", C.c_int32),
        ("bytes_per_row_read", C.c_double), ("build_ms", C.c_double), ("build_rows", C.c_int64), ("build_bytes_per_row", C.c_double),
    ]


class qhip_csv_options(C.Structure):
    _fields_ = [("has_header", C.c_int32), ("delimiter", C.c_int32), ("quote", C.c_int32), ("escape", C.c_int32)]


class ArrowSchemaStruct(C.Structure):
    pass


class ArrowArrayStruct(C.Structure):
    pass


ArrowSchemaStruct._fields_ = [
    ("format", C.c_char_p), ("name", C.c_char_p), ("metadata", C.c_char_p), ("flags", C.c_int64),
    ("n_children", C.c_int64), ("children", C.POINTER(C.POINTER(ArrowSchemaStruct))),
    ("dictionary", C.POINTER(ArrowSchemaStruct)), ("release", C.c_void_p), ("private_data", C.c_void_p),
]
ArrowArrayStruct._fields_ = [
    ("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64),
    ("n_children", C.c_int64), ("buffers", C.POINTER(C.c_void_p)), ("children", C.POINTER(C.POINTER(ArrowArrayStruct))),
    ("dictionary", C.POINTER(ArrowArrayStruct)), ("release", C.c_void_p), ("private_data", C.c_void_p),
]

_lib = None
_lib_lock = threading.Lock()


def load_library() -> C.CDLL:
    """Load libqhip.so (built in-tree by ``__graft_entry__.build()`` / ``make -C qurious_amd/csrc``)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the HIP backend has no Python/CPU fallback)")
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        P = C.POINTER
        sigs = {
            "qhip_ctx_create": (C.c_int, [C.c_int, P(vp)]),
            "qhip_ctx_destroy": (None, [vp]),
            "qhip_last_error": (C.c_char_p, [vp]),
            "qhip_version": (C.c_char_p, []),
            "qhip_device_available": (C.c_int, []),
            "qhip_ctx_last_stats": (C.c_int, [vp, P(qhip_exec_stats)]),
            "qhip_ctx_synchronize": (C.c_int, [vp]),
            "qhip_ctx_sync_count": (C.c_uint64, [vp]),
            "qhip_ctx_set_timing": (C.c_int, [vp, i32]),
            "qhip_ctx_set_wide_group_keys": (C.c_int, [vp, i32]),
            "qhip_ctx_wide_key_aggregates": (i64, [vp]),
            "qhip_ctx_set_wide_join_keys": (C.c_int, [vp, i32]),
            "qhip_ctx_set_csv_grammar": (C.c_int, [vp, i32]),
            "qhip_ctx_set_float_parse": (C.c_int, [vp, i32]),
            "qhip_ctx_wide_key_joins": (i64, [vp]),
            "qhip_ctx_allow_deferred_sizes": (C.c_int, [vp, i32]),
            "qhip_ctx_forget_plans": (C.c_int, [vp]),
            "qhip_ctx_device_name": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
            "qhip_table_from_arrow": (C.c_int, [vp, vp, P(vp), i64, P(vp)]),
            "qhip_table_from_arrow_lazy": (C.c_int, [vp, vp, P(vp), i64, P(vp)]),
            "qhip_table_from_csv": (C.c_int, [vp, vp, vp, i64, P(qhip_csv_options), P(i32), i32, i64, P(vp)]),
            "qhip_ctx_csv_pass_ms": (C.c_int, [vp, P(C.c_double), i32]),
            "qhip_table_from_json": (C.c_int, [vp, vp, vp, i64, P(i32), i32, i64, P(vp)]),
            "qhip_ctx_json_pass_ms": (C.c_int, [vp, P(C.c_double), i32]),
            "qhip_table_from_parquet": (C.c_int, [vp, vp, vp, i64, P(i32), i32, i64, P(vp)]),
            "qhip_ctx_parquet_pass_ms": (C.c_int, [vp, P(C.c_double), i32]),
            "qhip_ctx_parquet_unpack_ms": (C.c_int, [vp, P(C.c_double)]),
            "qhip_ctx_set_parquet_format": (C.c_int, [vp, i32]),
            "qhip_snappy_decode": (C.c_int, [vp, vp, i64, P(i64), P(i64), i64, vp, i64, P(i32)]),
            "qhip_ctx_set_parquet_encodings": (C.c_int, [vp, i32]),
            "qhip_ctx_set_parquet_codecs": (C.c_int, [vp, i32]),
            "qhip_zstd_decode": (C.c_int, [vp, vp, i64, P(i64), P(i64), i64, vp, i64, P(i32)]),
            "qhip_ctx_set_parquet_gzip": (C.c_int, [vp, i32]),
            "qhip_gzip_decode": (C.c_int, [vp, vp, i64, P(i64), P(i64), i64, vp, i64, P(i32)]),
            "qhip_ctx_set_parquet_lz4": (C.c_int, [vp, i32]),
            "qhip_lz4_decode": (C.c_int, [vp, vp, i64, P(i64), P(i64), i64, vp, i64, P(i32)]),
            "qhip_ctx_set_parquet_delta_byte_array": (C.c_int, [vp, i32]),
            "qhip_ctx_parquet_fill_ms": (C.c_int, [vp, P(C.c_double)]),
            "qhip_parquet_dba_decode": (C.c_int, [vp, vp, i64, P(i64), P(i32), P(i64), i64, vp, i64, P(i64), P(i64), P(i32)]),
            "qhip_ctx_parquet_delta_ms": (C.c_int, [vp, P(C.c_double)]),
            "qhip_parquet_delta_decode": (C.c_int, [vp, vp, i64, P(i64), P(i32), P(i64), i64, vp, i64, P(i64), P(i32)]),
            "qhip_table_to_arrow": (C.c_int, [vp, vp, i64, vp, vp]),
            "qhip_table_num_batches": (i64, [vp]),
            "qhip_table_batch_offsets": (C.c_int, [vp, P(i64), i64]),
            "qhip_table_num_rows": (i64, [vp]),
            "qhip_table_num_columns": (i64, [vp]),
            "qhip_table_column_bytes": (i64, [vp, i64]),
            "qhip_table_destroy": (None, [vp]),
            "qhip_filter_execute": (C.c_int, [vp, vp, P(qhip_expr), i32, i32, P(i32), i32, P(vp)]),
            "qhip_hash_aggregate_execute": (C.c_int, [vp, vp, P(qhip_expr), i32, i32, P(i32), i32, P(qhip_agg), i32,
                                                      P(C.c_char_p), P(vp)]),
            "qhip_hash_join_execute": (C.c_int, [vp, vp, vp, i32, P(qhip_expr), i32, P(qhip_expr), i32, P(i32), P(i32), i32,
                                                 P(qhip_expr), i32, i32, P(i32), P(i32), i32, i32, i32, P(vp)]),
            "qhip_nested_loop_join_execute": (C.c_int, [vp, vp, vp, i32, P(qhip_expr), i32, i32, P(i32), P(i32), i32, P(vp)]),
            "qhip_cross_join_execute": (C.c_int, [vp, vp, vp, P(vp)]),
            "qhip_projection_execute": (C.c_int, [vp, vp, P(qhip_expr), i32, P(i32), i32, P(C.c_char_p), P(vp)]),
            "qhip_sort_execute": (C.c_int, [vp, vp, P(qhip_expr), i32, P(i32), P(i32), P(i32), i32, i64, P(vp)]),
            "qhip_limit_execute": (C.c_int, [vp, vp, i64, i64, P(vp)]),
            "qhip_partition_by_key": (C.c_int, [vp, vp, P(qhip_expr), i32, P(i32), i32, i32, P(vp)]),
            "qhip_partition_filtered": (C.c_int, [vp, vp, P(qhip_expr), i32, P(i32), i32, i32, P(i32), i32, P(vp)]),
            "qhip_table_forget_statistics": (C.c_int, [vp]),
            "qhip_table_aux_bytes": (i64, [vp]),
            "qhip_table_concat": (C.c_int, [vp, P(vp), i32, P(vp)]),
            "qhip_table_column_buffer": (C.c_int, [vp, i64, i32, P(vp), P(i64)]),
            "qhip_table_wire_meta": (C.c_int, [vp, vp, P(i64), i32]),
            "qhip_table_keep_columns": (C.c_int, [vp, vp, P(i32), i32, P(vp)]),
            "qhip_table_pack": (C.c_int, [vp, vp, vp, i64]),
            "qhip_table_unpack_concat": (C.c_int, [vp, P(C.c_char_p), P(qhip_dtype), i32, P(i64), P(vp), i32, P(vp)]),
            "qhip_jit_compile_to_cache": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
        }
        for name, (res, args) in sigs.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


BENCH_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libqhip_bench.so")
_BENCH_LIB = None


def load_bench_library():
    """libqhip_bench.so (include/qhip_bench.h): the synthetic TPC-H-shaped table generators and the streaming-read yardstick —
    benchmark support, kept out of the product library"""
    global _BENCH_LIB
    if _BENCH_LIB is None:
        if not os.path.exists(BENCH_LIB_PATH):
            raise ImportError(f"{BENCH_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(BENCH_LIB_PATH)
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        for name, (res, args) in {
            "qhip_synth_lineitem": (C.c_int, [i64, i64] + [vp] * 9),
            "qhip_synth_customer": (C.c_int, [i64, i64, vp, vp, vp]),
            "qhip_synth_orders": (C.c_int, [i64, i64, i64, vp, vp, vp, vp]),
            "qhip_synth_q3_lineitem_count": (i64, [i64, i64]),
            "qhip_synth_q3_lineitem": (C.c_int, [i64, i64, vp, vp, vp, vp]),
            "qhip_bench_stream_read": (C.c_int, [i32, i64, i32, C.POINTER(C.c_double)]),
        }.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _BENCH_LIB = lib
    return _BENCH_LIB


class Context:
    """Owner of one qhip_ctx (one HIP device, one stream). One per process and device is enough."""

    def __init__(self, device: int = -1):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.qhip_ctx_create(device, C.byref(h))
        if rc != QHIP_OK:
            _raise(rc, self.lib.qhip_last_error(None).decode())
        self.handle = h

    def check(self, rc: int):
        if rc != QHIP_OK:
            _raise(rc, self.lib.qhip_last_error(self.handle).decode())

    def last_stats(self) -> dict:
        st = qhip_exec_stats()
        self.check(self.lib.qhip_ctx_last_stats(self.handle, C.byref(st)))
        d = {f[0]: getattr(st, f[0]) for f in qhip_exec_stats._fields_}
        d["main_kernel_name"] = st.main_kernel_name.decode()
        return d

    def synchronize(self):
        self.check(self.lib.qhip_ctx_synchronize(self.handle))

    def set_timing(self, on: bool):
        """qhip_exec_stats timings (HIP events around an operator's phases) on / off; off by default, they cost stream time."""
        self.check(self.lib.qhip_ctx_set_timing(self.handle, 1 if on else 0))

    def set_wide_group_keys(self, mode: int):
        """GROUP BY keys wider than the packed 8 key words (long Utf8 values, many columns) are first encoded to one group code
        per row: 0 off, 1 when the key does not fit, 2 every grouped aggregate over plain key columns. Never set: the
        environment's QHIP_AGG_WIDE_KEYS decides per call (default 0)."""
        self.check(self.lib.qhip_ctx_set_wide_group_keys(self.handle, int(mode)))

    def wide_key_aggregates(self) -> int:
        """Aggregate calls of this context that went through the wide-key encoding stage so far."""
        return int(self.lib.qhip_ctx_wide_key_aggregates(self.handle))

    def set_wide_join_keys(self, mode: int):
        """Hash join keys wider than the packed 8 key words (long Utf8 values, many columns) are first encoded to one shared key
        code per row of either side: 0 off, 1 when the key does not fit, 2 every hash join over plain key columns. Never set: the
        environment's QHIP_JOIN_WIDE_KEYS decides per call (default 0)."""
        self.check(self.lib.qhip_ctx_set_wide_join_keys(self.handle, int(mode)))

    def wide_key_joins(self) -> int:
        """Hash join calls of this context that went through the wide-key encoding stage so far."""
        return int(self.lib.qhip_ctx_wide_key_joins(self.handle))

    def set_csv_grammar(self, level: int):
        """The device CSV decoder's grammar: 1 (the default) plain fields only, any quote byte needs the host; 2 also canonical
        quoted fields, Boolean and Timestamp columns. QHIP_CSV_GRAMMAR sets it when the context is made."""
        self.check(self.lib.qhip_ctx_set_csv_grammar(self.handle, int(level)))

    def set_float_parse(self, level: int):
        """What the device CSV and JSON decoders parse in a float column: 1 (the default) Float64 spellings in Clinger's exact
        range only (a 17-digit value needs the host), Float32 columns refused; 2 every spelling of the strict grammar, correctly
        rounded on the device, and Float32 columns. QHIP_FLOAT_PARSE sets it when the context is made."""
        self.check(self.lib.qhip_ctx_set_float_parse(self.handle, int(level)))

    def csv_pass_ms(self) -> List[float]:
        """Device time (ms) of the last device CSV decode's passes: upload, scan, record starts, decode, Utf8 (timing on)."""
        out = (C.c_double * 5)()
        self.check(self.lib.qhip_ctx_csv_pass_ms(self.handle, out, 5))
        return list(out)

    def json_pass_ms(self) -> List[float]:
        """Device time (ms) of the last device JSON decode's passes: upload, scan, record starts, decode, Utf8 (timing on)."""
        out = (C.c_double * 5)()
        self.check(self.lib.qhip_ctx_json_pass_ms(self.handle, out, 5))
        return list(out)

    def parquet_pass_ms(self) -> List[float]:
        """Device time (ms) of the last device Parquet decode's passes: upload, levels, string walk, values, Utf8 (timing on)."""
        out = (C.c_double * 5)()
        self.check(self.lib.qhip_ctx_parquet_pass_ms(self.handle, out, 5))
        return list(out)

    def parquet_unpack_ms(self) -> float:
        """Device time (ms) of the unpack pass (Snappy pages, format level 2) of the last device Parquet decode, or of the last
        `snappy_decode`'s kernel (timing on). It lies between "upload" and "levels" and is part of neither."""
        out = C.c_double(0)
        self.check(self.lib.qhip_ctx_parquet_unpack_ms(self.handle, C.byref(out)))
        return float(out.value)

    def set_parquet_format(self, level: int):
        """The device Parquet decoder's format level: 1 (the default) uncompressed chunks only, a compressed file needs the host;
        2 also SNAPPY chunks — pyarrow's default — unpacked on the device. QHIP_PARQUET_FORMAT sets it when the context is made."""
        self.check(self.lib.qhip_ctx_set_parquet_format(self.handle, int(level)))

    def set_parquet_encodings(self, encodings: int):
        """The device Parquet decoder's encoding set, independent of the format level: 1 (the default) data pages V1 with PLAIN
        or dictionary values; 2 also data pages V2, RLE Boolean values, BYTE_STREAM_SPLIT, DELTA_BINARY_PACKED and
        DELTA_LENGTH_BYTE_ARRAY. QHIP_PARQUET_ENCODINGS sets it when the context is made."""
        self.check(self.lib.qhip_ctx_set_parquet_encodings(self.handle, int(encodings)))

    def set_parquet_codecs(self, codecs: int):
        """The device Parquet decoder's codec set, independent of the format level and the encoding set: 1 (the default) the
        codecs the format level admits; 2 also ZSTD chunks, each page a Zstandard frame decoded by a kernel of its own (the
        content checksum is not verified). SNAPPY stays with the format level. QHIP_PARQUET_CODECS sets it when the context is
        made."""
        self.check(self.lib.qhip_ctx_set_parquet_codecs(self.handle, int(codecs)))

    def set_parquet_gzip(self, on: int):
        """The device Parquet decoder's gzip switch, independent of the format level, the encoding set and the codec set: 0 (the
        default) a GZIP chunk takes the host path; 1 GZIP chunks are unpacked on the device, each page a gzip member inflated
        by a kernel of its own (the CRC32 is not verified). Brotli and zlib-wrapped pages stay on the host; LZ4 has a switch of
        its own. QHIP_PARQUET_GZIP sets it when the context is made."""
        self.check(self.lib.qhip_ctx_set_parquet_gzip(self.handle, int(on)))

    def set_parquet_lz4(self, on: int):
        """The device Parquet decoder's lz4 switch, independent of the format level, the encoding set, the codec set and the gzip
        switch: 0 (the default) an LZ4 chunk takes the host path; 1 LZ4_RAW chunks (what `compression="lz4"` writes) and chunks
        of the legacy LZ4 id (Hadoop's length frames where they tile the page, one bare block otherwise) are unpacked on the
        device, one wavefront per block. QHIP_PARQUET_LZ4 sets it when the context is made."""
        self.check(self.lib.qhip_ctx_set_parquet_lz4(self.handle, int(on)))

    def set_parquet_delta_byte_array(self, on: int):
        """The device Parquet decoder's DELTA_BYTE_ARRAY switch, independent of the format level, the encoding set, the codec set,
        the gzip switch and the lz4 switch: 0 (the default) a DELTA_BYTE_ARRAY page takes the host path; 1 such pages of Utf8
        columns and of FIXED_LEN_BYTE_ARRAY decimals are decoded on the device, the two length streams by k_pq_delta_dba and the
        prefixes by k_pq_dba_fill, 64 rows per step. A page whose first prefix is not 0 stays on the host. QHIP_PARQUET_DBA
        sets it when the context is made."""
        self.check(self.lib.qhip_ctx_set_parquet_delta_byte_array(self.handle, int(on)))

    def parquet_fill_ms(self) -> float:
        """Device time (ms) of the fill passes (k_pq_dba_fill, the DELTA_BYTE_ARRAY switch) of the last device Parquet decode, or
        of the last `dba_decode`'s fill kernel (timing on). It is part of none of `parquet_pass_ms`'s five values."""
        out = C.c_double(0)
        self.check(self.lib.qhip_ctx_parquet_fill_ms(self.handle, C.byref(out)))
        return float(out.value)

    def dba_decode(self, streams: Sequence[bytes], widths: Sequence[int], counts: Sequence[int]):
        """A testing and measurement aid (qhip_parquet_dba_decode): raw DELTA_BYTE_ARRAY value streams through the kernels of the
        DELTA_BYTE_ARRAY switch, in one call. `widths[k]`: the FIXED_LEN_BYTE_ARRAY width of stream k's values, 0 for
        BYTE_ARRAY; `counts[k]`: the values expected. Returns (values, statuses): statuses[k] is 0 or the needs-host reason for
        which stream k was refused, values[k] its values as a list of bytes (None when refused)."""
        n = len(streams)
        blob = b"".join(streams)
        offs = (C.c_int64 * (n + 1))()
        at = 0
        for k, s in enumerate(streams):
            offs[k] = at
            at += len(s)
        offs[n] = at
        w = (C.c_int32 * max(n, 1))(*[int(v) for v in widths])
        c = (C.c_int64 * max(n, 1))(*[int(v) for v in counts])
        nvo = sum(int(v) + 1 for v in counts)
        vo = (C.c_int64 * max(nvo, 1))()
        status = (C.c_int32 * max(n, 1))()
        total = C.c_int64(0)
        room = max(1 << 16, 8 * len(blob))
        while True:
            out = C.create_string_buffer(room)
            self.check(self.lib.qhip_parquet_dba_decode(self.handle, blob, len(blob), offs, w, c, n, out, room, vo, C.byref(total), status))
            if total.value <= room:
                break
            room = int(total.value)
        raw = out.raw
        values, at = [], 0
        for k in range(n):
            cnt = int(counts[k])
            values.append(None if status[k] else [raw[vo[at + i]:vo[at + i + 1]] for i in range(cnt)])
            at += cnt + 1
        return values, [int(status[k]) for k in range(n)]

    def parquet_delta_ms(self) -> float:
        """Device time (ms) of the delta pass (k_pq_delta, encoding set 2) of the last device Parquet decode, or of the last
        `delta_decode`'s kernel (timing on). It lies between "levels" and "string walk" and is part of neither."""
        out = C.c_double(0)
        self.check(self.lib.qhip_ctx_parquet_delta_ms(self.handle, C.byref(out)))
        return float(out.value)

    def delta_decode(self, streams: Sequence[bytes], widths: Sequence[int], counts: Sequence[int]):
        """A testing and measurement aid (qhip_parquet_delta_decode): raw DELTA_BINARY_PACKED streams through the device decoder
        of encoding set 2, one wavefront each, in one call. `widths[k]`: 4 or 8; `counts[k]`: the values expected of stream k.
        Returns (values, ends, statuses): statuses[k] is 0 or the needs-host reason (QH_PQ_R_DELTA_*) for which stream k was
        refused, values[k] its values as unsigned integers of its width (None when refused), ends[k] the byte position where
        the stream ended."""
        n = len(streams)
        data = b"".join(streams)
        off = (C.c_int64 * (n + 1))()
        for k, s in enumerate(streams):
            off[k + 1] = off[k] + len(s)
        wd = (C.c_int32 * max(n, 1))(*[int(v) for v in widths])
        cnt = (C.c_int64 * max(n, 1))(*[int(v) for v in counts])
        total = sum(int(c) * int(w) for c, w in zip(counts, widths))
        out = C.create_string_buffer(max(total, 1))
        ends = (C.c_int64 * max(n, 1))()
        status = (C.c_int32 * max(n, 1))()
        self.check(self.lib.qhip_parquet_delta_decode(self.handle, data, len(data), off, wd, cnt, n, out, total, ends, status))
        values, at, raw = [], 0, out.raw
        for k in range(n):
            nb = int(counts[k]) * int(widths[k])
            if status[k] == 0:
                w = int(widths[k])
                values.append([int.from_bytes(raw[at + i:at + i + w], "little") for i in range(0, nb, w)])
            else:
                values.append(None)
            at += nb
        return values, [int(ends[k]) for k in range(n)], [int(status[k]) for k in range(n)]

    def zstd_decode(self, streams: Sequence[bytes], dst_sizes: Sequence[int]):
        """A testing and measurement aid (qhip_zstd_decode): raw Zstandard frames through the device decoder of codec set 2, one
        wavefront each, in one call. `dst_sizes[k]`: the uncompressed size declared for frame k. Returns (outputs, statuses):
        statuses[k] is 0 or the needs-host reason (QH_PQ_R_ZSTD_*) for which frame k was refused, outputs[k] its bytes (None
        when refused)."""
        return self._unpack_decode(self.lib.qhip_zstd_decode, streams, dst_sizes)

    def gzip_decode(self, streams: Sequence[bytes], dst_sizes: Sequence[int]):
        """A testing and measurement aid (qhip_gzip_decode): raw gzip members through the device DEFLATE decoder of the gzip
        switch, one wavefront each, in one call. `dst_sizes[k]`: the uncompressed size declared for member k. Returns (outputs,
        statuses): statuses[k] is 0 or the needs-host reason (QH_PQ_R_GZIP_*) for which member k was refused, outputs[k] its
        bytes (None when refused)."""
        return self._unpack_decode(self.lib.qhip_gzip_decode, streams, dst_sizes)

    def lz4_decode(self, streams: Sequence[bytes], dst_sizes: Sequence[int]):
        """A testing and measurement aid (qhip_lz4_decode): bare LZ4 blocks through the device decoder of the lz4 switch, one
        wavefront each, in one call. `dst_sizes[k]`: the uncompressed size declared for block k. Returns (outputs, statuses):
        statuses[k] is 0 or the needs-host reason (QH_PQ_R_LZ4_*) for which block k was refused, outputs[k] its bytes (None
        when refused)."""
        return self._unpack_decode(self.lib.qhip_lz4_decode, streams, dst_sizes)

    def snappy_decode(self, streams: Sequence[bytes], dst_sizes: Sequence[int]):
        """A testing and measurement aid (qhip_snappy_decode): raw Snappy streams through the device decoder of format level 2,
        one wavefront each, in one call. `dst_sizes[k]`: the uncompressed size declared for stream k. Returns (outputs, statuses):
        statuses[k] is 0 or the needs-host reason (QH_PQ_R_SNAPPY_*) for which stream k was refused, outputs[k] its bytes
        (None when refused)."""
        return self._unpack_decode(self.lib.qhip_snappy_decode, streams, dst_sizes)

    def _unpack_decode(self, entry, streams: Sequence[bytes], dst_sizes: Sequence[int]):
        n = len(streams)
        data = b"".join(streams)
        off = (C.c_int64 * (n + 1))()
        for k, s in enumerate(streams):
            off[k + 1] = off[k] + len(s)
        dst = (C.c_int64 * max(n, 1))(*[int(v) for v in dst_sizes])
        total = sum(int(v) for v in dst_sizes if 0 <= int(v) <= 0x7FFFFFFF)
        out = C.create_string_buffer(max(total, 1))
        status = (C.c_int32 * max(n, 1))()
        self.check(entry(self.handle, data, len(data), off, dst, n, out, total, status))
        outs, at, raw = [], 0, out.raw
        for k in range(n):
            outs.append(raw[at:at + int(dst_sizes[k])] if status[k] == 0 else None)
            at += int(dst_sizes[k])
        return outs, [int(status[k]) for k in range(n)]

    def sync_count(self) -> int:
        """Host waits on the device made through the library so far (the difference around a plan = its round trips)."""
        return int(self.lib.qhip_ctx_sync_count(self.handle))

    def forget_plans(self):
        """Drop everything learnt about executed plans (lowered plans, join sizes, group counts); compiled kernels stay."""
        self.check(self.lib.qhip_ctx_forget_plans(self.handle))

    def allow_deferred_sizes(self, delta: int):
        self._allow_depth = 0 if delta == 0 else max(0, getattr(self, "_allow_depth", 0) + int(delta))
        self.lib.qhip_ctx_allow_deferred_sizes(self.handle, int(delta))

    def no_deferred_sizes(self):
        """Context manager: no hash join below may leave its size on the device. The multi-rank operators run under it: a
        join of deferred size can answer QHIP_RETRY on ONE rank only, whose re-execution of the input would repeat
        collectives the other ranks do not take part in."""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            depth = getattr(self, "_allow_depth", 0)
            if depth:
                self.lib.qhip_ctx_allow_deferred_sizes(self.handle, -depth)
            try:
                yield
            finally:
                if depth:
                    self.lib.qhip_ctx_allow_deferred_sizes(self.handle, depth)
        return _cm()

    def measure_stream_read(self, nbytes: int = 1 << 32, iters: int = 5) -> float:
        """Achieved GB/s of a plain streaming-read kernel over `nbytes` of HBM (the practical bandwidth ceiling): benchmark
        support, libqhip_bench.so (include/qhip_bench.h), not the product library."""
        out = C.c_double(0.0)
        self.synchronize()
        rc = load_bench_library().qhip_bench_stream_read(int(os.environ.get("QHIP_DEVICE", "0")), int(nbytes), int(iters), C.byref(out))
        if rc != 0:
            raise HipError(QHIP_HIP_ERROR, f"qhip_bench_stream_read failed ({rc})")
        return out.value

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self.check(self.lib.qhip_ctx_device_name(self.handle, buf, 256))
        return buf.value.decode()

    def close(self):
        if self.handle:
            self.lib.qhip_ctx_destroy(self.handle)
            self.handle = None


_ctx = None


def get_context() -> Context:
    """Process-wide context on the current HIP device (LOCAL_RANK under torch.distributed launchers)."""
    global _ctx
    if _ctx is None:
        dev = int(os.environ.get("QHIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _ctx = Context(dev)
    return _ctx


class DeviceTable:
    """HBM-resident Vec<RecordBatch> (qhip_table)."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self.handle = handle

    @staticmethod
    def from_batches(ctx: Context, schema: pa.Schema, batches, lazy: bool = False) -> "DeviceTable":
        """Upload now (default) or, with lazy=True, hand the batches over and let every column move to HBM the first time
        an operator or an export reads it (qhip_table_from_arrow_lazy)."""
        lib = ctx.lib
        c_schema = ArrowSchemaStruct()
        schema._export_to_c(C.addressof(c_schema))
        arrays = [ArrowArrayStruct() for _ in batches]
        try:
            for b, a in zip(batches, arrays):
                if b.schema != schema:
                    b = pa.RecordBatch.from_arrays(b.columns, schema=schema)
                b._export_to_c(C.addressof(a))
            ptrs = (C.c_void_p * max(1, len(arrays)))(*[C.addressof(a) for a in arrays])
            out = C.c_void_p()
            fn = lib.qhip_table_from_arrow_lazy if lazy else lib.qhip_table_from_arrow
            ctx.check(fn(ctx.handle, C.addressof(c_schema), ptrs, len(arrays), C.byref(out)))
            return DeviceTable(ctx, out)
        finally:
            _release_schema(c_schema)
            for a in arrays:
                _release_array(a)

    @staticmethod
    def from_csv_bytes(ctx: Context, schema: pa.Schema, data, has_header: bool = True, delimiter: str = ",", quote: Optional[str] = '"',
                       escape: Optional[str] = None, columns: Optional[Sequence[int]] = None, batch_rows: Optional[int] = None) -> "DeviceTable":
        """Decode a CSV file's bytes on the device (qhip_table_from_csv). `schema` names every field of a record; `columns` are
        the field indices to decode, in output order (None = all). `data`: bytes, or anything with the buffer protocol (an
        mmap). Raises UnsupportedError when the file lies outside the device's grammar — the caller then parses on the host."""
        buf = pa.py_buffer(data)   # (zero copy, read-only buffers too; alive until the call returns)
        n, addr = buf.size, (C.c_void_p(buf.address) if buf.size else None)
        opt = qhip_csv_options(1 if has_header else 0, ord(delimiter), ord(quote) if quote else -1, ord(escape) if escape else -1)
        cols = (C.c_int32 * max(1, len(columns or [])))(*[int(c) for c in (columns or [])])
        c_schema = ArrowSchemaStruct()
        schema._export_to_c(C.addressof(c_schema))
        try:
            out = C.c_void_p()
            ctx.check(ctx.lib.qhip_table_from_csv(ctx.handle, C.addressof(c_schema), addr, n, C.byref(opt), cols if columns else None,
                                                  len(columns or []), int(batch_rows or 0), C.byref(out)))
            return DeviceTable(ctx, out)
        finally:
            _release_schema(c_schema)

    @staticmethod
    def from_json_bytes(ctx: Context, schema: pa.Schema, data, columns: Optional[Sequence[int]] = None, batch_rows: Optional[int] = None) -> "DeviceTable":
        """Decode the bytes of a newline-delimited JSON file on the device (qhip_table_from_json). `schema` names every key a
        record may hold; `columns` are the field indices to decode, in output order (None = all). `data`: bytes, or anything with
        the buffer protocol (an mmap). Raises UnsupportedError, naming the reason and the record, when the file lies outside the
        device's grammar — the caller then parses on the host."""
        buf = pa.py_buffer(data)   # (zero copy, read-only buffers too; alive until the call returns)
        n, addr = buf.size, (C.c_void_p(buf.address) if buf.size else None)
        cols = (C.c_int32 * max(1, len(columns or [])))(*[int(c) for c in (columns or [])])
        c_schema = ArrowSchemaStruct()
        schema._export_to_c(C.addressof(c_schema))
        try:
            out = C.c_void_p()
            ctx.check(ctx.lib.qhip_table_from_json(ctx.handle, C.addressof(c_schema), addr, n, cols if columns else None, len(columns or []),
                                                   int(batch_rows or 0), C.byref(out)))
            return DeviceTable(ctx, out)
        finally:
            _release_schema(c_schema)

    @staticmethod
    def from_parquet_bytes(ctx: Context, schema: pa.Schema, data, columns: Optional[Sequence[int]] = None, batch_rows: Optional[int] = None) -> "DeviceTable":
        """Decode a Parquet file's bytes on the device (qhip_table_from_parquet). `schema`: the Arrow type of every field of the
        file, in file order (`pq.read_schema`); `columns`: the field indices to decode, in output order (None = all). `data`:
        bytes, or anything with the buffer protocol (an mmap). Raises UnsupportedError, naming the reason, when the file lies
        outside what the device decodes — the caller then reads it on the host."""
        buf = pa.py_buffer(data)   # (zero copy, read-only buffers too; alive until the call returns)
        n, addr = buf.size, (C.c_void_p(buf.address) if buf.size else None)
        cols = (C.c_int32 * max(1, len(columns or [])))(*[int(c) for c in (columns or [])])
        c_schema = ArrowSchemaStruct()
        schema._export_to_c(C.addressof(c_schema))
        try:
            out = C.c_void_p()
            ctx.check(ctx.lib.qhip_table_from_parquet(ctx.handle, C.addressof(c_schema), addr, n, cols if columns else None, len(columns or []),
                                                      int(batch_rows or 0), C.byref(out)))
            return DeviceTable(ctx, out)
        finally:
            _release_schema(c_schema)

    def forget_statistics(self):
        """drop the column statistics and narrow copies libqhip has collected on this table (qhip_table_forget_statistics)"""
        self.ctx.check(self.ctx.lib.qhip_table_forget_statistics(self.handle))

    @property
    def aux_bytes(self) -> int:
        return int(self.ctx.lib.qhip_table_aux_bytes(self.handle))

    @property
    def num_rows(self) -> int:
        return self.ctx.lib.qhip_table_num_rows(self.handle)

    @property
    def num_batches(self) -> int:
        return self.ctx.lib.qhip_table_num_batches(self.handle)

    @property
    def num_columns(self) -> int:
        return self.ctx.lib.qhip_table_num_columns(self.handle)

    def column_bytes(self, col: int) -> int:
        return self.ctx.lib.qhip_table_column_bytes(self.handle, col)

    def batch_offsets(self) -> List[int]:
        n = self.num_batches + 1
        out = (C.c_int64 * n)()
        self.ctx.check(self.ctx.lib.qhip_table_batch_offsets(self.handle, out, n))
        return list(out)

    def to_batches(self):
        nb = self.num_batches
        if nb > 8:
            # many batches: ONE download of every row, sliced on the host (zero-copy) at the batch boundaries
            a, s = ArrowArrayStruct(), ArrowSchemaStruct()
            self.ctx.check(self.ctx.lib.qhip_table_to_arrow(self.ctx.handle, self.handle, -1, C.addressof(a), C.addressof(s)))
            whole = pa.RecordBatch._import_from_c(C.addressof(a), C.addressof(s))
            off = self.batch_offsets()
            return [whole.slice(off[b], off[b + 1] - off[b]) for b in range(nb)]
        out = []
        for b in range(nb):
            a = ArrowArrayStruct()
            s = ArrowSchemaStruct()
            self.ctx.check(self.ctx.lib.qhip_table_to_arrow(self.ctx.handle, self.handle, b, C.addressof(a), C.addressof(s)))
            out.append(pa.RecordBatch._import_from_c(C.addressof(a), C.addressof(s)))
        return out

    def schema(self) -> pa.Schema:
        s = ArrowSchemaStruct()
        self.ctx.check(self.ctx.lib.qhip_table_to_arrow(self.ctx.handle, self.handle, 0, None, C.addressof(s)))
        return pa.Schema._import_from_c(C.addressof(s))

    def close(self):
        if self.handle:
            self.ctx.lib.qhip_table_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_RELEASE_FN = C.CFUNCTYPE(None, C.c_void_p)


def _release_schema(s: ArrowSchemaStruct):
    if s.release:
        _RELEASE_FN(s.release)(C.addressof(s))


def _release_array(a: ArrowArrayStruct):
    if a.release:
        _RELEASE_FN(a.release)(C.addressof(a))
