#!/usr/bin/env python3
"""The code generator's identity corpus: a named list of plans whose generated kernel source (or planning error) is
pinned byte for byte by tests/golden/codegen_digests.json (tests/test_codegen_identity_cpu.py).

The generated text IS the kernel: csrc/jit.cpp keys the compiled code object by a hash of it, so equal text means equal
kernels, equal kernel-cache file names and equal device behaviour. A change that only moves host code around
(csrc/codegen.cpp, exprgen.cpp, agg_shape.cpp) must leave every digest as it is. Needs no GPU: every plan goes through
the plan-only entry points of qurious_amd.planning.

    python tools/codegen_corpus.py --digests          # {name: [sha256, length]} as JSON
    python tools/codegen_corpus.py --dump DIR         # one text file per entry, to diff a mismatch

The corpus is the kernel catalog (catalog.catalog_sources()), a matrix over the branches of the generator the catalog
does not reach, one entry per environment switch the generator reads (at a non-default value), and plans that fail —
among them plans with two errors, to pin which one is reported. Every entry runs with all QHIP_* variables removed from
the environment except its own.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pyarrow as pa  # noqa: E402

from qurious_amd import _ffi, catalog, planning  # noqa: E402
from qurious_amd import expr as E  # noqa: E402
from qurious_amd.datatypes import Operator as Op, ScalarValue as SV  # noqa: E402
from qurious_amd.functions import DatetimeExtract  # noqa: E402

DEC = pa.decimal128(15, 2)
INTS = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64()]
NUMERIC = INTS + [pa.float32(), pa.float64(), pa.date32(), pa.date64(), DEC]


def schema(*types):
    return pa.schema([pa.field(f"c{k}", t) for k, t in enumerate(types)])


def col(k):
    return E.Column(f"c{k}", k)


def lit(v):
    return E.Literal(v)


def b(l, op, r):
    return E.BinaryExpr(l, op, r)


class RawIndex(E.PhysicalExpr):
    """Lowers to a fixed node index: roots and aggregate arguments outside the expression array."""

    def __init__(self, index):
        self.index = index

    def _lower(self, out):
        return self.index


class RawAgg(E.AggregateExpr):
    def __init__(self, kind, expr, return_type):
        self.kind, self.expr, self.return_type = kind, expr, return_type


def tname(t):
    return re.sub(r"[^A-Za-z0-9]+", "_", str(t)).strip("_")


def entries():
    """[(name, {env}, callable returning the source)]"""
    out = []

    def add(name, fn, **env):
        out.append((name, {k: str(v) for k, v in env.items()}, fn))

    P = planning
    i64, f64, f32, u8, u64, i32, boo, utf, d32 = pa.int64(), pa.float64(), pa.float32(), pa.uint8(), pa.uint64(), pa.int32(), pa.bool_(), pa.string(), pa.date32()
    gt0 = b(col(0), Op.Gt, lit(SV.Int64(0)))

    # ---------------------------------------------------------------- column loads
    # every storage class, nullable and not, in the plain form (projection: absolute row) and the tile-relative raw form (mask)
    loads = schema(i64, DEC, boo, utf, f32, u8, pa.null(), i32)
    for nulls in (False, True):
        hn = [nulls] * len(loads)
        tag = ", nullable" if nulls else ""
        pred = b(b(b(col(0), Op.Gt, lit(SV.Int64(1))), Op.And, b(col(1), Op.Lt, lit(SV.Decimal128(500, 15, 2)))), Op.And,
                 b(b(col(2), Op.Eq, lit(SV.Boolean(True))), Op.Or, b(col(3), Op.NotEq, lit(SV.Utf8("abc")))))
        pred = b(pred, Op.And, b(b(col(4), Op.LtEq, lit(SV.Float32(1.5))), Op.Or, b(col(5), Op.GtEq, lit(SV.UInt8(7)))))
        add("loads: mask kernel" + tag, lambda pred=pred, hn=hn: P.filter_source(loads, pred, hn))
        add("loads: mask kernel, plain loads" + tag, lambda pred=pred, hn=hn: P.filter_source(loads, pred, hn), QHIP_NO_NT=1)
        proj = [b(col(0), Op.Add, lit(SV.Int64(1))), E.Negative(col(1)), b(col(2), Op.And, lit(SV.Boolean(True))), E.IsNull(col(3)), E.Negative(col(4)),
                b(col(5), Op.Mul, lit(SV.UInt8(2))), E.IsNotNull(col(6)), E.CaseExpr([(col(2), col(3))], lit(SV.Utf8("no")))]
        add("loads: projection" + tag, lambda proj=proj, hn=hn: P.projection_source(loads, proj, hn))
        add("loads: projection, plain loads" + tag, lambda proj=proj, hn=hn: P.projection_source(loads, proj, hn), QHIP_NO_NT=1)
    add("loads: Null column compared is refused", lambda: P.filter_source(loads, b(col(6), Op.Eq, col(6))))
    add("loads: one-byte Utf8 by row number, projection", lambda: P.projection_source(loads, [b(col(3), Op.Eq, lit(SV.Utf8("A")))]), QHIP_PLAN_UTF8_FIXED1="3")
    add("loads: one-byte Utf8 by row number, mask", lambda: P.filter_source(loads, b(col(3), Op.Eq, lit(SV.Utf8("A")))), QHIP_PLAN_UTF8_FIXED1="3")
    # narrow copies (4 and 8 bytes) of Decimal128 and Int64 columns, raw and plain; indirect columns and record copies
    narrow = schema(DEC, DEC, i64, i64)
    npred = b(b(col(0), Op.Lt, col(1)), Op.And, b(col(2), Op.Lt, col(3)))
    for nt in (None, 1):
        env = dict(QHIP_PLAN_VALUE_BITS="0:20,1:50", QHIP_PLAN_NARROW_INTS="2")
        if nt:
            env["QHIP_NO_NT"] = 1
        tag = ", plain loads" if nt else ""
        add("narrow copies: mask" + tag, lambda: P.filter_source(narrow, npred), **env)
        add("narrow copies: key words" + tag, lambda: P.keys_source(narrow, [col(2), col(0), col(1)]), **env)
        add("narrow copies: probe" + tag, lambda: P.probe_source(narrow, [col(2), col(3)], npred), **env)
        add("indirect columns: mask" + tag, lambda: P.filter_source(narrow, npred), QHIP_PLAN_INDIRECT=1, **env)
        add("indirect columns from records: mask" + tag, lambda: P.filter_source(narrow, npred), QHIP_PLAN_INDIRECT=1, QHIP_PLAN_RECORDS="0:8,2:16", **env)
        add("indirect columns from records: key words" + tag, lambda: P.keys_source(narrow, [col(2), col(0)]), QHIP_PLAN_INDIRECT=1, QHIP_PLAN_RECORDS="0:8,2:16", **env)

    # ---------------------------------------------------------------- literals
    lits = schema(i64, utf, DEC, f64, f32, boo, d32, u64)
    lit_pred = [b(col(0), Op.Eq, lit(SV.Int64(-5))), b(col(1), Op.Eq, lit(SV.Utf8("BUILDING"))), b(col(2), Op.Eq, lit(SV.Decimal128(-(1 << 70), 15, 2))),
                b(col(3), Op.Eq, lit(SV.Float64(2.5))), b(col(4), Op.Eq, lit(SV.Float32(0.1))), b(col(5), Op.Eq, lit(SV.Boolean(False))),
                b(col(6), Op.Eq, E.CastExpr(lit(SV.Utf8("1995-03-15")), d32)), b(col(7), Op.Eq, lit(SV.UInt64((1 << 64) - 1)))]
    null_pred = [b(col(0), Op.Eq, lit(SV.Int64())), b(col(1), Op.Eq, lit(SV.Utf8())), b(col(2), Op.Eq, lit(SV.Decimal128(None, 15, 2))),
                 b(col(3), Op.Eq, lit(SV.Float64())), b(col(5), Op.Eq, lit(SV.Boolean()))]
    add("literals: every type", lambda: P.projection_source(lits, lit_pred))
    add("literals: typed NULLs", lambda: P.projection_source(lits, null_pred))
    add("literals: Utf8 on the left", lambda: P.filter_source(lits, b(lit(SV.Utf8("x")), Op.Eq, col(1))))
    add("literals: Utf8 both sides", lambda: P.filter_source(lits, b(b(lit(SV.Utf8("x")), Op.Eq, lit(SV.Utf8("a long literal"))), Op.And, gt0)))
    many = gt0
    for k in range(1, 25):
        many = b(many, Op.And, b(col(0), Op.NotEq, lit(SV.Int64(k))))
    add("literals: 25 literals is one too many", lambda: P.filter_source(lits, many))
    like24 = E.Like(False, col(1), lit(SV.Utf8("a%")))
    for k in range(24):
        like24 = b(b(col(0), Op.NotEq, lit(SV.Int64(k))), Op.And, like24)
    add("literals: 24 literals and a LIKE pattern is one too many", lambda: P.filter_source(lits, like24))
    wide = schema(*([i64] * 26))
    wpred = gt0
    for k in range(1, 26):
        wpred = b(wpred, Op.And, b(col(k), Op.Gt, col(0)))
    add("columns: 26 distinct columns is too many", lambda: P.filter_source(wide, wpred))

    # ---------------------------------------------------------------- comparisons and Kleene logic
    cmps = schema(utf, utf, f64, f64, boo, boo, i64, i64, f32, f32)
    for nulls in (False, True):
        hn = [nulls] * len(cmps)
        tag = ", nullable" if nulls else ""
        for op in (Op.Eq, Op.NotEq, Op.Gt, Op.GtEq, Op.Lt, Op.LtEq):
            ex = [b(col(0), op, col(1)), b(col(0), op, lit(SV.Utf8("abc"))), b(lit(SV.Utf8("abcdefghij")), op, col(1)), b(col(2), op, col(3)), b(col(4), op, col(5)),
                  b(col(6), op, col(7)), b(col(8), op, col(9))]
            add(f"compare {op.name}" + tag, lambda ex=ex, hn=hn: P.projection_source(cmps, ex, hn))
        for op in (Op.And, Op.Or):
            add(f"logic {op.name}, mask" + tag, lambda op=op, hn=hn: P.filter_source(cmps, b(b(col(4), op, col(5)), op, b(col(6), Op.Lt, col(7))), hn))
    add("logic: one nullable side", lambda: P.filter_source(cmps, b(b(col(4), Op.Or, col(5)), Op.And, col(5)), [False] * 4 + [True, False] + [False] * 4))
    add("is null / is not null", lambda: P.filter_source(cmps, b(E.IsNull(col(0)), Op.Or, E.IsNotNull(b(col(6), Op.Add, col(7)))), [True] * len(cmps)))
    add("compare: mismatched types", lambda: P.filter_source(cmps, b(col(0), Op.Eq, col(6))))
    add("logic: non-boolean operand", lambda: P.filter_source(cmps, b(col(4), Op.And, col(6))))

    # ---------------------------------------------------------------- arithmetic
    for t in INTS + [f32, f64]:
        s = schema(t, t)
        for nulls in (False, True):
            hn = [nulls, nulls]
            ex = [b(col(0), op, col(1)) for op in (Op.Add, Op.Sub, Op.Mul, Op.Div, Op.Mod)]
            add(f"arithmetic {tname(t)}" + (", nullable" if nulls else ""), lambda s=s, ex=ex, hn=hn: P.projection_source(s, ex, hn))
    add("arithmetic: checked div/rem in a raw-mode kernel", lambda: P.filter_source(schema(i64, i64), b(b(col(0), Op.Div, col(1)), Op.Gt, b(col(0), Op.Mod, col(1))), [True, False]))
    # a fused filter gates the flags of keys and arguments (the predicate's own stay unconditional; what has no fallible node is unchanged)
    fal = schema(i64, i64, f64)
    quot, narrow8 = b(col(0), Op.Div, col(1)), E.CastExpr(col(2), pa.int32())
    for nulls in (False, True):
        hn = [nulls] * len(fal)
        tag = ", nullable" if nulls else ""
        add("fallible argument under a predicate" + tag, lambda hn=hn: P.aggregate_source(fal, b(col(1), Op.NotEq, lit(SV.Int64(0))), [narrow8], [E.SumAggregateExpr(quot, i64)], hn))
        add("fallible argument under a fallible predicate" + tag,
            lambda hn=hn: P.aggregate_source(fal, b(b(col(0), Op.Mod, col(1)), Op.Eq, lit(SV.Int64(0))), [], [E.SumAggregateExpr(quot, i64)], hn))
        add("fallible argument, no predicate" + tag, lambda hn=hn: P.aggregate_source(fal, None, [narrow8], [E.SumAggregateExpr(quot, i64)], hn))
        add("fallible join key under a scan filter: probe" + tag, lambda hn=hn: P.probe_source(fal, [quot, narrow8], gt0, hn))
        add("fallible join key under a scan filter: build entries" + tag, lambda hn=hn: P.scatter_source(fal, [quot, narrow8], gt0, hn))
        add("fallible join key under a scan filter: dense build" + tag, lambda hn=hn: P.scatter_source(fal, [quot], gt0, hn), QHIP_PLAN_DENSE=1)
        add("fallible join key under a scan filter: partition" + tag, lambda hn=hn: P.partition_source(fal, [quot], gt0, 8, hn))
        add("fallible join key, no scan filter: probe" + tag, lambda hn=hn: P.probe_source(fal, [quot, narrow8], None, hn))
    add("arithmetic: Date32 + Date32 is refused", lambda: P.projection_source(schema(d32, d32), [b(col(0), Op.Add, col(1))]))
    add("arithmetic: mixed integer types are refused", lambda: P.projection_source(schema(i64, i32), [b(col(0), Op.Add, col(1))]))
    add("arithmetic: unknown operator", lambda: P.projection_source(schema(i64, i64), [_binary_raw(col(0), 13, col(1))]))
    # Decimal128: the three multiply tiers, the 64-bit and 128-bit sums with either side rescaled, division in Float64
    D1, D2, D3 = pa.decimal128(15, 2), pa.decimal128(12, 4), pa.decimal128(38, 0)
    dec = schema(D1, D2, D3, i64, f64)
    dex = [b(col(0), op, col(1)) for op in (Op.Add, Op.Sub, Op.Mul, Op.Div)] + [b(col(1), Op.Add, col(0)), b(col(0), Op.Div, col(3)), b(col(4), Op.Div, col(1)),
           b(col(3), Op.Div, col(0)), b(b(col(0), Op.Mul, col(1)), Op.Sub, col(2)), b(col(2), Op.Add, col(1))]
    for bits, tag in ((None, "unbounded"), ("0:13,1:24", "below 2^31"), ("0:40,1:20", "below 2^63"), ("0:62,1:62,2:62", "sums above 2^63")):
        env = {"QHIP_PLAN_VALUE_BITS": bits} if bits else {}
        for nulls in (False, True):
            hn = [nulls] * len(dec)
            ntag = ", nullable" if nulls else ""
            add(f"decimal arithmetic, {tag}{ntag}: projection", lambda hn=hn: P.projection_source(dec, dex, hn), **env)
            add(f"decimal arithmetic, {tag}{ntag}: mask", lambda hn=hn: P.filter_source(dec, b(b(col(0), Op.Mul, col(1)), Op.Gt, b(col(1), Op.Mul, col(0))), hn), **env)
    add("decimal arithmetic: remainder is refused", lambda: P.projection_source(dec, [b(col(0), Op.Mod, col(1))]))
    add("decimal arithmetic: decimal + integer is refused", lambda: P.projection_source(dec, [b(col(0), Op.Add, col(3))]))
    add("decimal arithmetic: division by a string is refused", lambda: P.projection_source(schema(D1, utf), [b(col(0), Op.Div, col(1))]))
    add("decimal arithmetic: scale above 38", lambda: P.projection_source(schema(pa.decimal128(38, 20), pa.decimal128(38, 20)), [b(col(0), Op.Mul, col(1))]))
    for t in (i64, f32, f64, DEC, pa.int8()):
        add(f"negative {tname(t)}", lambda t=t: P.projection_source(schema(t), [E.Negative(col(0))], [True]))
        add(f"negative {tname(t)}, not nullable", lambda t=t: P.projection_source(schema(t), [E.Negative(col(0))]))
    add("negative: unsigned is refused", lambda: P.projection_source(schema(u64), [E.Negative(col(0))]))

    # ---------------------------------------------------------------- the cast matrix
    numeric = NUMERIC + [pa.decimal128(20, 6), pa.decimal128(10, 0)]
    cast_types = numeric + [boo, utf, pa.null(), pa.time32("s"), pa.time64("ns"), pa.timestamp("us")]
    for f in cast_types:
        s = schema(f)
        for nulls in (False, True):
            for t in (numeric if nulls else cast_types):   # (one plan per pair: a refused pair fails its whole plan)
                add(f"cast {tname(f)} -> {tname(t)}" + (", nullable" if nulls else ""), lambda s=s, t=t, nulls=nulls: P.projection_source(s, [E.CastExpr(col(0), t)], [nulls]))
    add("cast: in a raw-mode kernel", lambda: P.filter_source(schema(i64, f64), b(E.CastExpr(col(0), pa.int8()), Op.Lt, E.CastExpr(col(1), pa.int8())), [True, False]))
    add("cast: literals fold on the host", lambda: P.projection_source(schema(i64), [b(col(0), Op.Add, E.CastExpr(lit(SV.Utf8("42")), i64)),
                                                                                     b(E.CastExpr(col(0), DEC), Op.Add, E.CastExpr(lit(SV.Float64(1.25)), DEC))]))
    add("cast: literal out of range", lambda: P.projection_source(schema(i64), [b(E.CastExpr(col(0), pa.int8()), Op.Add, E.CastExpr(lit(SV.Int64(300)), pa.int8()))]))

    # ---------------------------------------------------------------- CASE, LIKE, EXTRACT
    cs = schema(boo, i64, i64, utf, utf, DEC)
    for nulls in (False, True):
        hn = [nulls] * len(cs)
        tag = ", nullable" if nulls else ""
        ex = [E.CaseExpr([(col(0), col(1))], col(2)), E.CaseExpr([(col(0), col(3))], col(4)), E.CaseExpr([(col(0), col(3)), (b(col(1), Op.Gt, col(2)), lit(SV.Utf8("big")))], lit(SV.Utf8())),
              E.CaseExpr([(col(0), col(5))], lit(SV.Decimal128(None, 15, 2)))]
        add("case: projection" + tag, lambda ex=ex, hn=hn: P.projection_source(cs, ex, hn))
        add("case: mask" + tag, lambda hn=hn: P.filter_source(cs, b(E.CaseExpr([(col(0), col(3))], col(4)), Op.Eq, lit(SV.Utf8("x"))), hn))
        likes = [E.Like(False, col(3), lit(SV.Utf8("a%_b\\%"))), E.Like(True, col(3), lit(SV.Utf8("%x%"))), E.Like(False, col(3), col(4)), E.Like(True, col(3), col(4)),
                 E.Like(False, col(3), lit(SV.Utf8()))]
        add("like: projection" + tag, lambda likes=likes, hn=hn: P.projection_source(cs, likes, hn))
        for k, lk in enumerate(likes):
            add(f"like {k}: mask" + tag, lambda lk=lk, hn=hn: P.filter_source(cs, lk, hn))
    add("case: WHEN must be Boolean", lambda: P.projection_source(cs, [E.CaseExpr([(col(1), col(1))], col(2))]))
    add("case: branch types differ", lambda: P.projection_source(cs, [E.CaseExpr([(col(0), col(1))], col(3))]))
    add("like: non-string operand", lambda: P.filter_source(cs, E.Like(False, col(1), lit(SV.Utf8("a")))))
    add("like: computed pattern", lambda: P.filter_source(cs, E.Like(False, col(3), E.CaseExpr([(col(0), col(3))], col(4)))))
    ext_types = [d32, pa.date64(), pa.timestamp("s"), pa.timestamp("ms"), pa.timestamp("us"), pa.timestamp("ns")]
    es = schema(*ext_types)
    fx = DatetimeExtract()
    for nulls in (False, True):
        hn = [nulls] * len(es)
        tag = ", nullable" if nulls else ""
        for part in ("year", "MONTH", "day", "hour", "minute", "second", "week"):
            ex = [E.Function(fx, [lit(SV.Utf8(part)), col(k)]) for k in range(len(ext_types))]
            add(f"extract {part.lower()}" + tag, lambda ex=ex, hn=hn: P.projection_source(es, ex, hn))
        add("extract: mask" + tag, lambda hn=hn: P.filter_source(es, b(E.Function(fx, [lit(SV.Utf8("year")), col(0)]), Op.Eq, E.Function(fx, [lit(SV.Utf8("hour")), col(0)])), hn))
    add("extract: of a literal folds on the host", lambda: P.projection_source(es, [b(E.Function(fx, [lit(SV.Utf8("year")), col(0)]), Op.Add,
                                                                                      E.Function(fx, [lit(SV.Utf8("year")), E.CastExpr(lit(SV.Utf8("1995-03-15")), d32)]))]))
    add("extract: unknown part", lambda: P.projection_source(es, [E.Function(fx, [lit(SV.Utf8("epoch")), col(0)])]))
    add("extract: century", lambda: P.projection_source(es, [E.Function(fx, [lit(SV.Utf8("century")), col(0)])]))
    add("extract: part not a literal", lambda: P.projection_source(schema(d32, utf), [E.Function(fx, [col(1), col(0)])]))
    add("extract: NULL part", lambda: P.projection_source(es, [E.Function(fx, [lit(SV.Utf8()), col(0)])]))
    add("extract: from Int64", lambda: P.projection_source(schema(i64), [E.Function(fx, [lit(SV.Utf8("year")), col(0)])]))
    add("extract: one argument", lambda: P.projection_source(es, [E.Function(fx, [col(0)])]))
    add("expression: unknown kind", lambda: P.projection_source(es, [_node_raw(kind=31)]))
    add("expression: column out of range", lambda: P.projection_source(es, [b(col(77), Op.Eq, col(0))]))

    # ---------------------------------------------------------------- packed keys
    key_types = [i64, u8, i32, utf, d32, pa.date64(), DEC, pa.time32("s"), pa.time32("ms"), pa.time64("us"), pa.time64("ns")]
    ks = schema(*key_types)
    allk = [col(k) for k in range(len(key_types))]
    for nulls in (False, True):
        hn = [nulls] * len(ks)
        tag = ", nullable" if nulls else ""
        for k, t in enumerate(key_types):
            add(f"key {tname(t)}: key words" + tag, lambda k=k, hn=hn: P.keys_source(ks, [col(k)], hn))
            add(f"key {tname(t)}: group by" + tag, lambda k=k, hn=hn: P.aggregate_source(ks, None, [col(k)], [E.CountAggregateExpr(col(0))], hn))
        add("keys: Int64 + Utf8 + Decimal128, probe" + tag, lambda hn=hn: P.probe_source(ks, [col(0), col(3), col(6)], gt0, hn))
        add("keys: Int64 + Utf8 + Decimal128, dense probe" + tag, lambda hn=hn: P.probe_source(ks, [col(0), col(3), col(6)], gt0, hn), QHIP_PLAN_DENSE=1)
        add("keys: Int64 + Utf8 + Decimal128, build entries" + tag, lambda hn=hn: P.scatter_source(ks, [col(0), col(3), col(6)], gt0, hn))
        add("keys: Int64 + Utf8 + Decimal128, dense build" + tag, lambda hn=hn: P.scatter_source(ks, [col(0), col(3), col(6)], gt0, hn), QHIP_PLAN_DENSE=1)
        add("keys: Int64 + Utf8 + Decimal128, dense build, no filter" + tag, lambda hn=hn: P.scatter_source(ks, [col(0), col(3), col(6)], None, hn), QHIP_PLAN_DENSE=1)
        add("keys: Int64 + Utf8 + Decimal128, partition" + tag, lambda hn=hn: P.partition_source(ks, [col(0), col(3), col(6)], gt0, 16, hn))
        add("keys: Int64 + Utf8 + Decimal128, partition, no filter, device-side row count" + tag, lambda hn=hn: P.partition_source(ks, [col(0), col(3), col(6)], None, 3, hn),
            QHIP_PLAN_DEV_ROWS=1)
        add("keys: Int64 + Utf8 + Decimal128, group by" + tag, lambda hn=hn: P.aggregate_source(ks, gt0, [col(0), col(3), col(6)], [E.CountAggregateExpr(col(1))], hn))
        add("keys: computed Utf8 and literal Utf8" + tag, lambda hn=hn: P.aggregate_source(ks, None, [E.CaseExpr([(gt0, col(3))], lit(SV.Utf8("none"))), lit(SV.Utf8("a literal key of 31 bytes ......"))],
                                                                                           [E.CountAggregateExpr(col(1))], hn))
        add("keys: one-byte Utf8 keys, group by" + tag, lambda hn=hn: P.aggregate_source(ks, None, [col(3)], [E.CountAggregateExpr(col(1))], hn), QHIP_PLAN_UTF8_FIXED1="3")
        add("keys: one-byte Utf8 keys, plain loads" + tag, lambda hn=hn: P.aggregate_source(ks, None, [col(3)], [E.CountAggregateExpr(col(1))], hn), QHIP_PLAN_UTF8_FIXED1="3", QHIP_NO_NT=1)
        add("keys: one-byte Utf8 key, probe" + tag, lambda hn=hn: P.probe_source(ks, [col(3)], None, hn), QHIP_PLAN_UTF8_FIXED1="3")
    add("keys: Utf8 literal longer than 55 bytes", lambda: P.keys_source(ks, [lit(SV.Utf8("x" * 56))]))
    add("keys: Utf8 literal of 55 bytes", lambda: P.keys_source(ks, [lit(SV.Utf8("x" * 55))]))
    for t in (boo, f64, f32, pa.int8(), pa.int16(), pa.uint16(), pa.uint32(), u64, pa.null(), pa.timestamp("us")):
        add(f"key {tname(t)} is no hasher type: key words", lambda t=t: P.keys_source(schema(t), [col(0)]))
        add(f"key {tname(t)} is no hasher type: group by", lambda t=t: P.aggregate_source(schema(t, i64), None, [col(0)], [E.CountAggregateExpr(col(1))]))
    i61 = schema(*([i64] * 61))
    add("keys: 61 key columns, key words", lambda: P.keys_source(i61, [col(k) for k in range(61)]))
    add("keys: 61 key columns, group by", lambda: P.aggregate_source(i61, None, [col(k) for k in range(61)], [E.CountAggregateExpr(col(0))]))
    add("keys: 9 words, key words", lambda: P.keys_source(i61, [col(k) for k in range(9)]))
    add("keys: 9 words, group by", lambda: P.aggregate_source(i61, None, [col(k) for k in range(9)], [E.CountAggregateExpr(col(0))]))
    add("keys: 8 words, key words", lambda: P.keys_source(i61, [col(k) for k in range(8)]))
    add("keys: 8 words, group by", lambda: P.aggregate_source(i61, None, [col(k) for k in range(8)], [E.CountAggregateExpr(col(0))]))
    add("keys: 8 words and a null mask, group by", lambda: P.aggregate_source(i61, None, [col(k) for k in range(8)], [E.CountAggregateExpr(col(0))], [True] * 61))
    add("keys: 8 words, nullable, key words (no mask word)", lambda: P.keys_source(i61, [col(k) for k in range(8)], [True] * 61))
    for n_parts in (0, 1, 255, 256):
        add(f"partition into {n_parts} parts", lambda n_parts=n_parts: P.partition_source(ks, [col(0)], None, n_parts))
    # two errors in one plan: which is reported
    add("two errors: non-Boolean predicate and a Float64 key, group by", lambda: P.aggregate_source(schema(f64, i64), col(1), [col(0)], [E.CountAggregateExpr(col(1))]))
    add("two errors: non-Boolean predicate and a Float64 key, probe", lambda: P.probe_source(schema(f64, i64), [col(0)], col(1)))
    add("two errors: non-Boolean predicate and a Float64 key, partition", lambda: P.partition_source(schema(f64, i64), [col(0)], col(1), 4))
    add("two errors: non-Boolean predicate and 9 key words, group by", lambda: P.aggregate_source(i61, col(0), [col(k) for k in range(9)], [E.CountAggregateExpr(col(0))]))
    add("two errors: non-Boolean predicate and 9 key words, probe", lambda: P.probe_source(i61, [col(k) for k in range(9)], col(0)))
    add("two errors: non-Boolean predicate and 0 parts", lambda: P.partition_source(i61, [col(0)], col(0), 0))
    add("two errors: 9 key words and 0 parts", lambda: P.partition_source(i61, [col(k) for k in range(9)], None, 0))
    add("two errors: 61 keys of which one Float64", lambda: P.keys_source(schema(*([i64] * 60 + [f64])), [col(k) for k in range(61)]))
    add("two errors: non-Boolean predicate and a bad SUM, group by", lambda: P.aggregate_source(schema(i64, utf), col(0), [col(0)], [E.SumAggregateExpr(col(1), utf)]))
    add("two errors: 9 key words and a bad SUM", lambda: P.aggregate_source(schema(*([i64] * 9 + [utf])), None, [col(k) for k in range(9)], [E.SumAggregateExpr(col(9), utf)]))
    add("two errors: a bad SUM before a bad MIN", lambda: P.aggregate_source(schema(i64, utf), None, [col(0)], [E.SumAggregateExpr(col(1), utf), E.MinAggregateExpr(col(1), utf)]))
    add("two errors: a bad MIN before a bad SUM", lambda: P.aggregate_source(schema(i64, utf), None, [col(0)], [E.MinAggregateExpr(col(1), utf), E.SumAggregateExpr(col(1), utf)]))
    add("two errors: non-Boolean predicate and a Utf8 literal key that is too long", lambda: P.aggregate_source(schema(i64), col(0), [lit(SV.Utf8("x" * 56))], [E.CountAggregateExpr(col(0))]))
    add("two errors: mask root out of range beats typing", lambda: P.filter_source(schema(i64), RawIndex(5)))
    add("predicate: not Boolean, mask", lambda: P.filter_source(schema(i64), col(0)))
    add("predicate: not Boolean, group by", lambda: P.aggregate_source(schema(i64), col(0), [col(0)], [E.CountAggregateExpr(col(0))]))
    add("predicate: not Boolean, build entries", lambda: P.scatter_source(schema(i64), [col(0)], col(0)))

    # ---------------------------------------------------------------- aggregates
    ag = schema(i64, u64, f64, DEC, i32, f32, d32, pa.timestamp("ns"), utf, boo, pa.null(), u8)
    avg_dec = pa.decimal128(19, 6)

    def all_aggs():
        return [E.CountAggregateExpr(col(0)), E.SumAggregateExpr(col(0), i64), E.SumAggregateExpr(col(1), u64), E.SumAggregateExpr(col(2), f64), E.SumAggregateExpr(col(3), DEC),
                E.AvgAggregateExpr(col(2), f64, f64), E.AvgAggregateExpr(col(3), DEC, avg_dec), E.MinAggregateExpr(col(3), DEC), E.MaxAggregateExpr(col(3), DEC),
                E.MinAggregateExpr(col(0), i64), E.MaxAggregateExpr(col(1), u64), E.MinAggregateExpr(col(2), f64), E.MaxAggregateExpr(col(5), f32), E.MinAggregateExpr(col(6), d32),
                E.MaxAggregateExpr(col(7), pa.timestamp("ns")), E.MaxAggregateExpr(col(11), u8), E.CountAggregateExpr(col(8)), E.CountAggregateExpr(col(10)),
                E.SumAggregateExpr(b(col(3), Op.Mul, col(3)), pa.decimal128(31, 4)), E.CountAggregateExpr(lit(SV.Int64(1)))]

    for nulls in (False, True):
        hn = [nulls] * len(ag)
        tag = ", nullable" if nulls else ""
        add("aggregates: every kind, grouped" + tag, lambda hn=hn: P.aggregate_source(ag, gt0, [col(4)], all_aggs(), hn))
        add("aggregates: every kind, ungrouped" + tag, lambda hn=hn: P.aggregate_source(ag, gt0, [], all_aggs(), hn))
        add("aggregates: every kind, grouped, no filter" + tag, lambda hn=hn: P.aggregate_source(ag, None, [col(4), col(6)], all_aggs(), hn))
        add("aggregates: every kind, device-side row count" + tag, lambda hn=hn: P.aggregate_source(ag, None, [col(4)], all_aggs(), hn), QHIP_PLAN_DEV_ROWS=1)
        for k, a in enumerate(all_aggs()):
            add(f"aggregates: kind {k} alone" + tag, lambda k=k, hn=hn: P.aggregate_source(ag, None, [col(4)], [all_aggs()[k]], hn))
        add("aggregates: no aggregate at all" + tag, lambda hn=hn: P.aggregate_source(ag, None, [col(4)], [], hn))
    # the tuning policy: bounded Decimal128 arguments on both sides of 2^39 and 2^63, with and without narrow copies
    for bits in (38, 39, 40, 62, 63):
        for nd in (1, 0):
            add(f"aggregates: SUM/MIN of a Decimal128 below 2^{bits}" + ("" if nd else ", Arrow layout"),
                lambda: P.aggregate_source(ag, gt0, [col(4)], [E.SumAggregateExpr(col(3), DEC), E.MinAggregateExpr(col(3), DEC), E.CountAggregateExpr(col(3))]),
                QHIP_PLAN_VALUE_BITS=f"3:{bits}", QHIP_NARROW_DECIMALS=nd)
    s8 = schema(i32, *([DEC] * 13))
    for n in range(1, 14):
        sums = [E.SumAggregateExpr(col(k), DEC) for k in range(1, n + 1)]
        bits = ",".join(f"{k}:20" for k in range(1, n + 1))
        add(f"aggregates: {n} wide SUMs", lambda sums=sums: P.aggregate_source(s8, None, [col(0)], sums))
        add(f"aggregates: {n} narrow SUMs", lambda sums=sums: P.aggregate_source(s8, None, [col(0)], sums), QHIP_PLAN_VALUE_BITS=bits)
        add(f"aggregates: {n} narrow SUMs, Arrow layout", lambda sums=sums: P.aggregate_source(s8, None, [col(0)], sums), QHIP_PLAN_VALUE_BITS=bits, QHIP_NARROW_DECIMALS=0)
        add(f"aggregates: {n} narrow SUMs, nullable", lambda sums=sums: P.aggregate_source(s8, None, [col(0)], sums, [False] + [True] * 13), QHIP_PLAN_VALUE_BITS=bits)
    add("aggregates: slot too wide for the staged scatter", lambda: P.aggregate_source(s8, None, [col(0)], [E.MinAggregateExpr(col(k), DEC) for k in range(1, 7)]))
    # the consecutive-rows form: which column layouts allow it
    cons = schema(i32, i64, utf, boo, DEC, f64)
    for name, groups, arg, env in (("Int32 key, Int64 argument", [col(0)], col(1), {}), ("Utf8 key", [col(2)], col(1), {}), ("one-byte Utf8 key", [col(2)], col(1), {"QHIP_PLAN_UTF8_FIXED1": "2"}),
                                   ("Boolean in the filter", [col(0)], E.CaseExpr([(col(3), col(1))], lit(SV.Int64(0))), {}), ("16-byte Decimal128", [col(0)], col(4), {}),
                                   ("narrow Decimal128", [col(0)], col(4), {"QHIP_PLAN_VALUE_BITS": "4:30"}), ("indirect columns", [col(0)], col(1), {"QHIP_PLAN_INDIRECT": "1"}),
                                   ("no column at all", [], lit(SV.Int64(1)), {}), ("Float64 argument", [col(0)], col(5), {})):
        for mode in (0, 1, 2):
            def fn(groups=groups, arg=arg):
                t = DEC if (isinstance(arg, E.Column) and arg.index == 4) else f64 if (isinstance(arg, E.Column) and arg.index == 5) else i64
                return P.aggregate_source(cons, None, groups, [E.SumAggregateExpr(arg, t)])
            add(f"consecutive rows, mode {mode}: {name}", fn, QHIP_AGG_CONS=mode, **env)
        add(f"consecutive rows: {name}, nullable", lambda groups=groups, arg=arg: P.aggregate_source(cons, None, groups, [E.CountAggregateExpr(arg)], [True] * len(cons)), QHIP_AGG_CONS=2, **env)
    add("consecutive rows: device-side row count", lambda: P.aggregate_source(cons, None, [col(0)], [E.SumAggregateExpr(col(1), i64)]), QHIP_AGG_CONS=2, QHIP_PLAN_DEV_ROWS=1)
    # the errors of plan_aggregate
    add("aggregates: argument index out of range", lambda: P.aggregate_source(ag, None, [col(4)], [E.CountAggregateExpr(RawIndex(99))]))
    add("aggregates: negative argument index", lambda: P.aggregate_source(ag, None, [col(4)], [E.CountAggregateExpr(RawIndex(-1))]))
    add("aggregates: SUM returning Int32", lambda: P.aggregate_source(ag, None, [col(4)], [E.SumAggregateExpr(col(4), i32)]))
    add("aggregates: SUM of Int32 returning Int64", lambda: P.aggregate_source(ag, None, [col(4)], [E.SumAggregateExpr(col(4), i64)]))
    add("aggregates: AVG of Int64", lambda: P.aggregate_source(ag, None, [col(4)], [E.AvgAggregateExpr(col(0), i64, f64)]))
    add("aggregates: AVG of Decimal128 returning Float64", lambda: P.aggregate_source(ag, None, [col(4)], [E.AvgAggregateExpr(col(3), DEC, f64)]))
    add("aggregates: MIN returning another type", lambda: P.aggregate_source(ag, None, [col(4)], [E.MinAggregateExpr(col(0), i32)]))
    add("aggregates: MIN of Decimal128 returning another scale", lambda: P.aggregate_source(ag, None, [col(4)], [E.MinAggregateExpr(col(3), avg_dec)]))
    add("aggregates: MAX over Utf8", lambda: P.aggregate_source(ag, None, [col(4)], [E.MaxAggregateExpr(col(8), utf)]))
    add("aggregates: MIN over Boolean", lambda: P.aggregate_source(ag, None, [col(4)], [E.MinAggregateExpr(col(9), boo)]))
    add("aggregates: unknown kind", lambda: P.aggregate_source(ag, None, [col(4)], [RawAgg(9, col(0), i64)]))
    add("aggregates: the same argument twice shares its cells", lambda: P.aggregate_source(ag, None, [col(4)], [E.SumAggregateExpr(col(3), DEC), E.AvgAggregateExpr(col(3), DEC, avg_dec),
                                                                                                                E.CountAggregateExpr(col(3)), E.SumAggregateExpr(col(3), DEC)], [True] * len(ag)))

    # ---------------------------------------------------------------- exchange pass 2
    for n_parts in (2, 8, 9, 16, 17, 255):
        add(f"partition scatter: every width, {n_parts} parts", lambda n_parts=n_parts: P.part_scatter_source([0, 1, 2, 4, 8, 16], n_parts, [False, True, False, True, False, True]))
    add("partition scatter: no column", lambda: P.part_scatter_source([], 8))
    add("partition scatter: 9 columns", lambda: P.part_scatter_source([8] * 9, 8))
    add("partition scatter: 8 columns", lambda: P.part_scatter_source([8] * 8, 8))
    add("partition scatter: device-side row count", lambda: P.part_scatter_source([8, 4], 8), QHIP_PLAN_DEV_ROWS=1)
    ps = lambda: P.part_scatter_source([0, 1, 2, 4, 8, 16], 8, [False, False, True, False, False, True])  # noqa: E731
    for env in ({"QHIP_PART_SCATTER_R": 2}, {"QHIP_PART_SCATTER_R": 99}, {"QHIP_PART_SCATTER_DIRECT": 1}, {"QHIP_PART_SCATTER_DIRECT": 1, "QHIP_PART_SCATTER_NT": 1},
                {"QHIP_PART_SCATTER_DIRECT": 1, "QHIP_PART_SCATTER_NOSTORE": 1}, {"QHIP_PART_SCATTER_NOSTORE": 1}, {"QHIP_PART_SCATTER_NT": 1}, {"QHIP_PART_SCATTER_TB": 256},
                {"QHIP_PART_SCATTER_TB": 1000}, {"QHIP_PART_SCATTER_TB": 4096}, {"QHIP_PART_SCATTER_PIPE": 0}, {"QHIP_PART_SCATTER_TRASH": 1},
                {"QHIP_PART_SCATTER_TRASH": 1, "QHIP_PART_SCATTER_NT": 1, "QHIP_PART_SCATTER_NOSTORE": 1}):
        add("partition scatter: " + ", ".join(f"{k}={v}" for k, v in env.items()), ps, **env)

    # ---------------------------------------------------------------- projection and sort keys
    add("projection: 25 expressions", lambda: P.projection_source(schema(i64), [b(col(0), Op.Add, lit(SV.Int64(k))) for k in range(25)]))
    add("projection: 24 expressions", lambda: P.projection_source(schema(i64), [b(col(0), Op.Add, lit(SV.Int64(k % 20))) for k in range(24)]))
    add("projection: a computed Null", lambda: P.projection_source(schema(boo, pa.null()), [E.CaseExpr([(col(0), col(1))], col(1))]))
    add("projection: plain columns only", lambda: P.projection_source(schema(i64, utf), [col(0), col(1)]))
    add("projection: root out of range", lambda: P.projection_source(schema(i64), [RawIndex(7)]))
    sk_types = [i64, pa.int8(), pa.int16(), i32, u8, pa.uint16(), pa.uint32(), u64, f32, f64, boo, pa.null(), DEC, utf, d32, pa.date64(), pa.time32("s"), pa.time64("ns"), pa.timestamp("ms")]
    sk = schema(*sk_types)
    for nulls in (False, True):
        hn = [nulls] * len(sk)
        tag = ", nullable" if nulls else ""
        add("sort keys: every type" + tag, lambda hn=hn: P.sort_keys_source(sk, [col(k) for k in range(len(sk_types))], hn))
        for k, t in enumerate(sk_types):
            add(f"sort key {tname(t)}" + tag, lambda k=k, hn=hn: P.sort_keys_source(sk, [col(k)], hn))
        add("sort keys: computed" + tag, lambda hn=hn: P.sort_keys_source(sk, [b(col(0), Op.Add, col(0)), E.Negative(col(12)), E.IsNull(col(13)), E.CastExpr(col(3), f64)], hn))
    add("sort keys: a computed Utf8", lambda: P.sort_keys_source(sk, [E.CaseExpr([(col(10), col(13))], lit(SV.Utf8("z")))]))
    add("sort keys: 33 keys", lambda: P.sort_keys_source(sk, [col(k % 13) for k in range(33)]))
    add("sort keys: 32 keys", lambda: P.sort_keys_source(sk, [col(k % 13) for k in range(32)]))
    add("sort keys: none", lambda: P.sort_keys_source(sk, []))

    # ---------------------------------------------------------------- the switches the generator reads, at non-default values
    li = schema(d32, utf, utf, DEC, DEC, DEC, DEC, i64)
    q1 = dict(QHIP_PLAN_VALUE_BITS="3:13,4:24,5:4,6:4", QHIP_PLAN_UTF8_FIXED1="1,2")
    one = lit(SV.Decimal128(100, 15, 2))
    disc = b(col(4), Op.Mul, b(one, Op.Sub, col(5)))

    def q1ish():
        return P.aggregate_source(li, b(col(0), Op.LtEq, E.CastExpr(lit(SV.Utf8("1998-09-02")), d32)), [col(1), col(2)],
                                  [E.SumAggregateExpr(col(3), DEC), E.SumAggregateExpr(col(4), DEC), E.SumAggregateExpr(disc, pa.decimal128(31, 4)),
                                   E.AvgAggregateExpr(col(5), DEC, avg_dec), E.CountAggregateExpr(col(3))])

    add("switches: none (the plan the next entries vary)", q1ish, **q1)
    for env in ({"QHIP_NO_NT": 1}, {"QHIP_AGG_KC": 1}, {"QHIP_AGG_KC": 3}, {"QHIP_AGG_KC": 0}, {"QHIP_AGG_KC": ""}, {"QHIP_AGG_PART_PR": 1}, {"QHIP_AGG_PART_PR": 2}, {"QHIP_AGG_PART_PR": 0},
                {"QHIP_AGG_PART_PR": 9}, {"QHIP_AGG_CONS": 0}, {"QHIP_AGG_CONS": 2}, {"QHIP_AGG_CONS": 2, "QHIP_AGG_CONS_R": 2}, {"QHIP_AGG_CONS": 2, "QHIP_AGG_CONS_R": 8},
                {"QHIP_AGG_CONS": 2, "QHIP_AGG_CONS_R": 0}, {"QHIP_AGG_CONS": 2, "QHIP_AGG_CONS_R": 64}, {"QHIP_AGG_CONS_SB": 1}, {"QHIP_AGG_CONS_SB": 2}, {"QHIP_AGG_CONS_SB": 9},
                {"QHIP_AGG_CONS_PIPE": 0}, {"QHIP_AGG_PROF": 1}, {"QHIP_AGG_PIPE": 1}, {"QHIP_AGG_WAVES": 2}, {"QHIP_AGG_WAVES": 4, "QHIP_AGG_CONS": 2}, {"QHIP_AGG_R": 1}, {"QHIP_AGG_R": 3},
                {"QHIP_AGG_R": 8}, {"QHIP_AGG_R": ""}, {"QHIP_AGG_R": 0}, {"QHIP_PLAN_DEV_ROWS": 1}, {"QHIP_NARROW_DECIMALS": 0}):
        add("switches, aggregate: " + ", ".join(f"{k}={v}" for k, v in env.items()), q1ish, **dict(q1, **env))
    add("switches, aggregate, ungrouped: QHIP_AGG_KC=2", lambda: P.aggregate_source(li, None, [], [E.SumAggregateExpr(col(3), DEC)]), QHIP_AGG_KC=2)
    lpred = b(col(0), Op.Lt, E.CastExpr(lit(SV.Utf8("1995-03-15")), d32))
    for r in (1, 2, 16, 99):
        add(f"switches, mask: QHIP_MASK_R={r}", lambda: P.filter_source(li, lpred), QHIP_MASK_R=r)
    for env in ({"QHIP_PROBE_R": 1}, {"QHIP_PROBE_R": 2}, {"QHIP_PROBE_R": 3}, {"QHIP_PROBE_R": 8}, {"QHIP_PROBE_R": 99}, {"QHIP_PROBE_WAVES": 4}, {"QHIP_PROBE_R": 3, "QHIP_PROBE_WAVES": 7}):
        add("switches, probe: " + ", ".join(f"{k}={v}" for k, v in env.items()), lambda: P.probe_source(li, [col(7)], lpred), **env)
    for env in ({"QHIP_DENSE_PROBE_R": 1}, {"QHIP_DENSE_PROBE_R": 8}, {"QHIP_DENSE_PROBE_WAVES": 8}, {"QHIP_PLAN_NARROW_INTS": "7"}, {"QHIP_PLAN_NARROW_INTS": "7", "QHIP_DENSE_PROBE_R": 3},
                {"QHIP_PROBE_R": 3}):
        add("switches, dense probe: " + ", ".join(f"{k}={v}" for k, v in env.items()), lambda: P.probe_source(li, [col(7)], lpred), QHIP_PLAN_DENSE=1, **env)
    for env in ({"QHIP_PART_R": 1}, {"QHIP_PART_R": 8}, {"QHIP_PART_R": 99}, {"QHIP_PROBE_R": 2}, {"QHIP_PROBE_R": 2, "QHIP_PART_R": 2}):
        add("switches, partition: " + ", ".join(f"{k}={v}" for k, v in env.items()), lambda: P.partition_source(li, [col(7)], lpred, 8), **env)
    return out


def _binary_raw(left, op, right):
    class _B(E.PhysicalExpr):
        def _lower(self, o):
            return o.add(kind=E.K_BINARY, op=op, left=left._lower(o), right=right._lower(o))
    return _B()


def _node_raw(**kw):
    class _N(E.PhysicalExpr):
        def _lower(self, o):
            return o.add(**kw)
    return _N()


def _clean_env():
    saved = dict(os.environ)
    for k in list(os.environ):
        if k.startswith("QHIP_"):
            del os.environ[k]
    return saved


def _restore_env(saved):
    os.environ.clear()
    os.environ.update(saved)


def corpus():
    """{name: source text or "ERROR <code>: <message>"}, in corpus order."""
    out = {}
    saved = _clean_env()
    try:
        for name, src in catalog.catalog_sources():   # (sets and removes its own switches)
            out["catalog: " + name] = src
    finally:
        _restore_env(saved)
    for name, env, fn in entries():
        assert name not in out, "duplicate corpus entry " + name
        saved = _clean_env()
        try:
            os.environ.update(env)
            try:
                out[name] = fn()
            except _ffi.QuriousError as e:
                out[name] = f"ERROR {e.code}: {e}"
        finally:
            _restore_env(saved)
    return out


HEADER = ("Generated kernel source, digested: {entry: [sha256, bytes]}. Written by `python tools/codegen_corpus.py --digests > tests/golden/codegen_digests.json`. "
          "Regenerate it only in a change that alters generated code on purpose (or adds corpus entries), from a build of that change, and say so in the change; "
          "a change that only restructures the host code of the generator must pass tests/test_codegen_identity_cpu.py against this file as it is.")


def digests(texts=None):
    """{"#": HEADER, name: [sha256 of the text, its length in bytes]}"""
    texts = corpus() if texts is None else texts
    out = {"#": HEADER}
    out.update({name: [hashlib.sha256(t.encode()).hexdigest(), len(t.encode())] for name, t in texts.items()})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--digests", action="store_true", help="print {name: [sha256, length]} as JSON")
    ap.add_argument("--dump", metavar="DIR", help="write one text file per entry")
    a = ap.parse_args(argv)
    texts = corpus()
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        for k, (name, t) in enumerate(texts.items()):
            with open(os.path.join(a.dump, f"{k:04d}_" + re.sub(r"[^A-Za-z0-9]+", "_", name).strip("_")[:100] + ".txt"), "w") as f:
                f.write("# " + name + "\n" + t)
    if a.digests or not a.dump:
        json.dump(digests(texts), sys.stdout, indent=0, sort_keys=True)
        sys.stdout.write("\n")
    errors = sum(1 for t in texts.values() if t.startswith("ERROR "))
    print(f"{len(texts)} entries, {errors} of them errors", file=sys.stderr)


if __name__ == "__main__":
    main()
