"""The value vectors, expressions and error cases that tests/test_expr_model_cpu.py runs through the oracle and
tests/test_gpu_expr_semantics.py through the kernels; both compare with tests/expr_model.py.

A vector set is a table of N = 3 * 1024 + 37 rows (three tiles of the fused kernels and a ragged tail). Every column is its
type's edge values repeated, shuffled with a fixed seed, with about 10 % NULLs; the arrays are built from buffers and a NULL
slot holds a value that would overflow / divide by zero if it were read. The last column `id` is the row number.
No value vector raises (test_no_value_vector_raises); what raises lives in the error table at the end.
No float cast here uses a scale above 22 (expr_model.py: the model's authority ends there)."""
from __future__ import annotations

import math
import random
import struct
from typing import List, Sequence

import pyarrow as pa

import qurious_amd as q
from qurious_amd import Operator as Op
from qurious_amd import ScalarValue as S

from . import expr_model as M

N = 3 * 1024 + 37
I8, I16, I32, I64, U8, U16, U32, U64 = pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64()
F32, F64, D32, D64, BOOL = pa.float32(), pa.float64(), pa.date32(), pa.date64(), pa.bool_()
NAN, INF = math.nan, math.inf


def dec(p, s):
    return pa.decimal128(p, s)


def below(x: float) -> float:
    return math.nextafter(x, -INF)


def above(x: float) -> float:
    return math.nextafter(x, INF)


def f32_below(x: float) -> float:
    b = struct.unpack("<I", struct.pack("<f", x))[0]
    return struct.unpack("<f", struct.pack("<I", b - 1 if x > 0 else b + 1))[0]


def int_edges(t) -> List[int]:
    """MIN, MIN+1, -1, 0, 1, MAX-1, MAX and +-2^7, +-2^15, +-2^31, 2^32, 2^63-1 where the type holds them"""
    lo, hi = M.int_range(t)
    cand = [lo, lo + 1, -1, 0, 1, hi - 1, hi, 1 << 7, -(1 << 7), 1 << 15, -(1 << 15), 1 << 31, -(1 << 31), 1 << 32, (1 << 63) - 1]
    out = []
    for v in cand:
        if lo <= v <= hi and v not in out:
            out.append(v)
    return out


def col(name, index):
    return q.Column(name, index)


def lit(t, v):
    return q.Literal(S(t, v))


def cast(e, t):
    return q.CastExpr(e, t)


def b(l, op, r):
    return q.BinaryExpr(l, op, r)


class VectorSet:
    def __init__(self, name: str, seed: int, columns: Sequence[tuple]):
        """columns: (name, type, edge values, garbage under NULL)"""
        rng = random.Random(seed)
        self.name = name
        self.names, self.cols = [], []
        arrays = []
        for cname, t, edges, garbage in columns:
            vals = [edges[k % len(edges)] for k in range(N)]
            rng.shuffle(vals)
            vals = [None if rng.random() < 0.1 else v for v in vals]
            self.names.append(cname)
            self.cols.append(M.Value(t, vals))
            arrays.append(M.to_arrow(t, vals, garbage))
        self.names.append("id")
        self.cols.append(M.Value(I64, list(range(N))))
        arrays.append(pa.array(range(N), type=I64))
        self.schema = pa.schema([pa.field(n, a.type, True) for n, a in zip(self.names, arrays)])
        self.batch = pa.RecordBatch.from_arrays(arrays, schema=self.schema)
        self.exprs: List[tuple] = []      # (name, expression): every one is projected, and evaluated by the oracle
        self.filters: List[tuple] = []    # (name, predicate)
        self.agg_args: List[tuple] = []   # (name, expression, kinds): arguments of the fused aggregate
        self.agg_key = None               # a GROUP BY key expression
        self.agg_filter = None            # the fused predicate
        self.join_keys: List = []         # key expressions of the inner hash join (both sides)
        self.join_filter = None

    def c(self, name):
        return col(name, self.names.index(name))

    @property
    def id(self):
        return self.c("id")

    def table(self):
        return q.MemoryTable.try_new(self.schema, [self.batch])

    def scan(self, filter=None, table=None):
        return q.Scan(self.schema, table or self.table(), None, filter)


# ------------------------------------------------------------------------------------------------------------- integers
def _ints() -> VectorSet:
    i64max, i64min = (1 << 63) - 1, -(1 << 63)
    small = [-128, -127, -1, 0, 1, 126, 127]
    day_ms = M.MS_PER_DAY
    vs = VectorSet("ints", 11, [
        ("a8", I8, int_edges(I8), 127), ("a16", I16, int_edges(I16), 32767), ("a32", I32, int_edges(I32), (1 << 31) - 1),
        ("a64", I64, int_edges(I64) + [(1 << 60) + (1 << 36) + 1, (1 << 24) + 1, (1 << 53) + 1, -((1 << 24) + 3)], i64max),
        ("u8", U8, int_edges(U8), 255), ("u16", U16, int_edges(U16), 65535), ("u32", U32, int_edges(U32), (1 << 32) - 1),
        ("u64", U64, int_edges(U64) + [(1 << 60) + (1 << 36) + 1, (1 << 64) - (1 << 39) - 1], (1 << 64) - 1),
        ("s64", I64, small, i64max),                                            # fits every signed type; garbage overflows them
        ("n64", I64, [-7, -3, -2, 2, 3, 7, i64max, i64min, 1], 0),               # divisors: never 0, never -1; garbage divides by zero
        ("n32", I32, [-7, -3, 2, 3, 7, (1 << 31) - 1, -(1 << 31)], 0),
        ("nu64", U64, [1, 2, 3, 7, (1 << 64) - 1], 0),
        ("n8", I8, [-7, -3, 2, 3, 127, -128], 0),
        ("d32", D32, int_edges(I32), (1 << 31) - 1),
        ("d64", D64, [0, 1, -1, day_ms - 1, 1 - day_ms, day_ms, -day_ms, day_ms + 1, -day_ms - 1, ((1 << 31) - 1) * day_ms + day_ms - 1, -(1 << 31) * day_ms], i64max),
        ("b1", BOOL, [True, False], True), ("b2", BOOL, [False, True, True], True),
    ])
    c = vs.c
    E = vs.exprs
    for src, to in (("s64", I8), ("s64", I16), ("s64", I32), ("a16", I32), ("a32", I64), ("a8", I64), ("u8", U64), ("u8", I16), ("u16", I32), ("u32", I64),
                    ("u32", U64), ("d32", I32), ("a32", D32), ("d32", D64), ("d64", D32), ("d64", I64),
                    ("a64", F32), ("a64", F64), ("u64", F32), ("u64", F64), ("a32", F32), ("a32", F64), ("u32", F32), ("a8", F32),
                    ("b1", I32), ("b1", I64), ("b1", U8),
                    ("a64", dec(38, 19)), ("a32", dec(20, 2)), ("s64", dec(5, 2)), ("u64", dec(38, 18)), ("a8", dec(3, 0)), ("u32", dec(10, 0))):
        E.append((f"cast {src} -> {to}", cast(c(src), to)))
    for name, t in (("a8", I8), ("a16", I16), ("a32", I32), ("a64", I64), ("u8", U8), ("u16", U16), ("u32", U32), ("u64", U64)):
        E.append((f"{name} + 1", b(c(name), Op.Add, lit(t, 1))))
        E.append((f"{name} - 1", b(c(name), Op.Sub, lit(t, 1))))
        E.append((f"{name} * {name}", b(c(name), Op.Mul, c(name))))
        E.append((f"{name} * 3 + {name}", b(b(c(name), Op.Mul, lit(t, 3)), Op.Add, c(name))))
    for num, den in (("a64", "n64"), ("a32", "n32"), ("u64", "nu64"), ("a8", "n8")):
        E.append((f"{num} / {den}", b(c(num), Op.Div, c(den))))
        E.append((f"{num} % {den}", b(c(num), Op.Mod, c(den))))
    E.append(("a64 % -1", b(c("a64"), Op.Mod, lit(I64, -1))))   # (MIN % -1 = 0: the doubt of expr_model.py)
    E.append(("s64 % -1", b(c("s64"), Op.Mod, lit(I64, -1))))
    E.append(("a64 / 7", b(c("a64"), Op.Div, lit(I64, 7))))
    for name in ("a8", "a32", "a64"):
        E.append((f"-{name}", q.Negative(c(name))))
    E.append(("b1 AND b2", b(c("b1"), Op.And, c("b2"))))
    E.append(("b1 OR b2", b(c("b1"), Op.Or, c("b2"))))
    E.append(("a64 IS NULL", q.IsNull(c("a64"))))
    E.append(("b1 IS NOT NULL", q.IsNotNull(c("b1"))))
    E.append(("IF b1 THEN a64 ELSE s64", q.CaseExpr([(c("b1"), c("a64"))], c("s64"))))
    E.append(("IF a64 > 0 THEN a64 / n64 ELSE a64 % n64", q.CaseExpr([(b(c("a64"), Op.Gt, lit(I64, 0)), b(c("a64"), Op.Div, c("n64")))], b(c("a64"), Op.Mod, c("n64")))))
    E.append(("a64 < s64", b(c("a64"), Op.Lt, c("s64"))))
    E.append(("u64 >= 2^63", b(c("u64"), Op.GtEq, lit(U64, 1 << 63))))
    E.append(("b1 = b2", b(c("b1"), Op.Eq, c("b2"))))
    vs.filters = [
        ("int -> int", b(cast(c("s64"), I8), Op.Lt, lit(I8, 1))),
        ("Date64 -> Date32", b(cast(c("d64"), D32), Op.GtEq, lit(D32, 1))),
        ("int -> float", b(cast(c("a64"), F32), Op.Gt, lit(F32, float(1 << 60)))),     # one rounding: 2^60 + 2^37 passes, 2^60 would not
        ("bool -> int", b(cast(c("b1"), I32), Op.Eq, lit(I32, 1))),
        ("int -> decimal", b(cast(c("a64"), dec(38, 19)), Op.Gt, lit(dec(38, 19), 10 ** 19))),
        ("checked division", b(b(c("a64"), Op.Div, c("n64")), Op.LtEq, b(c("a64"), Op.Mod, c("n64")))),
        ("wrapping", b(b(c("a32"), Op.Add, lit(I32, 1)), Op.Lt, c("a32"))),
    ]
    # (SUM only where the exact sum stays far inside its accumulator; MIN / MAX never over a NaN or an all-NULL group)
    vs.agg_key = cast(c("s64"), I32)
    vs.agg_filter = b(cast(c("b1"), I32), Op.Eq, lit(I32, 1))
    vs.agg_args = [("int -> int", cast(c("a32"), I64), ("sum", "min")), ("int -> float", cast(c("a64"), F32), ("min", "max")),
                   ("int -> decimal", cast(c("a32"), dec(20, 2)), ("sum", "max")), ("int -> wide decimal", cast(c("a64"), dec(38, 19)), ("min", "max")), ("bool -> int", cast(c("b2"), I64), ("sum",)),
                   ("Date32 -> Date64", cast(c("d32"), D64), ("min", "max")), ("division", b(c("a64"), Op.Div, c("n64")), ("min", "max")),
                   ("remainder", b(c("u64"), Op.Mod, c("nu64")), ("min", "max")), ("wrapping", b(c("a64"), Op.Mul, c("a64")), ("min", "max"))]
    vs.join_keys = [cast(c("s64"), I32), cast(c("b1"), I64), cast(c("a8"), dec(3, 0)), b(c("s64"), Op.Div, c("n64"))]
    vs.join_filter = b(cast(c("b2"), I32), Op.Eq, lit(I32, 1))
    return vs


# --------------------------------------------------------------------------------------------------------------- floats
def _floats() -> VectorSet:
    p31, p63, p64 = float(1 << 31), float(1 << 63), float(1 << 64)
    halves = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5]
    vs = VectorSet("floats", 12, [
        ("x64", F64, halves + [NAN, below(p31), p31, -p31, below(-p31), below(p63), p63, -p63, below(-p63), below(p64), p64, float((1 << 24) + 1), float((1 << 24) + 3),
                               1e300, -1e300, 1e-40, 1e-320], NAN),
        ("x_i32", F64, halves + [below(p31), -p31, below(-p31), float((1 << 24) + 1)], p31),           # legal for Int32; garbage is not
        ("x_i64", F64, halves + [below(p63), -p63, float((1 << 53) + 2), -p31, p31], p63),
        ("x_u64", F64, [0.0, -0.0, -0.5, 0.5, 1.5, 2.5, below(p64), p63, float(1 << 32), below(p63)], p64),
        ("x_i8", F64, halves + [127.9, -128.9, 127.0, -128.0], 128.0),
        ("x_d", F64, halves + [0.125, 0.375, -0.125, 1234567.891, -99999999.99, 0.005, 0.015, 1e-9], INF),
        ("x_d23", F64, [float(10 ** 23), -float(10 ** 23), 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 1e22], INF),
        ("x_d38", F64, [float(10 ** 38), -float(10 ** 38), 2.5, -2.5, float(1 << 100)], INF),
        ("y32", F32, halves + [NAN, float(1 << 24), f32_below(p31), -p31, M.f32(3.4e38), M.f32(1e-40), M.f32(0.1)], NAN),
        ("y_i32", F32, halves + [f32_below(p31), -p31, float(1 << 24)], p31),
        ("nz64", F64, [0.5, -0.5, 1.5, -1.5, 2.5, 3.0, 1e10], 0.0),
        ("nz32", F32, [0.5, -0.5, 1.5, -1.5, 3.0, M.f32(1e10)], 0.0),
    ])
    c = vs.c
    E = vs.exprs
    for src, to in (("x64", F32), ("y32", F64), ("x_i32", I32), ("x_i32", I64), ("x_i64", I64), ("x_u64", U64), ("x_i8", I8), ("x_i8", I16), ("x_i8", I32),
                    ("y_i32", I32), ("y_i32", I64), ("x_d", dec(10, 2)), ("x_d", dec(20, 6)), ("x_d23", dec(23, 0)), ("x_d38", dec(38, 0)), ("y_i32", dec(12, 2))):
        E.append((f"cast {src} -> {to}", cast(c(src), to)))
    E.append(("x64 + x64", b(c("x64"), Op.Add, c("x64"))))
    E.append(("x64 - nz64", b(c("x64"), Op.Sub, c("nz64"))))
    E.append(("x64 * nz64", b(c("x64"), Op.Mul, c("nz64"))))
    E.append(("x_i64 / nz64", b(c("x_i64"), Op.Div, c("nz64"))))
    E.append(("x_i64 % nz64", b(c("x_i64"), Op.Mod, c("nz64"))))
    E.append(("y32 + y32", b(c("y32"), Op.Add, c("y32"))))
    E.append(("y32 * nz32", b(c("y32"), Op.Mul, c("nz32"))))
    E.append(("y_i32 / nz32", b(c("y_i32"), Op.Div, c("nz32"))))
    E.append(("y_i32 % nz32", b(c("y_i32"), Op.Mod, c("nz32"))))
    E.append(("-x64", q.Negative(c("x64"))))
    E.append(("-y32", q.Negative(c("y32"))))
    E.append(("x64 < nz64", b(c("x64"), Op.Lt, c("nz64"))))
    E.append(("x64 = NaN", b(c("x64"), Op.Eq, lit(F64, NAN))))
    E.append(("x64 >= +0.0", b(c("x64"), Op.GtEq, lit(F64, 0.0))))        # total order: -0.0 < +0.0
    E.append(("y32 <= 0.5", b(c("y32"), Op.LtEq, lit(F32, 0.5))))
    E.append(("x64 != x64", b(c("x64"), Op.NotEq, c("x64"))))               # total order: NaN = NaN
    E.append(("IF x64 < 0 THEN x64 ELSE -x64", q.CaseExpr([(b(c("x64"), Op.Lt, lit(F64, 0.0)), c("x64"))], q.Negative(c("x64")))))
    vs.filters = [
        ("float -> float", b(cast(c("x64"), F32), Op.Eq, lit(F32, float(1 << 24)))),
        ("float -> int", b(cast(c("x_i64"), I64), Op.Lt, lit(I64, 2))),
        ("float -> uint", b(cast(c("x_u64"), U64), Op.GtEq, lit(U64, 1 << 63))),
        ("float -> decimal", b(cast(c("x_d23"), dec(23, 0)), Op.GtEq, lit(dec(23, 0), 2))),
        ("total order", b(c("x64"), Op.GtEq, lit(F64, 0.0))),
        ("fmod", b(b(c("x_i64"), Op.Mod, c("nz64")), Op.Lt, lit(F64, 0.0))),
    ]
    vs.agg_key = cast(c("x_i8"), I32)
    vs.agg_filter = b(cast(c("x_d"), dec(10, 2)), Op.GtEq, lit(dec(10, 2), 0))
    vs.agg_args = [("float -> float", cast(c("x_i64"), F32), ("min", "max")), ("float -> int", cast(c("x_i64"), I64), ("min", "max")), ("float -> small int", cast(c("x_i8"), I64), ("sum",)),
                   ("float -> uint", cast(c("x_u64"), U64), ("min", "max")), ("float -> decimal", cast(c("x_d23"), dec(23, 0)), ("sum", "max")),
                   ("float -> decimal 38", cast(c("x_d38"), dec(38, 0)), ("min", "max")), ("fmod", b(c("x_i64"), Op.Mod, c("nz64")), ("min", "max")),
                   ("f32 -> int", cast(c("y_i32"), I32), ("min", "max"))]
    vs.join_keys = [cast(c("x_i8"), I32), cast(c("x_i64"), I64), cast(c("x_d"), dec(10, 2))]
    vs.join_filter = b(cast(c("y_i32"), I32), Op.GtEq, lit(I32, 0))
    return vs


# ------------------------------------------------------------------------------------------------------------- decimals
def _decimals() -> VectorSet:
    huge = (1 << 127) - 1

    def pm(*vals):
        out = [0]
        for v in vals:
            out += [v, -v]
        return out
    vs = VectorSet("decimals", 13, [
        ("ds", dec(9, 2), pm(1, 49, 50, 51, 149, 150, 151, 10 ** 9 - 1), huge),                                      # fits 31 bits
        ("dm", dec(18, 4), pm(1, 4999, 5000, 5001, 12345, 1 << 40, 10 ** 18 - 1), huge),                             # fits 63 bits
        ("dw", dec(38, 10), pm(1, 4999999999, 5 * 10 ** 9, 5 * 10 ** 9 + 1, 1 << 64, 1 << 100, 10 ** 38 - 1), huge),  # wider
        ("dw0", dec(38, 0), pm(1, 1 << 63, 1 << 70, 10 ** 29 - 1), huge),
        ("dnz", dec(9, 2), [1, -1, 3, -3, 150, -150, 10 ** 9 - 1, 1 - 10 ** 9], 0),
        ("dsm", dec(18, 4), pm(1, 9999, 10000, 10001) + [21474836479999, -21474836489999, 21474836470000], huge),
    ])
    c = vs.c
    E = vs.exprs
    for src, to in (("ds", dec(15, 6)), ("dm", dec(38, 10)), ("dw0", dec(38, 9)), ("ds", dec(9, 2)), ("dsm", dec(38, 20)),   # up (and the identity)
                    ("ds", dec(9, 0)), ("ds", dec(9, 1)), ("dm", dec(18, 2)), ("dm", dec(16, 0)), ("dw", dec(38, 4)), ("dw", dec(29, 0)),   # down by k
                    ("ds", I32), ("ds", I64), ("dm", I64), ("dsm", I32), ("dsm", I64),
                    ("ds", F64), ("ds", F32), ("dm", F64), ("dm", F32), ("dw", F64), ("dw0", F32), ("dw0", F64)):
        E.append((f"cast {src} -> {to}", cast(c(src), to)))
    for name, l, op, r in (("ds + dm", "ds", Op.Add, "dm"), ("dm - ds", "dm", Op.Sub, "ds"), ("ds * ds", "ds", Op.Mul, "ds"), ("ds * dm", "ds", Op.Mul, "dm"),
                           ("dm * dm", "dm", Op.Mul, "dm"), ("dw0 * ds", "dw0", Op.Mul, "ds"), ("dw0 + dm", "dw0", Op.Add, "dm"), ("dw + ds", "dw", Op.Add, "ds"),
                           ("ds / dnz", "ds", Op.Div, "dnz"), ("dm / dnz", "dm", Op.Div, "dnz"), ("dw / dnz", "dw", Op.Div, "dnz"), ("ds < dnz", "ds", Op.Lt, "dnz")):
        E.append((name, b(c(l), op, c(r))))
    E.append(("-dw", q.Negative(c("dw"))))
    E.append(("-ds", q.Negative(c("ds"))))
    E.append(("dw >= 5e-1", b(c("dw"), Op.GtEq, lit(dec(38, 10), 5 * 10 ** 9))))
    vs.filters = [
        ("decimal up", b(cast(c("dw0"), dec(38, 9)), Op.Gt, lit(dec(38, 9), 10 ** 28))),
        ("decimal down", b(cast(c("dm"), dec(18, 2)), Op.GtEq, lit(dec(18, 2), 50))),        # 0.5000 and 0.4999 -> 0.50 (half away from zero): both pass
        ("decimal down, negative", b(cast(c("dw"), dec(38, 4)), Op.LtEq, lit(dec(38, 4), -500000))),
        ("decimal -> int", b(cast(c("dsm"), I32), Op.Eq, lit(I32, 0))),
        ("decimal -> float", b(cast(c("dm"), F32), Op.Lt, lit(F32, 0.5))),
        ("decimal arithmetic", b(b(c("ds"), Op.Add, c("dm")), Op.Gt, b(c("dm"), Op.Sub, c("ds")))),
    ]
    vs.agg_key = cast(c("ds"), dec(9, 0))
    vs.agg_filter = b(cast(c("dsm"), I32), Op.GtEq, lit(I32, 0))
    vs.agg_args = [("decimal up", cast(c("dw0"), dec(38, 9)), ("min", "max")), ("decimal down", cast(c("dw"), dec(38, 4)), ("sum", "max")),
                   ("decimal -> int", cast(c("dm"), I64), ("sum", "min")), ("decimal -> float", cast(c("dm"), F32), ("min", "max")),
                   ("decimal -> double", cast(c("dw"), F64), ("min", "max")), ("product", b(c("dm"), Op.Mul, c("dm")), ("sum", "max")),
                   ("quotient", b(c("dm"), Op.Div, c("dnz")), ("min", "max"))]
    vs.join_keys = [cast(c("ds"), dec(9, 0)), cast(c("dsm"), I32), cast(c("dm"), dec(18, 2))]
    vs.join_filter = b(cast(c("dsm"), I64), Op.GtEq, lit(I64, -1))
    return vs


_SETS = {}


def vector_set(name: str) -> VectorSet:
    """built once per process and shared (never modified)"""
    if name not in _SETS:
        _SETS[name] = {"ints": _ints, "floats": _floats, "decimals": _decimals}[name]()
    return _SETS[name]


SET_NAMES = ("ints", "floats", "decimals")


def chunks(exprs: Sequence[tuple], limit: int = 20) -> List[List[tuple]]:
    """the expressions in groups one Projection kernel takes (at most 24 outputs, columns and literals; 20 leaves room)"""
    return [list(exprs[k:k + limit]) for k in range(0, len(exprs), limit)]


# ---------------------------------------------------------------------------------------------------------- error cases
# One table, one plan per context, many fallible expressions over columns of their own; a run poisons exactly ONE row of
# one column (or a pair of columns), so the same kernels serve every case.
POISON_ROWS = (17, 2 * 1024 + 500, 3 * 1024 + 30)   # first tile, last full tile, ragged tail


class ErrorTable:
    """columns: g (the fused filter passes g > 0), k (a key), then one column per fallible expression, then id"""
    COLUMNS = [
        # name, type, harmless values, garbage under NULL
        ("g", I64, [1, 2, 3], 1), ("k", I64, [0, 1, 2, 3, 4, 5, 6], 0),
        ("num", I64, [-9, -1, 0, 5, 1 << 40, -(1 << 63)], 7), ("den", I64, [1, 2, -3, 7, -1 << 20], 0),
        ("ci", I64, [-(1 << 31), -1, 0, (1 << 31) - 1], 1 << 40),
        ("cf", F64, [0.5, -2.5, below(float(1 << 63)), -float(1 << 63)], NAN),
        ("cu", F64, [0.0, -0.5, below(float(1 << 64))], -1.0),
        ("cid", I64, [0, 1, -1, 10 ** 8 - 1, 1 - 10 ** 8], 1 << 62),
        ("cdd", dec(38, 0), [0, 1, -1, 10 ** 29 - 1, 1 - 10 ** 29], (1 << 127) - 1),
        ("cdn", dec(9, 2), [0, 49, 50, -50, 999999949, -999999949], 999999999),
        ("cdi", dec(18, 4), [0, 9999, -9999, 21474836479999, -21474836489999], 10 ** 18 - 1),
        ("cfd", F64, [float(10 ** 23), -float(10 ** 23), 0.5, -0.5], INF),
        ("cf32", F64, [below(float(1 << 31)), below(-float(1 << 31)), 2.5], float(1 << 31)),
    ]

    def __init__(self):
        self.names = [c[0] for c in self.COLUMNS] + ["id"]
        self.types = [c[1] for c in self.COLUMNS] + [I64]
        self.garbage = [c[3] for c in self.COLUMNS] + [0]
        rng = random.Random(99)
        self.base = []
        for name, _t, edges, _g in self.COLUMNS:
            vals = [edges[k % len(edges)] for k in range(N)]
            rng.shuffle(vals)
            if name not in ("g", "k"):
                vals = [None if rng.random() < 0.1 else v for v in vals]
            self.base.append(vals)
        self.base.append(list(range(N)))
        for r in POISON_ROWS:   # the poisoned rows are plain rows otherwise: valid everywhere, passing the filter
            for k, column in enumerate(self.COLUMNS):
                self.base[k][r] = column[2][0]
        self.schema = pa.schema([pa.field(n, t, True) for n, t in zip(self.names, self.types)])
        self._base_arrays, self._cases, self._exprs, self._filter = None, {}, None, None

    def c(self, name):
        return col(name, self.names.index(name))

    def exprs(self) -> List[tuple]:
        """(family, expression): `family` names the columns a poison goes into"""
        if self._exprs is not None:
            return self._exprs   # (the same objects every time: expr_model.Memo goes by identity)
        c = self.c
        self._exprs = [("div", b(c("num"), Op.Div, c("den"))), ("mod", b(c("num"), Op.Mod, c("den"))), ("ci", cast(c("ci"), I32)), ("cf", cast(c("cf"), I64)),
                ("cu", cast(c("cu"), U64)), ("cid", cast(c("cid"), dec(38, 30))), ("cdd", cast(c("cdd"), dec(38, 9))), ("cdn", cast(c("cdn"), dec(7, 0))),
                ("cdi", cast(c("cdi"), I32)), ("cfd", cast(c("cfd"), dec(23, 0))), ("cf32", cast(c("cf32"), I32))]
        return self._exprs

    # (name, {column: poison value}, the model's error kind)
    POISONS = [
        ("x / 0", {"den": 0}, M.DIVIDE_BY_ZERO),
        ("MIN / -1", {"num": -(1 << 63), "den": -1}, M.ARITH_OVERFLOW),
        ("Int64 2^31 -> Int32", {"ci": 1 << 31}, M.CAST_OVERFLOW),
        ("Float64 2^63 -> Int64", {"cf": float(1 << 63)}, M.CAST_OVERFLOW),                           # defect 3
        ("Float64 below -2^63 -> Int64", {"cf": below(-float(1 << 63))}, M.CAST_OVERFLOW),
        ("NaN -> Int64", {"cf": NAN}, M.CAST_OVERFLOW),
        ("inf -> Int64", {"cf": INF}, M.CAST_OVERFLOW),
        ("Float64 2^64 -> UInt64", {"cu": float(1 << 64)}, M.CAST_OVERFLOW),                          # defect 3
        ("Float64 -1 -> UInt64", {"cu": -1.0}, M.CAST_OVERFLOW),
        ("Int64 10^18 -> Decimal128(38, 30)", {"cid": 10 ** 18}, M.CAST_OVERFLOW),                     # defect 2: the product wraps into range
        ("Int64 10^8 -> Decimal128(38, 30)", {"cid": 10 ** 8}, M.CAST_OVERFLOW),                       # (the plain precision overflow)
        ("Decimal128(38, 0) 10^30 -> (38, 9)", {"cdd": 10 ** 30}, M.CAST_OVERFLOW),                    # defect 2
        ("Decimal128(38, 0) -10^29 -> (38, 9)", {"cdd": -10 ** 29}, M.CAST_OVERFLOW),
        ("Decimal128(9, 2) 9999999.99 -> (7, 0) rounds to 10^7", {"cdn": 999999950}, M.CAST_OVERFLOW),
        ("Decimal128(18, 4) 2^31 -> Int32", {"cdi": (1 << 31) * 10 ** 4}, M.CAST_OVERFLOW),
        ("Float64 above 10^23 -> Decimal128(23, 0)", {"cfd": above(float(10 ** 23))}, M.CAST_OVERFLOW),
        ("inf -> Decimal128(23, 0)", {"cfd": INF}, M.CAST_OVERFLOW),
        ("NaN -> Decimal128(23, 0)", {"cfd": NAN}, M.CAST_OVERFLOW),
        ("Float64 2^31 -> Int32", {"cf32": float(1 << 31)}, M.CAST_OVERFLOW),
    ]

    def case(self, pname=None, row=None, mode="live"):
        """(columns as the model sees them, RecordBatch) with POISONS[pname] at `row`; cached, never modified.
        mode: "live" (the poisoned row is valid and passes the filter), "null" (the poison lies under a NULL, in the values
        buffer), "rejected" (the row's g is 0: the fused filter g > 0 rejects it). No pname: the harmless table."""
        key = (pname, row, mode if pname else "live")
        if key in self._cases:
            return self._cases[key]
        if self._base_arrays is None:
            self._base_arrays = [M.to_arrow(t, v, g) for t, v, g in zip(self.types, self.base, self.garbage)]
        cols, arrays = [M.Value(t, v) for t, v in zip(self.types, self.base)], list(self._base_arrays)
        if pname is not None:
            poison = next(p for n, p, _ in self.POISONS if n == pname)
            changed = dict(poison)
            if mode == "rejected":
                changed["g"] = 0
            for name, v in changed.items():
                k = self.names.index(name)
                vals = list(self.base[k])
                under = None
                if mode == "null" and name != "g":
                    vals[row], under = None, {row: v}
                else:
                    vals[row] = v
                cols[k] = M.Value(self.types[k], vals)
                arrays[k] = M.to_arrow(self.types[k], vals, self.garbage[k], under)
        self._cases[key] = (cols, pa.RecordBatch.from_arrays(arrays, schema=self.schema))
        return self._cases[key]

    def filter(self):
        if self._filter is None:
            self._filter = b(self.c("g"), Op.Gt, lit(I64, 0))
        return self._filter


_ERR = []


def error_table() -> ErrorTable:
    if not _ERR:
        _ERR.append(ErrorTable())
    return _ERR[0]
