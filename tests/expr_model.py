"""An exact model of the expression semantics, independent of the oracle (oracle/qoracle.c) and of the kernels.

It states what the reference's physical/expr/{binary,cast,negative,case,is_null}.rs compute on arrow-rs (`CastOptions { safe:
false }`), in plain Python over lists of None / int / float / bool with a pyarrow DataType as the type tag:

  * Python integers carry every integer, date and decimal value (a Decimal128 is its unscaled integer);
  * `struct` is used only to round a value to Float32 / to take the bits of a float;
  * evaluate() returns a Value (type, list of values) or an error kind: DIVIDE_BY_ZERO, ARITH_OVERFLOW, CAST_OVERFLOW.

What it models
  casts       int -> int: error outside the target range.  Date32 -> Date64: * 86 400 000; Date64 -> Date32: / 86 400 000,
              truncating (the quotient is NOT range-checked here: arrow-rs wraps, the oracle raises; no vector leaves Int32).
              int -> float: ONE round-to-nearest-even (Int64 -> Float32 does not go through Float64).
              float -> int: truncation toward zero; legal exactly for -2^(b-1) <= trunc(x) < 2^(b-1) (signed) and
              0 <= trunc(x) < 2^b (unsigned), as num::cast has it: 2^63 and 2^64 themselves are errors; NaN is an error.
              int -> decimal(p, s) and decimal upscale by k: checked multiply, then |v| < 10^p. Both together are exactly
              |value| < 10^(p - k) (value == 0 when p <= k).
              decimal downscale: round half away from zero, then the precision check.  decimal -> int: truncating division,
              then the range check.  decimal -> float: (double)v / 10^scale (then narrowed to Float32, if asked).
              float -> decimal(p, s): round_half_away(x * 10^s) in Float64, converted to an integer, |v| < 10^p checked ON THE
              INTEGER (float(10**23) < 10^23 is a legal Decimal128(23, 0)).  bool -> int: 1 / 0.
  integers    + - * and unary minus wrap to the type's width; / and % are checked (DivideByZero; MIN / -1: ArithOverflow) and
              evaluated on valid rows only.
  decimals    + - * with the result types of csrc/expr.cpp (binary.rs); / runs in Float64.
  floats      + - * / in the type's own precision, % is fmod; comparisons in IEEE total order (-NaN < -inf < -0.0 < +0.0 < inf < NaN).
  logic       Kleene AND / OR, IS [NOT] NULL, IF as arrow `zip`: both sides are evaluated for every row, so both can raise.
  garbage     what lies under a NULL never raises: a fallible operation looks at valid rows only.

Where it is NOT authoritative (no test vector goes there, asserted where it can be)
  * a float cast involving 10^scale with scale > 22: 10^scale is then not exact in a double, and arrow-rs's `powi` and a
    decimal literal of the kernels may differ in the last bit;
  * Decimal128 + - * whose exact result leaves i128 (divergence (5): the kernels wrap silently);
  * a NaN that an operation GENERATES (0/0, inf - inf, fmod(x, 0)): IEEE 754 leaves its sign to the implementation. NaNs that
    are passed through, negated or narrowed are bit-exact and are modelled;
  * signed MIN % -1: kernels and oracle return 0 and so does the model. DOUBT: Rust's `checked_rem` returns None there, so
    arrow-rs's `mod_checked` probably reports an overflow; there is no arrow-rs source at hand to settle it.
"""
from __future__ import annotations

import math
import struct
from typing import List, NamedTuple, Optional, Sequence, Union

import pyarrow as pa

import qurious_amd as q
from qurious_amd import Operator

DIVIDE_BY_ZERO, ARITH_OVERFLOW, CAST_OVERFLOW = "DivideByZero", "ArithOverflow", "CastOverflow"
# what the product reports for each kind (csrc/ctx.cpp)
MESSAGE = {DIVIDE_BY_ZERO: "Divide by zero", ARITH_OVERFLOW: "Arithmetic overflow", CAST_OVERFLOW: "Cast error"}
MS_PER_DAY = 86_400_000


class Value(NamedTuple):
    type: pa.DataType
    values: list


class _Raise(Exception):
    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


# ---------------------------------------------------------------------------------------------------------------- types
def is_int(t) -> bool:
    return pa.types.is_integer(t) or pa.types.is_date(t)


def is_float(t) -> bool:
    return pa.types.is_floating(t)


def is_dec(t) -> bool:
    return pa.types.is_decimal128(t)


def int_bits(t) -> int:
    return 32 if pa.types.is_date32(t) else 64 if pa.types.is_date64(t) else t.bit_width


def is_signed(t) -> bool:
    return pa.types.is_date(t) or pa.types.is_signed_integer(t)


def int_range(t):
    b = int_bits(t)
    return (-(1 << (b - 1)), (1 << (b - 1)) - 1) if is_signed(t) else (0, (1 << b) - 1)


def wrap(t, v: int) -> int:
    b = int_bits(t)
    v &= (1 << b) - 1
    return v - (1 << b) if is_signed(t) and v >> (b - 1) else v


# --------------------------------------------------------------------------------------------------------------- floats
def f32(x: float) -> float:
    """x rounded to Float32 (round to nearest even; overflow gives an infinity), as a Python float"""
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def int_to_f32(v: int) -> float:
    """ONE round-to-nearest-even of an integer to Float32"""
    a = abs(v)
    shift = a.bit_length() - 24
    if shift > 0:
        qt, rem, half = a >> shift, a & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (qt & 1)):
            qt += 1
        a = qt << shift
    return float(-a if v < 0 else a)   # (24 significant bits: exact in a double)


def float_bits(t, x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0] if pa.types.is_float32(t) else struct.unpack("<Q", struct.pack("<d", x))[0]


def total_order_key(x: float) -> int:
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def round_half_away(x: float) -> float:
    """C round()"""
    if math.isnan(x) or math.isinf(x):
        return x
    fl = math.floor(abs(x))
    r = fl + 1.0 if abs(x) - fl >= 0.5 else fl
    return math.copysign(r, x)


def _fdiv(a: float, b: float) -> float:
    if b == 0.0:
        if a == 0.0 or math.isnan(a):
            return math.nan   # (generated NaN: sign not modelled)
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _pow10_float(scale: int) -> float:
    assert 0 <= scale <= 22, "the model is authoritative only while 10^scale is exact in a double"
    return float(10 ** scale)


def _in_i128(v: int) -> int:
    assert -(1 << 127) <= v < (1 << 127), "decimal arithmetic left i128: outside the model (DESIGN.md section 4, divergence (5))"
    return v


# ---------------------------------------------------------------------------------------------------------------- casts
def cast_value(frm, to, v):
    """one valid value; raises _Raise(CAST_OVERFLOW)"""
    if frm == to:
        return v
    if pa.types.is_boolean(frm):
        assert is_int(to)
        return 1 if v else 0
    if is_int(frm) and is_int(to):
        if pa.types.is_date32(frm) and pa.types.is_date64(to):
            return v * MS_PER_DAY
        if pa.types.is_date64(frm) and pa.types.is_date32(to):
            r = abs(v) // MS_PER_DAY
            r = -r if v < 0 else r
            assert int_range(to)[0] <= r <= int_range(to)[1], "Date64 -> Date32 outside Int32: not modelled"
            return r
        lo, hi = int_range(to)
        if not lo <= v <= hi:
            raise _Raise(CAST_OVERFLOW)
        return v
    if is_int(frm) and is_float(to):
        return int_to_f32(v) if pa.types.is_float32(to) else float(v)   # (float(int) is correctly rounded)
    if is_float(frm) and is_float(to):
        return f32(v) if pa.types.is_float32(to) else v
    if is_float(frm) and is_int(to):
        if math.isnan(v) or math.isinf(v):
            raise _Raise(CAST_OVERFLOW)
        t = int(v)   # truncates toward zero, exact
        lo, hi = int_range(to)
        if not lo <= t <= hi:   # i.e. lo <= trunc(x) < 2^bits
            raise _Raise(CAST_OVERFLOW)
        return t
    if is_int(frm) and is_dec(to):
        return _scaled(v, to.scale, to.precision)
    if is_dec(frm) and is_dec(to):
        if to.scale >= frm.scale:
            return _scaled(v, to.scale - frm.scale, to.precision)
        d = 10 ** (frm.scale - to.scale)
        a = abs(v)
        r = a // d + (1 if 2 * (a % d) >= d else 0)   # half away from zero
        r = -r if v < 0 else r
        if abs(r) >= 10 ** to.precision:
            raise _Raise(CAST_OVERFLOW)
        return r
    if is_dec(frm) and is_float(to):
        x = float(v) / _pow10_float(frm.scale)
        return f32(x) if pa.types.is_float32(to) else x
    if is_dec(frm) and is_int(to):
        r = abs(v) // 10 ** frm.scale
        r = -r if v < 0 else r
        lo, hi = int_range(to)
        if not lo <= r <= hi:
            raise _Raise(CAST_OVERFLOW)
        return r
    if is_float(frm) and is_dec(to):
        x = round_half_away(v * _pow10_float(to.scale))
        if math.isnan(x) or math.isinf(x):
            raise _Raise(CAST_OVERFLOW)
        r = int(x)
        if abs(r) >= 10 ** to.precision:   # on the integer: the double nearest to 10^p may be below 10^p
            raise _Raise(CAST_OVERFLOW)
        return r
    raise NotImplementedError(f"model: cast {frm} -> {to}")


def _scaled(v: int, k: int, precision: int) -> int:
    # checked multiply (|v * 10^k| < 2^127) and |v * 10^k| < 10^precision <= 10^38 < 2^127: the second implies the first
    r = v * 10 ** k
    if abs(r) >= 10 ** precision:
        raise _Raise(CAST_OVERFLOW)
    return r


# ----------------------------------------------------------------------------------------------------------- arithmetic
def decimal_result_type(op, lt, rt):
    """csrc/expr.cpp (binary.rs): the result type of Decimal128 + - *"""
    p1, s1, p2, s2 = lt.precision, lt.scale, rt.precision, rt.scale
    if op in (Operator.Add, Operator.Sub):
        s = max(s1, s2)
        return pa.decimal128(min(38, max(p1 - s1, p2 - s2) + s + 1), s)
    assert op == Operator.Mul and s1 + s2 <= 38
    return pa.decimal128(min(38, p1 + p2 + 1), s1 + s2)


def _to_f64(t, v) -> float:
    return float(v) / _pow10_float(t.scale) if is_dec(t) else float(v)


def _arith(op, lt, rt):
    """(result type, function of two valid values)"""
    if is_dec(lt) or is_dec(rt):
        if op == Operator.Div:
            return pa.float64(), lambda x, y: _fdiv(_to_f64(lt, x), _to_f64(rt, y))
        assert is_dec(lt) and is_dec(rt)
        t = decimal_result_type(op, lt, rt)
        if op == Operator.Mul:
            return t, lambda x, y: _in_i128(x * y)
        ml, mr = 10 ** (t.scale - lt.scale), 10 ** (t.scale - rt.scale)
        if op == Operator.Add:
            return t, lambda x, y: _in_i128(_in_i128(x * ml) + _in_i128(y * mr))
        return t, lambda x, y: _in_i128(_in_i128(x * ml) - _in_i128(y * mr))
    assert lt == rt, (lt, rt)
    if is_float(lt):
        rnd = f32 if pa.types.is_float32(lt) else (lambda x: x)
        if op == Operator.Add:
            return lt, lambda x, y: rnd(x + y)
        if op == Operator.Sub:
            return lt, lambda x, y: rnd(x - y)
        if op == Operator.Mul:
            return lt, lambda x, y: rnd(x * y)
        if op == Operator.Div:
            return lt, lambda x, y: rnd(_fdiv(x, y))
        return lt, lambda x, y: math.nan if (y == 0.0 or math.isinf(x) or math.isnan(x) or math.isnan(y)) else math.fmod(x, y)
    assert pa.types.is_integer(lt)
    lo, hi = int_range(lt)
    if op == Operator.Add:
        return lt, lambda x, y: wrap(lt, x + y)
    if op == Operator.Sub:
        return lt, lambda x, y: wrap(lt, x - y)
    if op == Operator.Mul:
        return lt, lambda x, y: wrap(lt, x * y)

    def divmod_checked(x, y):
        if y == 0:
            raise _Raise(DIVIDE_BY_ZERO)
        if op == Operator.Div:
            r = abs(x) // abs(y)
            r = -r if (x < 0) != (y < 0) else r
            if not lo <= r <= hi:   # signed MIN / -1
                raise _Raise(ARITH_OVERFLOW)
            return r
        if y == -1:
            return 0   # DOUBT (module docstring): MIN % -1 is 0 today; arrow-rs's mod_checked probably reports an overflow
        r = abs(x) % abs(y)
        return -r if x < 0 else r   # the sign of the dividend
    return lt, divmod_checked


def _compare(op, t, a, b) -> bool:
    if is_float(t):
        a, b = total_order_key(a), total_order_key(b)
    elif pa.types.is_boolean(t):
        a, b = int(a), int(b)
    return {Operator.Eq: a == b, Operator.NotEq: a != b, Operator.Gt: a > b, Operator.GtEq: a >= b, Operator.Lt: a < b, Operator.LtEq: a <= b}[op]


# ------------------------------------------------------------------------------------------------------------ evaluation
def _eval(e, cols: Sequence[Value], n: int, rec=None) -> Value:
    """`rec` evaluates a child (Memo passes one that remembers)"""
    if rec is None:
        def rec(x):
            return _eval(x, cols, n)
    if isinstance(e, q.Column):
        return cols[e.index]
    if isinstance(e, q.Literal):
        t, v = e.value.dtype, e.value.value
        if v is not None and is_float(t):
            v = f32(float(v)) if pa.types.is_float32(t) else float(v)
        return Value(t, [v] * n)
    if isinstance(e, q.CastExpr):
        c = rec(e.expr)
        return Value(e.data_type, [None if v is None else cast_value(c.type, e.data_type, v) for v in c.values])
    if isinstance(e, q.IsNull):
        return Value(pa.bool_(), [v is None for v in rec(e.expr).values])
    if isinstance(e, q.IsNotNull):
        return Value(pa.bool_(), [v is not None for v in rec(e.expr).values])
    if isinstance(e, q.Negative):
        c = rec(e.expr)
        if is_float(c.type):
            return Value(c.type, [None if v is None else -v for v in c.values])
        if is_dec(c.type):
            return Value(c.type, [None if v is None else _in_i128(-v) for v in c.values])
        return Value(c.type, [None if v is None else wrap(c.type, -v) for v in c.values])
    if isinstance(e, q.CaseExpr):
        acc = rec(e.else_expr)
        for when, then in reversed(e.when_then):   # nested zip(mask, truthy, falsy); every branch is evaluated in full
            m, t = rec(when), rec(then)
            assert pa.types.is_boolean(m.type) and t.type == acc.type
            acc = Value(t.type, [tv if mv else fv for mv, tv, fv in zip(m.values, t.values, acc.values)])
        return acc
    assert isinstance(e, q.BinaryExpr), type(e)
    l, r = rec(e.left), rec(e.right)
    op = e.op
    if op in (Operator.And, Operator.Or):
        absorbing = op == Operator.Or
        out = []
        for a, b in zip(l.values, r.values):
            if a is not None and b is not None:
                out.append((a or b) if absorbing else (a and b))
            elif (a is not None and a == absorbing) or (b is not None and b == absorbing):
                out.append(absorbing)   # false AND NULL = false, true OR NULL = true
            else:
                out.append(None)
        return Value(pa.bool_(), out)
    if op <= Operator.LtEq:
        assert l.type == r.type, (l.type, r.type)
        return Value(pa.bool_(), [None if a is None or b is None else _compare(op, l.type, a, b) for a, b in zip(l.values, r.values)])
    t, fn = _arith(op, l.type, r.type)
    return Value(t, [None if a is None or b is None else fn(a, b) for a, b in zip(l.values, r.values)])


def evaluate(expr, cols: Sequence[Value]) -> Union[Value, str]:
    """the expression over the columns: a Value, or the error kind the evaluation ends with"""
    n = len(cols[0].values) if cols else 1
    try:
        return _eval(expr, cols, n)
    except _Raise as r:
        return r.kind


def keep_rows(cols: Sequence[Value], mask: Value) -> List[Value]:
    """Filter / a scan's filter: the rows whose mask is valid and true"""
    return [Value(c.type, [v for v, m in zip(c.values, mask.values) if m]) for c in cols]


def aggregate(kind: str, v: Value, groups: Optional[list] = None) -> dict:
    """{group: SUM / MIN / MAX / COUNT of the valid values} (one group `()` when `groups` is None). SUM of integers wraps to
    64 bits, of decimals to 128; floats only have MIN / MAX here: their sum depends on the order of the rows.
    Not modelled, and asserted: MIN / MAX over a NaN or of a group without any valid value. There the reference's accumulators
    (aggregate/{min,max}.rs: PartialOrd against the type's extreme value) answer neither NaN nor NULL; no vector goes there."""
    out = {}
    for k, x in enumerate(v.values):
        g = () if groups is None else groups[k]
        cur = out.setdefault(g, 0 if kind == "count" else None)
        if x is None:
            continue
        if kind == "count":
            out[g] = cur + 1
        elif kind == "sum":
            assert not is_float(v.type)
            s = (cur or 0) + x
            out[g] = wrap(v.type, s) if is_int(v.type) else ((s + (1 << 127)) % (1 << 128)) - (1 << 127)
        else:
            assert not (is_float(v.type) and math.isnan(x)), "MIN / MAX over NaN is not modelled"
            key = total_order_key if is_float(v.type) else (lambda y: y)
            better = cur is None or (key(x) < key(cur) if kind == "min" else key(x) > key(cur))
            out[g] = x if better else cur
    assert kind not in ("min", "max") or None not in out.values(), "MIN / MAX of a group without a valid value is not modelled"
    return out


def columns_read(e) -> set:
    """the column indices an expression reads"""
    if isinstance(e, q.Column):
        return {e.index}
    if isinstance(e, q.Literal):
        return set()
    if isinstance(e, q.CaseExpr):
        parts = [e.else_expr] + [x for wt in e.when_then for x in wt]
    elif isinstance(e, q.BinaryExpr):
        parts = [e.left, e.right]
    else:
        parts = [e.expr]
    return set().union(*[columns_read(x) for x in parts])


class Memo:
    """evaluate / keep_rows / aggregate remembered by the IDENTITY of the expression and of the value lists it reads: tables
    that share all but one column (the error cases) then cost one column's worth of work each. Everything seen is kept alive,
    so identities stay unique; nothing remembered is ever modified."""

    def __init__(self):
        self._memo, self._alive = {}, []

    def _get(self, key, alive, compute):
        if key not in self._memo:
            self._memo[key] = compute()
            self._alive.append(alive)
        return self._memo[key]

    def evaluate(self, expr, cols: Sequence[Value]):
        """like evaluate(); sub-expressions are remembered too"""
        n = len(cols[0].values)

        def rec(e):
            reads = [cols[k].values for k in sorted(columns_read(e))]
            key = ("e", id(e), n) + tuple(id(v) for v in reads)
            return self._get(key, (e, reads), lambda: _eval(e, cols, n, rec))   # (an error is not remembered: it propagates)
        try:
            return rec(expr)
        except _Raise as r:
            return r.kind

    def keep_rows(self, cols: Sequence[Value], mask: Value) -> List[Value]:
        return [self._get(("k", id(c.values), id(mask.values)), (c.values, mask.values), lambda c=c: keep_rows([c], mask)[0]) for c in cols]

    def aggregate(self, kind: str, v: Value, groups: Optional[list] = None) -> dict:
        return self._get(("a", kind, id(v.values), id(groups)), (v.values, groups), lambda: aggregate(kind, v, groups))


# ------------------------------------------------------------------------------------------------ arrays from / to buffers
_STRUCT = {pa.int8(): "b", pa.int16(): "h", pa.int32(): "i", pa.int64(): "q", pa.uint8(): "B", pa.uint16(): "H", pa.uint32(): "I", pa.uint64(): "Q",
           pa.float32(): "f", pa.float64(): "d", pa.date32(): "i", pa.date64(): "q"}


def to_arrow(t, values: Sequence, garbage=None, under_null: Optional[dict] = None) -> pa.Array:
    """A nullable array built FROM BUFFERS, so that a NULL slot's bytes are `garbage` (a raw value of the type: unscaled for
    a Decimal128; `under_null` = {row: raw value} overrides it for single rows) instead of the zeros a builder would leave."""
    n = len(values)
    valid = bytearray((n + 7) // 8)
    for k, v in enumerate(values):
        if v is not None:
            valid[k >> 3] |= 1 << (k & 7)
    raw = [(under_null or {}).get(k, garbage) if v is None else v for k, v in enumerate(values)]
    assert all(v is not None for v in raw), "a NULL needs a garbage value"
    if pa.types.is_boolean(t):
        data = bytearray((n + 7) // 8)
        for k, v in enumerate(raw):
            if v:
                data[k >> 3] |= 1 << (k & 7)
    elif is_dec(t):
        data = b"".join(int(v).to_bytes(16, "little", signed=True) for v in raw)
    else:
        data = struct.pack("<%d%s" % (n, _STRUCT[t]), *raw)
    nulls = sum(v is None for v in values)
    return pa.Array.from_buffers(t, n, [pa.py_buffer(bytes(valid)) if nulls else None, pa.py_buffer(bytes(data))], null_count=nulls)


def from_arrow(arr) -> Value:
    """the array's values in the model's representation, read from its buffers (unscaled decimals, raw dates, exact floats)"""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks() if arr.num_chunks != 1 else arr.chunk(0)
    t, n, off = arr.type, len(arr), arr.offset
    vb, db = arr.buffers()[0], arr.buffers()[1]
    valid = [True] * n
    if vb is not None and arr.null_count:
        bits = vb.to_pybytes()
        valid = [bool(bits[(off + k) >> 3] >> ((off + k) & 7) & 1) for k in range(n)]
    raw = db.to_pybytes()
    if pa.types.is_boolean(t):
        vals = [bool(raw[(off + k) >> 3] >> ((off + k) & 7) & 1) for k in range(n)]
    elif is_dec(t):
        vals = [int.from_bytes(raw[16 * (off + k):16 * (off + k) + 16], "little", signed=True) for k in range(n)]
    else:
        c = _STRUCT[t]
        w = struct.calcsize(c)
        vals = list(struct.unpack_from("<%d%s" % (n, c), raw, off * w))
    return Value(t, [v if ok else None for v, ok in zip(vals, valid)])


def same_values(t, got: Sequence, want: Sequence) -> Optional[str]:
    """None when equal — integers and decimals as integers, floats BIT FOR BIT (NaN and the sign of zero included) — else a
    description of the first difference"""
    if len(got) != len(want):
        return f"{len(got)} rows, expected {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        if (g is None) != (w is None):
            return f"row {k}: got {g!r}, expected {w!r}"
        if g is None:
            continue
        if is_float(t):
            if float_bits(t, g) != float_bits(t, w):
                return f"row {k}: got {g!r} ({float_bits(t, g):#x}), expected {w!r} ({float_bits(t, w):#x})"
        elif g != w:
            return f"row {k}: got {g!r}, expected {w!r}"
    return None
