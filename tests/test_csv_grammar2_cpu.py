"""Grammar level 2 of the device CSV decoder without a GPU (csrc/device/qhip_csv.inc: the quote-aware record walk, the Boolean and
Timestamp parsers, the undoubling copy's lane logic): tests/cpp/csv_grammar2_tests.cpp includes the file as plain host C++ and
decodes a file into a text dump, which is compared with `pyarrow.csv.read_csv` (column_types, default parse options) on the same
bytes. Built with g++ as a stand-alone program (nothing of it is loaded into Python), once plainly and once with the address and
undefined-behaviour sanitizers; the file and every buffer carry exactly the 64 bytes of slack a device allocation has."""
import datetime
import decimal
import io
import os
import random
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qurious_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "cpp", "csv_grammar2_tests.cpp")
FLAGS = ["-std=c++17", "-g", "-Wall", "-Werror", "-I" + CSRC]
SAN = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
BOTH = ("plain", "san")

R_LONE_CR, R_EMPTY_LINE, R_FIELD_COUNT, R_INT, R_DATE, R_DECIMAL, R_FLOAT, R_QUOTING, R_BOOL, R_TIMESTAMP = 3, 4, 5, 6, 7, 8, 9, 12, 13, 14

TS = {"s": pa.timestamp("s"), "ms": pa.timestamp("ms"), "us": pa.timestamp("us"), "ns": pa.timestamp("ns")}
DIGITS = {"s": 0, "ms": 3, "us": 6, "ns": 9}
DEC = pa.decimal128(15, 2)
TYPE_CODE = {pa.int8(): "i8", pa.int16(): "i16", pa.int32(): "i32", pa.int64(): "i64", pa.uint8(): "u8", pa.uint16(): "u16",
             pa.uint32(): "u32", pa.uint64(): "u64", pa.float64(): "f64", pa.date32(): "date", pa.string(): "utf8", pa.bool_(): "bool",
             TS["s"]: "ts0", TS["ms"]: "ts3", TS["us"]: "ts6", TS["ns"]: "ts9"}


def _code(t):
    return f"dec:{t.precision}:{t.scale}" if pa.types.is_decimal(t) else TYPE_CODE[t]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("csv_grammar2_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("csv_grammar2_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


def _finish(r):
    assert r.returncode == 0, r.stderr.decode()
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()
    return r.stdout.decode().split("\n")[:-1]


def _run(exes, which, data, types, header=True, delim=",", quote='"', proj=None):
    path = str(exes["dir"] / "in.csv")
    with open(path, "wb") as f:
        f.write(data)
    args = [exes[which], "decode", path, ",".join(_code(t) for t in types), "1" if header else "0", str(ord(delim)), str(ord(quote) if quote else -1),
            ",".join(map(str, proj)) if proj else "-"]
    return _finish(subprocess.run(args, capture_output=True))


def _host(data, names, types, include=None):
    conv = pacsv.ConvertOptions(column_types=dict(zip(names, types)), include_columns=include)
    return pacsv.read_csv(io.BytesIO(data), convert_options=conv)


def _cell(v, t):
    if v is None:
        return "N"
    if pa.types.is_float64(t):
        return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]
    if pa.types.is_date32(t):
        return str((v - datetime.date(1970, 1, 1)).days)
    if pa.types.is_decimal(t):
        return str(int(v.scaleb(t.scale, context=decimal.Context(prec=100))))
    if pa.types.is_string(t):
        return "s" + v.encode().hex()
    if pa.types.is_boolean(t):
        return "1" if v else "0"
    return str(v)


def _expect(tbl):
    cols = []
    for c, f in zip(tbl.columns, tbl.schema):
        if pa.types.is_timestamp(f.type):
            c = c.cast(pa.int64())
        cols.append([_cell(v, f.type) for v in c.to_pylist()])
    return ["ROWS %d" % tbl.num_rows] + ["\t".join(r) for r in zip(*cols)]


def _check(exes, data, names, types, which=BOTH):
    want = _expect(_host(data, names, types))
    for w in which:
        assert _run(exes, w, data, types) == want
    return want


def _needs_host(exes, data, types, reason, record, **kw):
    for w in BOTH:
        assert _run(exes, w, data, types, **kw) == ["NEEDS_HOST %d %d" % (reason, record)], data


def test_the_undoubling_copy_against_a_byte_serial_one(exes):
    """runs of 1..130 quotes at every offset 0..129, through the 64-byte steps with a simulated ballot"""
    for w in BOTH:
        assert _finish(subprocess.run([exes[w], "undouble"], capture_output=True)) == ["UNDOUBLE OK %d" % (130 * 130)]


def test_quoted_spellings(exes):
    names, types = ["s", "i", "d", "m", "f", "u"], [pa.string(), pa.int32(), pa.date32(), DEC, pa.float64(), pa.string()]
    rows = ['"a,b","1","1995-03-15","-.5","1.5",x', '"a""b","-5",1995-03-15,"1",2.5,"y"', '"""",7,"0001-01-01",.5,"-0.0",""""""',
            '"","","","","",""', ',,,,,', 'plain,"007","9999-12-31","5.","1e3","tab\there, ä€\U0001f600 ""q"""']
    for end in ("\n", "\r\n"):
        data = (",".join(names) + "\n" + end.join(rows) + end).encode()
        want = _check(exes, data, names, types)
        assert want[1].split("\t")[0] == "s" + b"a,b".hex() and want[2].split("\t")[0] == "s" + b'a"b'.hex()
        assert want[3].split("\t")[0] == "s" + b'"'.hex() and want[3].split("\t")[5] == "s" + b'""'.hex()
        assert want[4] == "s\tN\tN\tN\tN\ts" and want[5] == "s\tN\tN\tN\tN\ts"      # "" is NULL but for Utf8, where it is the empty string
    # the quoted header Arrow's writer produces; another delimiter and quote
    data = b'"s","i"\n"x",1\n'
    _check(exes, data, ["s", "i"], [pa.string(), pa.int32()])
    for w in BOTH:
        assert _run(exes, w, b"s|i\n'a|''b'|'3'\n", [pa.string(), pa.int32()], delim="|", quote="'") == ["ROWS 1", "s" + b"a|'b".hex() + "\t3"]
        assert _run(exes, w, b's,i\n"a,3\n', [pa.string(), pa.int32()], quote=None) == ["ROWS 1", "s" + b'"a'.hex() + "\t3"]   # no byte is a quote
    # a quoted field is parsed by the same strict grammar: what needs the host unquoted needs it quoted
    for t, text, reason in ((pa.int32(), '" 1"', R_INT), (pa.int32(), '"+1"', R_INT), (pa.int32(), '"1""2"', R_INT), (pa.date32(), '"1995-3-15"', R_DATE),
                            (DEC, '"1e2"', R_DECIMAL), (pa.float64(), '" 1"', R_FLOAT), (pa.float64(), '"1"""', R_FLOAT)):
        _needs_host(exes, ("k,v\n1,\n2,%s\n" % text).encode(), [pa.int32(), t], reason, 2)


NON_CANONICAL = {"inside": 'ab"c', "behind": '"ab"c', "twice": '"ab"c"d"', "open": '"abc', "odd": '"a"b"', "lone": '"'}


def test_non_canonical_quoting_in_projected_and_unprojected_fields(exes):
    types = [pa.int32(), pa.string(), pa.int32()]
    for what, text in NON_CANONICAL.items():
        for end in ("\n", ""):
            for field in (1, 2):     # in the middle of a record and as its last field
                row = ["2", "ok", "5"]
                row[field] = text
                data = ("a,b,c\n1,x,3\n%s%s" % (",".join(row), end)).encode()
                _needs_host(exes, data, types, R_QUOTING, 2)                       # projected
                _needs_host(exes, data, types, R_QUOTING, 2, proj=[0])             # unprojected: the structure depends on it
    # Arrow reads these leniently (a value, not an error): the device does not imitate that
    assert _host(b'a,b\n1,ab"c\n', ["a", "b"], [pa.int32(), pa.string()]).column("b").to_pylist() == ['ab"c']


def test_line_ends_inside_quotes(exes):
    two = [pa.int32(), pa.string()]
    _needs_host(exes, b'k,v\n1,a\n2,"b\nc"\n3,d\n', two, R_QUOTING, 2)       # the record is cut: its first piece has no closing quote
    _needs_host(exes, b'k,v\n1,a\n2,"b\r\nc"\n3,d\n', two, R_QUOTING, 2)
    _needs_host(exes, b'k,v\n1,a\n2,"b""\nc"\n3,d\n', two, R_QUOTING, 2)     # ("" in front of the cut is a pair, not a closing quote)
    _needs_host(exes, b'k,v\n1,a\n2,"b\nc"\n', two, R_QUOTING, 2, proj=[0])
    _needs_host(exes, b'k,v\n1,"a\rb"\n', two, R_LONE_CR, 1)                   # a lone '\r' keeps its reason, inside quotes or not
    _needs_host(exes, b'k,v\n1,a\rb\n', two, R_LONE_CR, 1)
    _needs_host(exes, b'k,v\n1,"a\n\nb"\n', two, R_EMPTY_LINE, 2)


KINDS = ("plain", "quoted", "delims", "pairs")


def _rand_field(rng, t, kind):
    if pa.types.is_string(t):
        base = rng.choice(["", "a", "xy", "hello world", "ä€\U0001f600", "x" * rng.randint(60, 70), "nul\x00byte"])
        if kind == "delims":
            base = rng.choice([",", base + ",", "," + base + ",,"])
        if kind == "pairs":
            base = rng.choice(['"', '""', base + '"', '"' + base, base[:1] + '"' * rng.randint(1, 5) + base[1:]])
    elif pa.types.is_int32(t):
        base = rng.choice(["", "0", "-17", "2147483647", str(rng.randint(-10 ** 6, 10 ** 6))])
    elif pa.types.is_date32(t):
        base = rng.choice(["", datetime.date.fromordinal(rng.randint(1, 3652059)).isoformat()])
    elif pa.types.is_boolean(t):
        base = rng.choice(["", "true", "false"])
    elif pa.types.is_timestamp(t):
        base = rng.choice(["", "1995-03-15 12:34:56", "2024-02-29T23:59:59.5", "1970-01-01 00:00:00.000001"])
    else:
        base = rng.choice(["", "1.5", "-.5", "12", "%d.%02d" % (rng.randint(0, 10 ** 6), rng.randint(0, 99))])
    if kind == "plain":
        return base
    return '"' + base.replace('"', '""') + '"'


def test_random_records_of_plain_and_quoted_fields(exes):
    names = ["s", "i", "d", "b", "t", "m", "u"]
    types = [pa.string(), pa.int32(), pa.date32(), pa.bool_(), TS["us"], DEC, pa.string()]
    rng = random.Random(20260202)
    seen = dict.fromkeys(KINDS, 0)
    recs = []
    for _ in range(3000):
        row = []
        for t in types:
            kind = rng.choice(KINDS if pa.types.is_string(t) else KINDS[:2])
            seen[kind] += 1
            row.append(_rand_field(rng, t, kind))
        recs.append(",".join(row))
    assert all(seen[k] > 0 for k in KINDS), seen
    data = (",".join(names) + "\n" + "".join(r + rng.choice(["\n", "\r\n"]) for r in recs)).encode()
    _check(exes, data, names, types)
    # a projection: the unprojected fields are walked (quotes, delimiters inside) but not parsed
    want = _expect(_host(data, names, types, include=["u", "b", "i"]))
    for w in BOTH:
        assert _run(exes, w, data, types, proj=[6, 3, 1]) == want
    # every way of leaving the canonical form, at a random field of a random record
    left = dict.fromkeys(NON_CANONICAL, 0)
    for what, text in NON_CANONICAL.items():
        for _ in range(5):
            r, f = rng.randrange(len(recs)), rng.choice([0, 6])
            fields = ["x", "1", "1995-03-15", "true", "", "1.5", "y"]
            fields[f] = text
            bad = list(recs)
            bad[r] = ",".join(fields)
            bdata = (",".join(names) + "\n" + "\n".join(bad) + "\n").encode()
            assert _run(exes, "plain", bdata, types) == ["NEEDS_HOST %d %d" % (R_QUOTING, r + 1)], (what, r, f)
            assert _run(exes, "plain", bdata, types, proj=[1]) == ["NEEDS_HOST %d %d" % (R_QUOTING, r + 1)], (what, r, f)
            left[what] += 1
    assert all(left.values())


def test_the_empty_quoted_field_of_every_type(exes):
    types = [pa.int8(), pa.int64(), pa.uint64(), pa.float64(), pa.date32(), DEC, pa.bool_(), TS["s"], TS["ms"], TS["us"], TS["ns"], pa.string()]
    names = ["c%d" % k for k in range(len(types))]
    data = (",".join(names) + "\n" + ",".join(['""'] * len(types)) + "\n" + ",".join([""] * len(types)) + "\n").encode()
    want = _check(exes, data, names, types)
    assert want[1:] == ["\t".join(["N"] * (len(types) - 1) + ["s"])] * 2


def test_boolean_spellings(exes):
    data = b'k,b\n1,true\n2,false\n3,\n4,"true"\n5,"false"\n6,""\n'
    assert _check(exes, data, ["k", "b"], [pa.int32(), pa.bool_()])[1:] == ["1\t1", "2\t0", "3\tN", "4\t1", "5\t0", "6\tN"]
    # Arrow accepts more spellings (True, FALSE, 0, 1): those go to the host, with everything it refuses
    for text in ("True", "FALSE", "TRUE", "False", "0", "1", "t", "f", "yes", "no", " true", "true ", "tru", "truee", "falsE", "NULL", '"t""rue"'):
        _needs_host(exes, ("k,b\n1,true\n2,%s\n" % text).encode(), [pa.int32(), pa.bool_()], R_BOOL, 2)
    for text in ("True", "FALSE", "0", "1"):
        assert _host(("b\n%s\n" % text).encode(), ["b"], [pa.bool_()]).column(0).to_pylist() == [text in ("True", "1")]


def _ts_text(dt, frac_digits, frac, sep):
    s = "%04d-%02d-%02d%s%02d:%02d:%02d" % (dt.year, dt.month, dt.day, sep, dt.hour, dt.minute, dt.second)
    return s + ("." + ("%09d" % frac)[:frac_digits] if frac_digits else "")


EPOCH = datetime.datetime(1970, 1, 1)


def _units(dt, frac_digits, frac, unit):
    """the int64 a timestamp spelled by _ts_text stands for (frac: nanoseconds, of which frac_digits digits are written)"""
    secs = (dt - EPOCH).days * 86400 + (dt - EPOCH).seconds
    kept = int(("%09d" % frac)[:frac_digits].ljust(9, "0")) if frac_digits else 0
    return secs * 10 ** DIGITS[unit] + kept // 10 ** (9 - DIGITS[unit])


@pytest.mark.parametrize("unit", list(TS))
def test_timestamps_at_the_edges_of_the_range(exes, unit):
    k = DIGITS[unit]
    years = (1, 9999) if unit != "ns" else (1678, 2261)
    texts, want = [], []
    for y in years:
        for dt in (datetime.datetime(y, 1, 1, 0, 0, 0), datetime.datetime(y, 12, 31, 23, 59, 59)):
            for sep in " T":
                for fd in sorted({0, 1, k} if k else {0}):
                    frac = 999_999_999 if dt.month == 12 else 0
                    texts.append(_ts_text(dt, fd, frac, sep))
                    want.append(_units(dt, fd, frac, unit))
    # every day boundary of a leap year and of a year that is none
    for y in (2024, 1900):
        d = datetime.datetime(y, 1, 1)
        while d.year == y:
            texts += [_ts_text(d, 0, 0, " "), _ts_text(d + datetime.timedelta(seconds=86399), 0, 0, "T")]
            want += [_units(d, 0, 0, unit), _units(d, 0, 0, unit) + 86399 * 10 ** k]
            d += datetime.timedelta(days=1)
    if unit == "ns":
        # both ends as Arrow C++ 25 has them: int64 would reach down to 1677-09-21T00:12:43.145224192, but Arrow refuses every
        # instant whose whole seconds (here -9223372037) do not fit as nanoseconds, and its answer is the yardstick
        texts += ["1677-09-21T00:12:44", "1677-09-21T00:12:44.000000001", "2262-04-11T23:47:16.854775807", "2262-04-11 23:47:16"]
        want += [-9223372036 * 10 ** 9, -9223372036 * 10 ** 9 + 1, 2 ** 63 - 1, 9223372036 * 10 ** 9]
    data = ("t\n" + "\n".join(texts) + "\n").encode()
    got = _check(exes, data, ["t"], [TS[unit]])
    assert [int(x) for x in got[1:]] == want
    if unit == "ns":     # one step outside either end: Arrow errors, the device needs the host
        for text in ("1677-09-21T00:12:43.999999999", "1677-09-21T00:12:43.145224192", "1677-09-21T00:12:43.145224191", "2262-04-11T23:47:16.854775808",
                     "1677-09-21 00:12:43", "2262-04-11 23:47:17", "0001-01-01 00:00:00",
                     "9999-12-31 23:59:59"):
            _needs_host(exes, ("t\n%s\n" % text).encode(), [TS[unit]], R_TIMESTAMP, 1)
            with pytest.raises(pa.ArrowInvalid):
                _host(("t\n%s\n" % text).encode(), ["t"], [TS[unit]])


@pytest.mark.parametrize("unit", list(TS))
def test_a_hundred_thousand_random_instants(exes, unit):
    rng = random.Random(DIGITS[unit] + 77)
    lo, hi = (datetime.datetime(1, 1, 1), datetime.datetime(9999, 12, 31, 23, 59, 59)) if unit != "ns" else \
        (datetime.datetime(1677, 9, 22), datetime.datetime(2262, 4, 11))
    span = int((hi - lo).total_seconds())
    texts, want = [], np.empty(100_000, dtype=np.int64)
    for i in range(100_000):
        dt = lo + datetime.timedelta(seconds=rng.randint(0, span))
        fd, frac = rng.randint(0, DIGITS[unit]), rng.randint(0, 999_999_999)
        texts.append(_ts_text(dt, fd, frac, rng.choice(" T")))
        want[i] = _units(dt, fd, frac, unit)
    data = ("t\n" + "\n".join(texts) + "\n").encode()
    got = _run(exes, "plain", data, [TS[unit]])
    assert got[0] == "ROWS 100000"
    assert np.array_equal(np.array(got[1:], dtype=np.int64), want)
    host = _host(data, ["t"], [TS[unit]]).column(0).combine_chunks().cast(pa.int64()).to_numpy()
    assert np.array_equal(host, want)
    small = ("t\n" + "\n".join(texts[:5000]) + "\n").encode()     # ... a smaller sample under the sanitizers
    assert [int(x) for x in _run(exes, "san", small, [TS[unit]])[1:]] == want[:5000].tolist()


# spellings Arrow accepts but the strict grammar leaves to the host, and spellings Arrow refuses: the errors belong to the host
TS_LENIENT = ["1995-03-15", "1995-03-15 01:02", "1995-03-15T01", "1995-03-15 1:02:03"]
TS_REFUSED = ["1995-03-15 01:02:03Z", "1995-03-15 01:02:03+01:00", "1995-03-15 24:00:00", "1995-03-15 23:59:60", "1995-03-15 23:60:00",
              "1995-02-30 00:00:00", "0000-01-01 00:00:00", "1995-03-15  01:02:03", "1995-03-15t01:02:03", "1995-03-15 01:02:03.", "1995-03-15 01-02-03",
              "1995-03-15 01:02:03 ", " 1995-03-15 01:02:03", "1995-03-15 01:02:0x", "1995-03-15 01:02:03,5", "NULL", "1995-03-15 01:02:03.5.5"]


@pytest.mark.parametrize("unit", list(TS))
def test_timestamp_spellings_that_need_the_host(exes, unit):
    k = DIGITS[unit]
    texts = TS_LENIENT + [t for t in TS_REFUSED if "," not in t] + ['"1995-03-15 01:02:03,5"', "1995-03-15 01:02:03." + "1" * (k + 1), '"1995-03-15"" 01:02:03"']
    for text in texts:
        _needs_host(exes, ("k,t\n1,1995-03-15 01:02:03\n2,%s\n" % text).encode(), [pa.int32(), TS[unit]], R_TIMESTAMP, 2)
    # (more fraction digits than the unit holds: Arrow refuses them)
    with pytest.raises(pa.ArrowInvalid):
        _host(("t\n1995-03-15 01:02:03." + "1" * (k + 1) + "\n").encode(), ["t"], [TS[unit]])
    good = ["1995-03-15 01:02:03", '"1995-03-15T01:02:03"'] + (["1995-03-15 01:02:03." + "1" * d for d in range(1, k + 1)])
    _check(exes, ("t\n" + "\n".join(good) + "\n").encode(), ["t"], [TS[unit]])


def test_grammar_one_is_untouched(exes):
    """the level-1 walk of the same file: a quote byte never reaches it (the splitter reports it), and what it decodes is
    what the level-2 walk decodes when no byte is a quote"""
    data = b"k,s,f\n1,abc,1.5\n,,\n-3,x y,1e3\n"
    types = [pa.int64(), pa.string(), pa.float64()]
    want = _expect(_host(data, ["k", "s", "f"], types))
    for w in BOTH:
        assert _run(exes, w, data, types) == want
        assert _run(exes, w, data, types, quote=None) == want
