"""The device JSON decoder without a GPU (csrc/device/qhip_json.inc: the record walk over one object per line, the value grammar
of every column type, the unescaping copy's lane logic): tests/cpp/json_tests.cpp includes the file as plain host C++ and decodes
a file into a text dump, which is compared with `pyarrow.json.read_json(explicit_schema=...)` on the same bytes. Built with g++ as
a stand-alone program (nothing of it is loaded into Python), once plainly and once with the address and undefined-behaviour
sanitizers; the file and every buffer carry exactly the 64 bytes of slack a device allocation has.

Every row of DESIGN §3.10's two tables is re-checked here against the pyarrow that is installed: a "decoded" spelling must give the
host's value, a "needs the host" spelling must be refused with its reason and 1-based record, in a projected and in an unprojected
field, and what the host does with it (a lenient reading or an error) is asserted next to it."""
import datetime
import decimal
import io
import json
import os
import random
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.json as pajson
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qurious_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "cpp", "json_tests.cpp")
FLAGS = ["-std=c++17", "-g", "-Wall", "-Werror", "-I" + CSRC]
SAN = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
BOTH = ("plain", "san")

R_LONE_CR, R_EMPTY_LINE, R_SYNTAX, R_INT, R_DATE, R_DECIMAL, R_FLOAT, R_UTF8 = 3, 4, 5, 6, 7, 8, 9, 10
R_KEY_ESCAPE, R_TIMESTAMP, R_KEY_UNKNOWN, R_KEY_TWICE, R_NESTED, R_UESCAPE, R_ESCAPE, R_CONTROL, R_KIND = 12, 14, 15, 16, 17, 18, 19, 20, 21

TS = {"s": pa.timestamp("s"), "ms": pa.timestamp("ms"), "us": pa.timestamp("us"), "ns": pa.timestamp("ns")}
DIGITS = {"s": 0, "ms": 3, "us": 6, "ns": 9}
DEC = pa.decimal128(15, 2)
INTS = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64()]
TYPE_CODE = {pa.int8(): "i8", pa.int16(): "i16", pa.int32(): "i32", pa.int64(): "i64", pa.uint8(): "u8", pa.uint16(): "u16",
             pa.uint32(): "u32", pa.uint64(): "u64", pa.float64(): "f64", pa.date32(): "date", pa.string(): "utf8", pa.bool_(): "bool",
             TS["s"]: "ts0", TS["ms"]: "ts3", TS["us"]: "ts6", TS["ns"]: "ts9"}


def _code(t):
    return f"dec:{t.precision}:{t.scale}" if pa.types.is_decimal(t) else TYPE_CODE[t]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("json_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("json_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


def _finish(r):
    assert r.returncode == 0, r.stderr.decode()
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()
    return r.stdout.decode().split("\n")[:-1]


def _run(exes, which, data, names, types, proj=None):
    path = str(exes["dir"] / "in.json")
    with open(path, "wb") as f:
        f.write(data)
    args = [exes[which], "decode", path, ",".join(names), ",".join(_code(t) for t in types), ",".join(map(str, proj)) if proj else "-"]
    return _finish(subprocess.run(args, capture_output=True))


def _host(data, names, types, select=None):
    tbl = pajson.read_json(io.BytesIO(data), parse_options=pajson.ParseOptions(explicit_schema=pa.schema(list(zip(names, types)))))
    return tbl.select(select) if select is not None else tbl


def _cell(v, t):
    if v is None:
        return "N"
    if pa.types.is_float64(t):
        return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]
    if pa.types.is_date32(t):
        return str(v)
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
        if pa.types.is_date32(f.type):
            c = c.cast(pa.int32())                # (python's date does not reach Int32's limits)
        cols.append([_cell(v, f.type) for v in c.to_pylist()])
    return ["ROWS %d" % tbl.num_rows] + ["\t".join(r) for r in zip(*cols)]


def _check(exes, data, names, types, which=BOTH):
    host = _host(data, names, types)
    assert host.schema.names == list(names) and [f.type for f in host.schema] == list(types)
    want = _expect(host)
    for w in which:
        assert _run(exes, w, data, names, types) == want, data[:200]
    return want


def _needs_host(exes, data, names, types, reason, record, which=BOTH, **kw):
    for w in which:
        assert _run(exes, w, data, names, types, **kw) == ["NEEDS_HOST %d %d" % (reason, record)], data[:200]


def _host_refuses(data, names, types):
    with pytest.raises((pa.ArrowInvalid, pa.ArrowNotImplementedError)):
        _host(data, names, types)


def _value_case(exes, t, text, reason, host):
    """the spelling `text` as the value of a field of type t, in record 2 of 3: refused with `reason` whether the field is
    projected or not; host: "refuses", or the python value the host reads from it (a lenient reading the device leaves to it),
    or "reads" where the host's value is its own business (RapidJSON's 17-digit doubles, decimals beyond their precision)"""
    names, types = ["k", "v", "w"], [pa.int32(), t, pa.string()]
    data = ('{"k":1,"w":"a"}\n{"k":2,"v":%s,"w":"b"}\n{"k":3}\n' % text).encode()
    _needs_host(exes, data, names, types, reason, 2)
    _needs_host(exes, data, names, types, reason, 2, proj=[2, 0])
    if host == "refuses":
        _host_refuses(data, names, types)
    elif host == "reads":
        assert _host(data, names, types).column("v").to_pylist()[1] is not None, text
    else:
        assert _host(data, names, types).column("v").to_pylist() == [None, host, None], text


def test_the_unescaping_copy_against_a_byte_serial_one(exes):
    """runs of 1..130 backslashes at every offset 0..129, through the 64-byte steps with a simulated ballot"""
    for w in BOTH:
        assert _finish(subprocess.run([exes[w], "unescape"], capture_output=True)) == ["UNESCAPE OK %d" % (130 * 130)]


def test_structure_that_is_decoded(exes):
    names, types = ["a", "s", "b"], [pa.int64(), pa.string(), pa.bool_()]
    rows = ['{"a":1,"s":"x","b":true}', ' \t{ "a" :\t2 , "s" : "y" ,"b":false }\t ', '{"b":null,"s":null,"a":null}', '{}', '{ }', '{"s":"only"}',
            '{"b":true,"a":-7}', '{"s":"","a":0}']
    for end in ("\n", "\r\n"):
        for final in (end, ""):
            data = (end.join(rows) + final).encode()
            want = _check(exes, data, names, types)
            assert want[3] == want[4] == want[5] == "N\tN\tN" and want[8] == "0\ts\tN"
    # a projection in another order than the schema's; a one-record file without a line end
    data = ("\n".join(rows) + "\n").encode()
    want = _expect(_host(data, names, types, select=["b", "a"]))
    for w in BOTH:
        assert _run(exes, w, data, names, types, proj=[2, 0]) == want
    _check(exes, b'{"a":5}', names, types)


def test_structure_that_needs_the_host(exes):
    names, types = ["a", "s"], [pa.int64(), pa.string()]
    good = '{"a":1,"s":"x"}'
    host = lambda data: _host(data, names, types)   # noqa: E731
    # the splitter's verdicts
    _needs_host(exes, (good + "\n" + good + "\r" + good + "\n").encode(), names, types, R_LONE_CR, 2)
    _needs_host(exes, (good + "\n\n" + good + "\n").encode(), names, types, R_EMPTY_LINE, 2)
    _needs_host(exes, ("\n" + good + "\n").encode(), names, types, R_EMPTY_LINE, 1)
    assert host((good + "\n\n" + good + "\n").encode()).num_rows == 2            # the host skips empty and blank lines
    assert host((good + "\n  \n" + good + "\n").encode()).num_rows == 2
    for w in BOTH:
        assert _run(exes, w, b"", names, types) == ["NEEDS_HOST empty 0"]
        assert _run(exes, w, b"\xef\xbb\xbf" + good.encode() + b"\n", names, types) == ["NEEDS_HOST bom 0"]
    # the walk's, in record 2 of 3, with a projection that leaves the offending field out as well
    cases = [
        ("   ", R_SYNTAX, 2),                                     # a blank line
        (good + good, R_SYNTAX, 4),                               # two objects on one line: the host reads both
        (good + " x", R_SYNTAX, "refuses"),
        (good + "\x0c", R_SYNTAX, "refuses"),
        ("[1]", R_SYNTAX, "refuses"),
        ('{"a":1,"s":"x"', R_SYNTAX, "refuses"),                  # cut records
        ('{"a":1,"s":"x', R_SYNTAX, "refuses"),
        ('{"a":1,"s":"x\\', R_SYNTAX, "refuses"),
        ('{"a":1,"s', R_SYNTAX, "refuses"),
        ('{"a":', R_SYNTAX, "refuses"),
        ('{"a"', R_SYNTAX, "refuses"),
        ('{"a":1,"s":"x",}', R_SYNTAX, "refuses"),                # a trailing comma
        ('{"a":1 "s":"x"}', R_SYNTAX, "refuses"),
        ('{"a" 1}', R_SYNTAX, "refuses"),
        ('{a:1}', R_SYNTAX, "refuses"),
        ('{"a":nul}', R_SYNTAX, "refuses"),
        ('{"a":truee}', R_SYNTAX, "refuses"),
        ('{"a":+1}', R_SYNTAX, "refuses"),
        ('{"a":}', R_SYNTAX, "refuses"),
        ('{"\\u0061":1}', R_KEY_ESCAPE, 3),                       # the host resolves the escape: key a
        ('{"a\\n":1}', R_KEY_ESCAPE, None),
        ('{"a":1,"zz":2}', R_KEY_UNKNOWN, None),                  # the host appends a column
        ('{"A":1}', R_KEY_UNKNOWN, None),
        ('{"":1}', R_KEY_UNKNOWN, None),
        ('{"a":1,"s":"x","a":2}', R_KEY_TWICE, "refuses"),
        ('{"s":"x","s":"x"}', R_KEY_TWICE, "refuses"),
        ('{"a":{"x":1}}', R_NESTED, "refuses"),
        ('{"a":[1]}', R_NESTED, "refuses"),
        ('{"s":{}}', R_NESTED, "refuses"),
        ('{"s":[]}', R_NESTED, "refuses"),
    ]
    for text, reason, what in cases:
        data = (good + "\n" + text + "\n" + good + "\n").encode()
        _needs_host(exes, data, names, types, reason, 2)
        _needs_host(exes, data, names, types, reason, 2, proj=[1])
        _needs_host(exes, data, names, types, reason, 2, proj=[0])
        if what == "refuses":
            _host_refuses(data, names, types)
        elif what is None:
            assert len(host(data).schema) == 3                    # a new column
        else:
            assert host(data).num_rows == what and len(host(data).schema) == 2
    # a record cut by a raw line end inside a string: its first piece has no closing quote
    for cut in ('{"a":1,"s":"x\ny"}', '{"a":1,"s":"x\r\ny"}', '{"a":1,"s":"x\\\\\ny"}'):
        data = (good + "\n" + cut + "\n" + good + "\n").encode()
        _needs_host(exes, data, names, types, R_SYNTAX, 2)
        _needs_host(exes, data, names, types, R_SYNTAX, 2, proj=[0])
        _host_refuses(data, names, types)


def test_integer_spellings_and_limits(exes):
    for t in INTS:
        bits, signed = t.bit_width, pa.types.is_signed_integer(t)
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
        texts = [str(lo), str(hi), "0", "7", str(hi - 1)] + (["-0", "-1", str(lo + 1)] if signed else [])
        data = "".join('{"v":%s}\n' % x for x in texts).encode()
        want = _check(exes, data, ["v"], [t])
        assert want[1:] == [str(int(x)) for x in texts]
        for text in (str(hi + 1), str(lo - 1), "99999999999999999999", "1.0", "1E3", "1e0", "0.0"):
            _value_case(exes, t, text, R_INT, "refuses")
        for text in ("01", "-01", "00"):                          # leading zeros: no JSON number, the host's parser stops there
            _value_case(exes, t, text, R_INT, "refuses")
        if not signed:
            _value_case(exes, t, "-1", R_INT, "refuses")
            _value_case(exes, t, "-0", R_INT, "refuses")          # any '-' in an unsigned column: the host refuses "-0" too
        for text in ('"1"', "true", '""'):
            _value_case(exes, t, text, R_KIND, "refuses")
        _value_case(exes, t, "-", R_INT, "refuses")


def test_date32_is_a_number_of_days(exes):
    want = _check(exes, b'{"d":9000}\n{"d":0}\n{"d":-719162}\n{"d":2147483647}\n{"d":-2147483648}\n{"d":null}\n{}\n', ["d"], [pa.date32()], which=("plain",))
    assert want[1:] == ["9000", "0", "-719162", "2147483647", "-2147483648", "N", "N"]
    assert _host(b'{"d":9000}\n', ["d"], [pa.date32()]).column(0).to_pylist() == [datetime.date(1994, 8, 23)]
    for w in BOTH:
        assert _run(exes, w, b'{"d":9000}\n{"d":-1}\n', ["d"], [pa.date32()]) == ["ROWS 2", "9000", "-1"]
    _value_case(exes, pa.date32(), '"1995-03-15"', R_KIND, "refuses")
    for text in ("2147483648", "-2147483649", "1.5", "1e2", "007"):
        _value_case(exes, pa.date32(), text, R_DATE, "refuses")


def test_float_spellings(exes):
    texts = ["0", "-0", "-0.0", "0.0", "1", "-1.5", "1e3", "1E3", "1e+3", "2.5e-3", "1.25E+10", "9007199254740992", "123456789012345e-22", "1e22", "1e-22",
             "0.1", "0.3", "123456.789", "5e0", "0e5", "100", "9007199254740991e7"]
    data = "".join('{"f":%s}\n' % x for x in texts).encode()
    want = _check(exes, data, ["f"], [pa.float64()])
    assert want[1:4] == ["0000000000000000", "8000000000000000", "8000000000000000"]      # -0 and -0.0 keep their sign
    # the host reads these too, the device leaves them to it
    for text, value in (("9007199254740993", 9007199254740992.0), ("0.12345678901234567", "reads"), ("1e23", 1e23), ("1e-23", "reads"), ("1e308", 1e308)):
        _value_case(exes, pa.float64(), text, R_FLOAT, value)
    for text in ("1e400", "01", "-01.5", "1.", "1.e3", "1e", "1e+", "-"):
        _value_case(exes, pa.float64(), text, R_FLOAT, "refuses")
    for text in (".5", "+1", "nan", "inf"):
        _value_case(exes, pa.float64(), text, R_SYNTAX, "refuses")
    for text in ("NaN", "Infinity"):                                  # the host's parser knows these two words
        _value_case(exes, pa.float64(), text, R_SYNTAX, "reads")
    for text in ('"1.5"', "true", "false"):
        _value_case(exes, pa.float64(), text, R_KIND, "refuses")


def test_a_hundred_thousand_fast_path_floats_bit_for_bit(exes):
    rng = random.Random(7)
    texts = []
    for _ in range(100_000):
        digits = str(rng.randint(0, 1 << 53) if rng.random() < 0.5 else rng.randint(0, 10 ** rng.randint(1, 15)))
        nf = rng.randint(0, len(digits) - 1)                  # fraction digits: the point stands inside the digits
        power = rng.randint(-22, 22)                          # the effective power of ten of the digits read as one integer
        written = power + nf
        s = digits[:len(digits) - nf] + ("." + digits[len(digits) - nf:] if nf else "")
        if written or rng.random() < 0.2:
            s += rng.choice("eE") + rng.choice(["", "+"] if written >= 0 else [""]) + str(written)
        texts.append(("-" if rng.random() < 0.3 else "") + s)
    data = "".join('{"f":%s}\n' % x for x in texts).encode()
    got = _run(exes, "plain", data, ["f"], [pa.float64()])
    assert got[0] == "ROWS 100000", got[0]
    host = _host(data, ["f"], [pa.float64()]).column(0).combine_chunks().to_numpy().view(np.uint64)
    assert np.array_equal(np.array([int(x, 16) for x in got[1:]], dtype=np.uint64), host)
    py = np.array([float(x) for x in texts], dtype=np.float64).view(np.uint64)
    assert np.array_equal(host, py)
    small = "".join('{"f":%s}\n' % x for x in texts[:5000]).encode()
    assert _run(exes, "san", small, ["f"], [pa.float64()]) == ["ROWS 5000"] + got[1:5001]


def test_decimal_spellings(exes):
    t = pa.decimal128(10, 2)
    texts = ["12", "12.3", "-0.5", "0", "-0", "0.25", "99999999.99", "-99999999.99", '"12.34"', '".5"', '"5."', '"-.5"', '"007"', '"-0"', '"99999999.99"', "null"]
    data = "".join('{"d":%s}\n' % x for x in texts).encode()
    want = _check(exes, data, ["d"], [t])
    assert want[1:5] == ["1200", "1230", "-50", "0"] and want[9:12] == ["1234", "50", "500"]
    D = decimal.Decimal
    for text, value in (("1e2", D("100.00")), ('"1e2"', D("100.00")), ('"+1.5"', D("1.50")), ("1E0", D("1.00")), ("1.5e1", D("15.00"))):
        _value_case(exes, t, text, R_DECIMAL, value)
    for text in ("100000000", '"100000000"', "123456789.1"):           # beyond the precision: the host does not check it
        _value_case(exes, t, text, R_DECIMAL, "reads")
    _value_case(exes, t, '"1\\u0032"', R_DECIMAL, D("12.00"))            # the host resolves the escape
    for text in ("1.234", '"1.234"', '""', '" 1"', '"1 "', '"1.2.3"', '"."', '"-"', '"abc"', "1.", "01", "-01.5", "-"):
        _value_case(exes, t, text, R_DECIMAL, "refuses")
    _value_case(exes, t, ".5", R_SYNTAX, "refuses")
    for text in ("true", "false"):
        _value_case(exes, t, text, R_KIND, "refuses")
    for p, s in ((38, 0), (38, 10), (38, 38), (1, 0), (5, 5)):
        tt = pa.decimal128(p, s)
        top = "9" * p
        spell = (top[:p - s] or "0") + ("." + top[p - s:] if s else "")
        texts = [spell, "-" + spell, '"%s"' % spell, '"-%s"' % spell, "0"]
        _check(exes, "".join('{"d":%s}\n' % x for x in texts).encode(), ["d"], [tt])
        over = "1" + "0" * (p - s) if p > s else "1"
        _value_case(exes, tt, over, R_DECIMAL, "reads" if s else "refuses")   # (10^38 does not fit; below that the host does not check)


def test_random_decimals_as_numbers_and_as_strings(exes):
    rng = random.Random(11)
    t = pa.decimal128(20, 4)
    texts = []
    for _ in range(20000):
        whole, frac_digits = rng.randint(0, 10 ** rng.randint(1, 16) - 1), rng.randint(0, 4)
        s = ("-" if rng.random() < 0.4 else "") + str(whole) + ("." + "".join(rng.choice("0123456789") for _ in range(frac_digits)) if frac_digits else "")
        texts.append('"%s"' % s if rng.random() < 0.5 else s)
    data = "".join('{"d":%s}\n' % x for x in texts).encode()
    _check(exes, data, ["d"], [t], which=("plain",))
    _check(exes, "".join('{"d":%s}\n' % x for x in texts[:3000]).encode(), ["d"], [t], which=("san",))


def test_boolean_and_null_literals(exes):
    data = b'{"k":1,"b":true}\n{"k":2,"b":false}\n{"k":3,"b":null}\n{"k":4}\n'
    assert _check(exes, data, ["k", "b"], [pa.int32(), pa.bool_()])[1:] == ["1\t1", "2\t0", "3\tN", "4\tN"]
    for text in ("1", "0", '"true"', '"false"', '""'):
        _value_case(exes, pa.bool_(), text, R_KIND, "refuses")
    for text in ("True", "TRUE", "tru", "truee", "nul", "nulll", "NULL", "fals", "yes"):
        _value_case(exes, pa.bool_(), text, R_SYNTAX, "refuses")
    # null is NULL for a column of every type
    types = INTS + [pa.float64(), pa.date32(), DEC, pa.bool_(), TS["s"], TS["ms"], TS["us"], TS["ns"], pa.string()]
    names = ["c%d" % k for k in range(len(types))]
    row = "{" + ",".join('"%s":null' % n for n in names) + "}\n"
    want = _check(exes, (row + "{}\n").encode(), names, types)
    assert want[1:] == ["\t".join(["N"] * len(types))] * 2


def _ts_text(dt, frac_digits, frac, sep):
    s = "%04d-%02d-%02d%s%02d:%02d:%02d" % (dt.year, dt.month, dt.day, sep, dt.hour, dt.minute, dt.second)
    return s + ("." + ("%09d" % frac)[:frac_digits] if frac_digits else "")


EPOCH = datetime.datetime(1970, 1, 1)


def _units(dt, frac_digits, frac, unit):
    secs = (dt - EPOCH).days * 86400 + (dt - EPOCH).seconds
    kept = int(("%09d" % frac)[:frac_digits].ljust(9, "0")) if frac_digits else 0
    return secs * 10 ** DIGITS[unit] + kept // 10 ** (9 - DIGITS[unit])


@pytest.mark.parametrize("unit", list(TS))
def test_timestamps_at_each_units_limits(exes, unit):
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
    rng = random.Random(k)
    lo, hi = (datetime.datetime(1, 1, 1), datetime.datetime(9999, 12, 31, 23, 59, 59)) if unit != "ns" else (datetime.datetime(1677, 9, 22), datetime.datetime(2262, 4, 11))
    for _ in range(3000):
        dt = lo + datetime.timedelta(seconds=rng.randint(0, int((hi - lo).total_seconds())))
        fd, frac = rng.randint(0, k), rng.randint(0, 999_999_999)
        texts.append(_ts_text(dt, fd, frac, rng.choice(" T")))
        want.append(_units(dt, fd, frac, unit))
    if unit == "ns":
        texts += ["1677-09-21T00:12:44", "1677-09-21T00:12:44.000000001", "2262-04-11T23:47:16.854775807", "2262-04-11 23:47:16"]
        want += [-9223372036 * 10 ** 9, -9223372036 * 10 ** 9 + 1, 2 ** 63 - 1, 9223372036 * 10 ** 9]
    data = "".join('{"t":"%s"}\n' % x for x in texts).encode()
    got = _check(exes, data, ["t"], [TS[unit]])
    assert [int(x) for x in got[1:]] == want
    t = TS[unit]
    if unit == "ns":
        for text in ("1677-09-21T00:12:43.999999999", "2262-04-11T23:47:16.854775808", "1677-09-21 00:12:43", "2262-04-11 23:47:17", "0001-01-01 00:00:00"):
            _value_case(exes, t, '"%s"' % text, R_TIMESTAMP, "refuses")
    _value_case(exes, t, '"1995-03-15"', R_TIMESTAMP, datetime.datetime(1995, 3, 15))          # the date-only spelling: the host reads it
    _value_case(exes, t, '"1995-03-15 01:02"', R_TIMESTAMP, datetime.datetime(1995, 3, 15, 1, 2))
    _value_case(exes, t, '"1995-03-15 01:02:0\\u0033"', R_TIMESTAMP, datetime.datetime(1995, 3, 15, 1, 2, 3))
    for text in ('"1995-03-15 01:02:03.%s"' % ("1" * (k + 1)), '""', '"1995-02-30 00:00:00"', '"1995-03-15 24:00:00"', '" 1995-03-15 01:02:03"', '"1995-03-15 01:02:03 "',
                 '"1995-03-15 01:02:03."', '"abc"'):
        _value_case(exes, t, text, R_TIMESTAMP, "refuses")
    for text in ("5", "19950315", "true"):
        _value_case(exes, t, text, R_KIND, "refuses")


def test_timestamps_with_a_zone_need_the_host(exes):
    _value_case(exes, TS["s"], '"1995-03-15 01:02:03Z"', R_TIMESTAMP, datetime.datetime(1995, 3, 15, 1, 2, 3))       # the host accepts these for unit s
    _value_case(exes, TS["s"], '"1995-03-15 01:02:03+01:00"', R_TIMESTAMP, datetime.datetime(1995, 3, 15, 0, 2, 3))


SIMPLE = {'\\"': '"', "\\\\": "\\", "\\/": "/", "\\b": "\b", "\\f": "\f", "\\n": "\n", "\\r": "\r", "\\t": "\t"}


def test_string_spellings(exes):
    inners = ["", "a", "ä€\U0001f600", "with / slash", "x" * 64, "y" * 65, "nul"] + list(SIMPLE) + ["".join(SIMPLE), "a" + "".join(SIMPLE) * 9 + "z"]
    inners += ["q" * 60 + e + "r" * 10 for e in SIMPLE] + ["ä" * 31 + e + "€" * 30 for e in SIMPLE]           # escapes on and around the 64-byte step
    inners += ["p" * k + "\\\\" * 40 + "\\n" + "s" * 70 for k in (0, 1, 23, 24, 25, 63)]
    data = "".join('{"k":%d,"s":"%s"}\n' % (i, x) for i, x in enumerate(inners)).encode()
    want = _check(exes, data, ["k", "s"], [pa.int32(), pa.string()])
    plain = [json.loads('"%s"' % x) for x in inners]                 # (an independent reading of the escapes)
    assert [r.split("\t")[1] for r in want[1:]] == ["s" + x.encode().hex() for x in plain]
    t = pa.string()
    _value_case(exes, t, '"\\u0041"', R_UESCAPE, "A")
    _value_case(exes, t, '"ab\\u00e4"', R_UESCAPE, "abä")
    for text in ('"\\q"', '"\\x41"', '"\\0"', '"\\U0041"', '"a\\ b"', "\"\\'\""):
        _value_case(exes, t, text, R_ESCAPE, "refuses")
    for text in ('"a\x01b"', '"\x1f"', '"tab\there"', '"\x00"'):
        _value_case(exes, t, text, R_CONTROL, "refuses")
    for text in ("5", "1.5", "true", "false"):
        _value_case(exes, t, text, R_KIND, "refuses")
    # invalid UTF-8: the host lets it through unvalidated, the Utf8 columns here do not
    for raw in (b"\xff", b"\xc3", b"\xe2\x82", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"a\x80"):
        data = b'{"k":1}\n{"k":2,"s":"' + raw + b'"}\n'
        _needs_host(exes, data, ["k", "s"], [pa.int32(), pa.string()], R_UTF8, 2)
        _needs_host(exes, data, ["k", "s"], [pa.int32(), pa.string()], R_UTF8, 2, proj=[0])
        assert _host(data, ["k", "s"], [pa.int32(), pa.string()]).num_rows == 2


def test_backslash_runs_through_the_decoder(exes):
    """runs of backslashes of every length 1..130 (2 k raw backslashes, then an escaped quote for an odd count) at offsets around
    the 64-byte steps: where the string ends depends on the run's parity, and the copy must drop every other backslash"""
    inners = []
    for run in range(1, 131):
        for at in (0, 1, 31, 62, 63, 64, 65, 129):
            inners.append("a" * at + "\\\\" * (run // 2) + ('\\"' if run % 2 else "") + "b" * (run % 7))
    data = "".join('{"s":"%s"}\n' % x for x in inners).encode()
    want = _check(exes, data, ["s"], [pa.string()])
    assert [json.loads('"%s"' % x) for x in inners] == _host(data, ["s"], [pa.string()]).column(0).to_pylist()


def _rand_value(rng, t):
    if rng.random() < 0.1:
        return "null"
    if pa.types.is_string(t):
        return '"%s"' % rng.choice(["", "a", "hello world", "ä€\U0001f600", "x" * rng.randint(60, 70), 'say \\"hi\\"', "line\\nbreak\\ttab", "\\\\" * rng.randint(1, 40),
                                    "p" * rng.randint(50, 70) + "\\/" + "q" * rng.randint(0, 80), "{not,an:object}", "[1,2]"])
    if pa.types.is_int32(t):
        return rng.choice(["0", "-17", "2147483647", "-2147483648", str(rng.randint(-10 ** 6, 10 ** 6))])
    if pa.types.is_uint64(t):
        return rng.choice(["0", "18446744073709551615", str(rng.randint(0, 10 ** 18))])
    if pa.types.is_date32(t):
        return str(rng.randint(-719162, 2932896))
    if pa.types.is_boolean(t):
        return rng.choice(["true", "false"])
    if pa.types.is_timestamp(t):
        return '"%s"' % rng.choice(["1995-03-15 12:34:56", "2024-02-29T23:59:59.5", "1970-01-01 00:00:00.000001", "0001-01-01T00:00:00"])
    if pa.types.is_float64(t):
        return rng.choice(["1.5", "-0.0", "1e3", "0.1", "123456.789", str(rng.randint(-10 ** 9, 10 ** 9))])
    v = rng.choice(["1.5", "-0.5", "12", "%d.%02d" % (rng.randint(0, 10 ** 6), rng.randint(0, 99))])
    return '"%s"' % v if rng.random() < 0.5 else v


def test_random_records_with_shuffled_keys_missing_keys_nulls_and_blanks(exes):
    names = ["s", "i", "d", "b", "t", "m", "u", "f", "comment"]
    types = [pa.string(), pa.int32(), pa.date32(), pa.bool_(), TS["us"], DEC, pa.uint64(), pa.float64(), pa.string()]
    rng = random.Random(20261020)
    ws = lambda: rng.choice(["", "", "", " ", "\t", "  ", " \t "])   # noqa: E731
    recs = []
    for _ in range(3000):
        keys = [k for k in range(len(names)) if rng.random() < 0.85]
        if rng.random() < 0.5:
            rng.shuffle(keys)
        pairs = ['"%s"%s:%s%s' % (names[k], ws(), ws(), _rand_value(rng, types[k])) for k in keys]
        recs.append(ws() + "{" + ws() + (ws() + "," + ws()).join(pairs) + ws() + "}" + ws())
    data = "".join(r + rng.choice(["\n", "\r\n"]) for r in recs).encode()
    _check(exes, data, names, types)
    want = _expect(_host(data, names, types, select=["comment", "b", "i", "s"]))
    for w in BOTH:
        assert _run(exes, w, data, names, types, proj=[8, 3, 1, 0]) == want
    # a duplicate key, of a projected and of an unprojected field, at a random record
    for _ in range(6):
        r, k = rng.randrange(len(recs)), rng.choice([1, 8])
        bad = list(recs)
        bad[r] = '{"%s":null,"i":5,"comment":"c","%s":null}' % (names[k], names[k])
        bdata = ("\n".join(bad) + "\n").encode()
        for proj in (None, [1], [8], [0]):
            assert _run(exes, "plain", bdata, names, types, proj=proj) == ["NEEDS_HOST %d %d" % (R_KEY_TWICE, r + 1)]
        _host_refuses(bdata, names, types)


def test_key_lookup(exes):
    """keys that are prefixes of one another, the empty key, 64 fields in reversed order"""
    names, types = ["a", "ab", "abc", "", "b"], [pa.int32()] * 5
    data = b'{"abc":3,"ab":2,"a":1,"":4,"b":5}\n{"b":1,"":2}\n{"ab":7}\n'
    assert _check(exes, data, names, types)[1:] == ["1\t2\t3\t4\t5", "N\tN\tN\t2\t1", "N\t7\tN\tN\tN"]
    names = ["field_%02d" % k for k in range(64)]
    types = [pa.int64()] * 64
    rows = ["{" + ",".join('"%s":%d' % (n, 100 * r + k) for k, n in order) + "}" for r, order in
            enumerate([list(enumerate(names)), list(enumerate(names))[::-1], list(enumerate(names))[::2], list(enumerate(names))[63:]])]
    want = _check(exes, ("\n".join(rows) + "\n").encode(), names, types)
    assert want[2].split("\t")[63] == "163" and want[3].split("\t")[:3] == ["200", "N", "202"] and want[4].split("\t")[62:] == ["N", "363"]


def test_the_library_exports_the_entry_points():
    """the C ABI of the decoder (include/qhip.h); without a context both calls refuse their arguments and touch no device"""
    import ctypes as C
    from qurious_amd._ffi import load_library
    lib = load_library()
    assert hasattr(lib, "qhip_table_from_json") and hasattr(lib, "qhip_ctx_json_pass_ms")
    out = C.c_void_p()
    assert lib.qhip_table_from_json(None, None, None, 0, None, 0, 0, C.byref(out)) != 0 and not out.value
    ms = (C.c_double * 5)()
    assert lib.qhip_ctx_json_pass_ms(None, ms, 5) != 0
    with open(os.path.join(ROOT, "include", "qhip.h")) as f:
        header = f.read()
    assert "int qhip_table_from_json(qhip_ctx* ctx, const struct ArrowSchema* schema, const void* bytes, int64_t n_bytes," in header


def test_a_required_field_belongs_to_the_host(tmp_path):
    """a schema field that is not nullable: the host refuses a record in which it is absent or null, where the device's walk would
    store a NULL. The device path hands such a schema to the host before it touches a device, so this runs without one"""
    from qurious_amd import datasource
    schema = pa.schema([pa.field("a", pa.int64(), nullable=False), pa.field("b", pa.string())])
    for text, names in (('{"a":1,"b":"x"}\n{"b":"y"}\n', "a required field was absent"), ('{"a":1,"b":"x"}\n{"a":null}\n', "a required field was null")):
        path = str(tmp_path / "t.json")
        with open(path, "w") as f:
            f.write(text)
        assert datasource._device_read_json(path, schema, None, None) is None
        assert datasource._device_read_json(path, schema, None, ["b"]) is None
        for device in (False, True):
            with pytest.raises(pa.ArrowInvalid, match=names):
                datasource.read_json(path, schema=schema, device=device)
    with open(path, "w") as f:
        f.write('{"a":1,"b":"x"}\n{"a":2}\n')
    assert datasource._device_read_json(path, schema, None, None) is None
    both = [datasource.read_json(path, schema=schema, device=d) for d in (False, True)]
    assert both[0].decoded_on_device is False and both[1].decoded_on_device is False
    assert pa.Table.from_batches(both[1].data).equals(pa.Table.from_batches(both[0].data)) and both[0].data[0].column("a").to_pylist() == [1, 2]
