"""The float parsers of float_parse level 2 without a GPU (csrc/device/qhip_float.inc, qhip_pow5.inc; the column kinds
QH_CSV_K_FLOAT64_FULL and QH_CSV_K_FLOAT32 of qhip_csv.inc and qhip_json.inc): tests/cpp/float_parse_tests.cpp includes the files
as plain host C++ and compares the parsers with glibc's strtod / strtof in its own process; the expectations that are not glibc's
come from here: Python's `float()` for Float64, pyarrow for Float32 (never `numpy.float32(text)`, which rounds twice) and
`pyarrow.csv.read_csv` / `pyarrow.json.read_json` under an explicit schema for whole files. Built with g++ as a stand-alone
program (nothing of it is loaded into Python), once plainly and once with the address and undefined-behaviour sanitizers."""
import io
import os
import random
import struct
import subprocess
import sys

import pyarrow as pa
import pyarrow.csv as pacsv
import pyarrow.json as pajson
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qurious_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "cpp", "float_parse_tests.cpp")
FLAGS = ["-std=c++17", "-g", "-Wall", "-Werror", "-I" + CSRC]
SAN = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
BOTH = ("plain", "san")
R_FLOAT = 9

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pow5_table  # noqa: E402

sys.path.pop(0)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("float_parse_tests")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("san", SAN)):
        exe = str(d / ("float_parse_tests_" + name))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", exe, SOURCE])
        out[name] = exe
    out["dir"] = d
    return out


def _finish(r):
    assert r.returncode == 0, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()
    return r.stdout.decode().split("\n")[:-1]


def _run(exes, which, *args):
    return _finish(subprocess.run([exes[which]] + [str(a) for a in args], capture_output=True))


def _parse(exes, which, kind, texts):
    path = str(exes["dir"] / "fields.txt")
    with open(path, "w") as f:
        f.write("".join(t + "\n" for t in texts))
    out = _run(exes, which, "parse", kind, path)
    assert len(out) == len(texts)
    return out


def _b64(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def _b32(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]


def _arrow_f32(texts):
    """pyarrow's Float32 of every text (one rounding, from the decimal): the values as Python floats, exact"""
    data = ("v\n" + "".join(t + "\n" for t in texts)).encode()
    col = pacsv.read_csv(io.BytesIO(data), convert_options=pacsv.ConvertOptions(column_types={"v": pa.float32()})).column(0)
    return col.to_pylist()


def test_the_table_is_what_the_script_generates(exes):
    want = ["%016x %016x" % e for e in gen_pow5_table.entries()]
    assert len(want) == 651
    for w in BOTH:
        assert _run(exes, w, "table") == want
    with open(gen_pow5_table.OUT) as f:
        assert f.read() == gen_pow5_table.text()      # the committed text is the generated one


def test_a_million_float64_bit_patterns_at_17_digits(exes):
    assert _run(exes, "plain", "diff64", 1_000_000, 20261021) == ["DIFF64 OK 1000000"]
    assert _run(exes, "san", "diff64", 50_000, 7) == ["DIFF64 OK 50000"]


def test_a_million_float32_bit_patterns_at_9_digits(exes):
    out = _run(exes, "plain", "diff32", 1_000_000, 20261022)
    assert out[0].startswith("DIFF32 OK 1000000 refused "), out
    assert _run(exes, "san", "diff32", 50_000, 8)[0].startswith("DIFF32 OK 50000 ")


def test_shortest_spellings_of_float64(exes):
    rng = random.Random(20261023)
    vals = []
    while len(vals) < 100_000:
        b = rng.getrandbits(64)
        if len(vals) % 16 == 0:
            b &= ~(0x7FF << 52)                       # subnormals
        if (b >> 52) & 0x7FF != 0x7FF:
            vals.append(struct.unpack("<d", struct.pack("<Q", b))[0])
    texts = [repr(v) for v in vals]
    assert max(len(t.lstrip("-").split("e")[0].replace(".", "").strip("0")) for t in texts) == 17      # significant digits
    assert _parse(exes, "plain", "f64", texts) == [_b64(v) for v in vals]
    assert _parse(exes, "san", "f64", texts[:5000]) == [_b64(v) for v in vals[:5000]]


def test_random_digit_strings(exes):
    """1 .. 40 digits, a point and an exponent at random, as Float64 and as Float32: equal to strtod / strtof, or refused in a
    class the program confirms with strtod — the value rounds to zero or infinity, or there are more than 19 significant digits and
    the bounds differ (both kinds must occur for the run to mean anything)"""
    out = _run(exes, "plain", "digits", 400_000, 20261024)
    assert out[0].startswith("DIGITS OK 400000 "), out
    w = out[0].split()
    counts = dict(zip(w[3::2], map(int, w[4::2])))
    assert counts["accepted"] > 400_000 and counts["range"] > 1000 and counts["long"] > 20, counts
    assert _run(exes, "san", "digits", 20_000, 9)[0].startswith("DIGITS OK 20000 ")


def test_clinger_range_inputs_keep_their_bits(exes):
    assert _run(exes, "plain", "clinger", 100_000, 20261025) == ["CLINGER OK 100000"]
    assert _run(exes, "san", "clinger", 5_000, 10) == ["CLINGER OK 5000"]


LONG_ZEROS = "0." + "0" * 400 + "1e+401"
DECODED64 = ["5e-324", "2.2250738585072011e-308", "2.2250738585072014e-308", "1.7976931348623157e308", "9007199254740993", "9007199254740995",
             "0.1000000000000000055511151231257827021181583404541015625", LONG_ZEROS, "-0.0", "-0e0", "0e999999", "1e-0000000000000000000005",
             "6.02214076e23", "1E5", "-1.5e+300", "123456789012345678", "1234567890123456789012345678901234567890", "0.30000000000000004",
             "4.9e-324", "1e-323", "00012.5000", "1" + "0" * 30, "1." + "0" * 30]
REFUSED64 = ["2e-324", "1.7976931348623159e308", "1e309", "1e400", "1e-400", "9007199254740993.0000000000000000001", "1e999999999999999999999999",
             "1e-999999999999999999999999", "+1", ".5", "5.", "1e", "1e+", "inf", "nan", "1 ", " 1", "0x1p3", "-", "1e5.0", "1..5", "--1", "1e--5", "-inf", "Infinity",
             "1_000", "1,5", "1f", "1d", "e5", "-.5", "-5."]


def test_named_cases_float64(exes):
    assert struct.unpack("<Q", struct.pack("<d", float("5e-324")))[0] == 1
    assert float("2.2250738585072011e-308").hex() == "0x0.fffffffffffffp-1022" and float("2.2250738585072014e-308").hex() == "0x1.0000000000000p-1022"
    assert float("9007199254740993") == 2.0 ** 53 and float("9007199254740995") == 2.0 ** 53 + 4
    assert float("9007199254740993.0000000000000000001") == 2.0 ** 53 + 2      # what decoding the 19-digit truncation alone would miss
    assert float("0.1000000000000000055511151231257827021181583404541015625") == 0.1 and float(LONG_ZEROS) == 1.0
    assert float("2e-324") == 0.0 and float("1.7976931348623159e308") == float("inf")
    for w in BOTH:
        assert _parse(exes, w, "f64", DECODED64) == [_b64(float(t)) for t in DECODED64]
        assert _parse(exes, w, "f64", REFUSED64) == ["R%d" % R_FLOAT] * len(REFUSED64)
        assert _parse(exes, w, "f64", ["", "0", "-0"]) == ["N", _b64(0.0), _b64(-0.0)]


DECODED32 = ["1.000000059604644776", "1e-45", "3.4028235e38", "3.40282356e38", "1.17549435e-38", "1.1754942e-38", "16777217", "16777219", "0.1", "-0.0", "0e99",
             "7.0064923216240854e-46", "1.000000059604644775", "1.000000059604644776000000000000000000"]
# (the two long ones: a binary32 tie has 24 digits, so the 19-digit bounds straddle it however close the text is)
REFUSED32 = ["3.4028236e38", "1e-46", "1e39", "7.006492321624085e-46", "1.00000005960464477539062500001", "1.0000000596046447753906250000", "+1", ".5", "5.",
             "nan", "inf"]


def test_named_cases_float32(exes):
    want = _arrow_f32(DECODED32)
    assert want[0] == 1.0000001192092896 and want[1] == 2.0 ** -149
    assert want[12] == 1.0 and want[13] == 1.0000001192092896      # 19 digits just below the halfway point; 37 digits, zeros behind the 19th
    # what pyarrow makes of the range cases is not a finite nonzero value: the host keeps deciding them
    assert _arrow_f32(["3.4028236e38", "1e-46"]) == [float("inf"), 0.0]
    for w in BOTH:
        assert _parse(exes, w, "f32", DECODED32) == [_b32(v) for v in want]
        assert _parse(exes, w, "f32", REFUSED32) == ["R%d" % R_FLOAT] * len(REFUSED32)


# ---- whole files through the record walks
NAMES = ["k", "a", "x", "b", "y"]
TYPES = [pa.int64(), pa.float64(), pa.float32(), pa.float64(), pa.float32()]
CODES = "i64,f64,f32,f64,f32"
SCHEMA = pa.schema(list(zip(NAMES, TYPES)))


def _rand64(rng):
    b = rng.getrandbits(64)
    return struct.unpack("<d", struct.pack("<Q", b & ~(1 << 62) if (b >> 52) & 0x7FF == 0x7FF else b))[0]      # finite


def _rand32(rng):
    b = rng.getrandbits(32)
    return struct.unpack("<f", struct.pack("<I", b & ~(1 << 30) if (b >> 23) & 0xFF == 0xFF else b))[0]


def _rows(seed, n=200, json=False):
    rng = random.Random(seed)
    specials = DECODED64[:12] + ["1e-45", "1.000000059604644776", "3.4028235e38"]
    if json:
        specials[specials.index("0e999999")] = "0e308"      # (Arrow's JSON tokenizer refuses a zero with a larger exponent: below)
    rows = []
    for r in range(n):
        row = [str(rng.randint(-10 ** 12, 10 ** 12)) if rng.random() > 0.1 else None]
        for t in TYPES[1:]:
            u = rng.random()
            if u < 0.12:
                row.append(None)
            elif pa.types.is_float64(t):
                row.append(rng.choice(specials[:12]) if u < 0.3 else repr(_rand64(rng)))
            else:
                row.append(rng.choice(specials[12:] + ["0.1", "-2.5e-3"]) if u < 0.3 else "%.9g" % _rand32(rng))
        rows.append(row)
    return rows


def _cell(v, t):
    if v is None:
        return "N"
    return str(v) if pa.types.is_integer(t) else _b32(v) if pa.types.is_float32(t) else _b64(v)


def _expect(tbl):
    cols = [[_cell(v, f.type) for v in c.to_pylist()] for c, f in zip(tbl.columns, tbl.schema)]
    return ["ROWS %d" % tbl.num_rows] + ["\t".join(r) for r in zip(*cols)]


def _file(exes, data):
    path = str(exes["dir"] / "in.txt")
    with open(path, "wb") as f:
        f.write(data)
    return path


@pytest.mark.parametrize("grammar", [1, 2])
def test_a_csv_file_against_pyarrow(exes, grammar):
    rng = random.Random(grammar)
    rows = _rows(100 + grammar)
    if grammar == 2:      # a quoted CSV: every field in quotes but some of the empty ones ("" and nothing are both NULL)
        lines = [",".join(('"%s"' % v) if v is not None else rng.choice(['""', ""]) for v in row) for row in rows]
        head = ",".join('"%s"' % n for n in NAMES)
    else:
        lines = [",".join(v or "" for v in row) for row in rows]
        head = ",".join(NAMES)
    data = (head + "\n" + "".join(ln + rng.choice(["\n", "\r\n"]) for ln in lines)).encode()
    host = pacsv.read_csv(io.BytesIO(data), convert_options=pacsv.ConvertOptions(column_types=SCHEMA))
    assert host.num_rows == 200 and all(c.null_count for c in host.columns)
    for w in BOTH:
        assert _run(exes, w, "csv", _file(exes, data), CODES, grammar, "-") == _expect(host)
        assert _run(exes, w, "csv", _file(exes, data), CODES, grammar, "4,1") == _expect(host.select(["y", "a"]))      # a projection, out of order
    # the level-1 kind on the same file: its first 17-digit value sends the file to the host
    out = _run(exes, "plain", "csv", _file(exes, data), "i64,f64c,f32,f64,f32", grammar, "-")
    assert out[0].startswith("NEEDS_HOST %d " % R_FLOAT), out
    # one offending value: the reason and the record
    bad = data.replace(lines[69].encode(), (lines[69].split(",")[0] + ',1e400,,,').encode())
    for w in BOTH:
        assert _run(exes, w, "csv", _file(exes, bad), CODES, grammar, "-") == ["NEEDS_HOST %d 70" % R_FLOAT]
        assert _run(exes, w, "csv", _file(exes, bad), CODES, grammar, "0,2") == _expect(
            pacsv.read_csv(io.BytesIO(bad), convert_options=pacsv.ConvertOptions(column_types=SCHEMA, include_columns=["k", "x"])))      # unprojected: never parsed


def test_a_json_file_against_pyarrow(exes):
    rng = random.Random(3)
    rows = _rows(103, json=True)
    lines = []
    for row in rows:
        pairs = []
        for n, v in zip(NAMES, row):
            if v is None and rng.random() < 0.5:
                continue                                  # a missing key; else the literal null
            pairs.append('"%s": %s' % (n, "null" if v is None else v.replace("e+", rng.choice(["e+", "E"]))))
        lines.append("{" + ", ".join(pairs) + "}")
    data = ("\n".join(lines) + "\n").encode()
    host = pajson.read_json(io.BytesIO(data), parse_options=pajson.ParseOptions(explicit_schema=SCHEMA))
    assert host.num_rows == 200 and all(c.null_count for c in host.columns)
    for w in BOTH:
        assert _run(exes, w, "json", _file(exes, data), ",".join(NAMES), CODES, "-") == _expect(host)
        assert _run(exes, w, "json", _file(exes, data), ",".join(NAMES), CODES, "4,1") == _expect(host.select(["y", "a"]))
    # JSON validates every value, projected or not; a number with a leading zero is no JSON number
    # ... and Arrow's tokenizer refuses a zero whose exponent less the fraction digits exceeds 308, which is a value for the CSV
    # reader, and for the parser when it is not told that the token is JSON
    tokenizer = ["0e999999", "0e309", "-0.00e311", "0e09999"]
    for text in tokenizer:
        with pytest.raises(pa.ArrowInvalid, match="Number too big"):
            pajson.read_json(io.BytesIO(('{"a": %s}\n' % text).encode()), parse_options=pajson.ParseOptions(explicit_schema=SCHEMA))
    assert _parse(exes, "plain", "f64", tokenizer) == [_b64(float(t)) for t in tokenizer]
    fine = ["0.00e310", "1" + "0" * 320 + "e-320", "0e308"]
    got = pajson.read_json(io.BytesIO("".join('{"a": %s}\n' % t for t in fine).encode()), parse_options=pajson.ParseOptions(explicit_schema=SCHEMA))
    assert got.column("a").to_pylist() == [0.0, 1.0, 0.0]
    fine_file = _file(exes, "".join('{"a": %s}\n' % t for t in fine).encode())
    assert _run(exes, "plain", "json", fine_file, ",".join(NAMES), CODES, "1") == ["ROWS 3", _b64(0.0), _b64(1.0), _b64(0.0)]
    for text in ["1e400", "2e-324", "9007199254740993.0000000000000000001", "01.5", "-01", "+1", "1.", ".5"] + tokenizer:
        bad = data.replace(lines[69].encode(), ('{"a": %s}' % text).encode())
        for proj in ("-", "0"):
            out = _run(exes, "plain", "json", _file(exes, bad), ",".join(NAMES), CODES, proj)
            assert out[0].split()[0] == "NEEDS_HOST" and out[0].split()[2] == "70", (text, out)
            if text[0] not in "+.":
                assert out == ["NEEDS_HOST %d 70" % R_FLOAT], (text, out)


@pytest.mark.parametrize("mode,code", [("repr", "f64"), ("round6", "f64c")])
def test_the_timing_tools_float_columns(exes, mode, code):
    """tools/csv_decode_timing.py and tools/json_decode_timing.py --floats: what they write decodes through the walks, the
    `repr` columns with the level-2 kind, the `round6` columns with level 1's (Clinger's range), equal to pyarrow"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import csv_decode_timing
        import json_decode_timing
    finally:
        sys.path.pop(0)
    assert csv_decode_timing.FLOAT_NAMES == json_decode_timing.FLOAT_NAMES
    names = csv_decode_timing.FLOAT_NAMES
    schema = pa.schema([(n, pa.float64()) for n in names])
    tbl = pa.table(csv_decode_timing.float_columns(0, 3000, mode), names=names)
    sink = io.BytesIO()
    pacsv.write_csv(tbl, sink, write_options=pacsv.WriteOptions(quoting_style="none"))
    data = sink.getvalue()
    digits = max(len(f.lstrip("-").split("e")[0].replace(".", "").strip("0")) for f in data.decode().split("\n", 1)[1].replace("\n", ",").split(",") if f)
    assert digits == (17 if mode == "repr" else 13)
    want = _expect(pacsv.read_csv(io.BytesIO(data), convert_options=pacsv.ConvertOptions(column_types=schema)))
    assert want == _expect(tbl)
    assert _run(exes, "plain", "csv", _file(exes, data), ",".join([code] * 2), 1, "-") == want
    lines = json_decode_timing.json_lines(pa.table(json_decode_timing.float_columns(0, 3000, mode), names=names), None)
    jdata = "".join(lines.to_pylist()).encode()
    assert _run(exes, "plain", "json", _file(exes, jdata), ",".join(names), ",".join([code] * 2), "-") == want
    if mode == "repr":
        assert _run(exes, "plain", "csv", _file(exes, data), "f64c,f64c", 1, "-")[0].startswith("NEEDS_HOST %d " % R_FLOAT)
