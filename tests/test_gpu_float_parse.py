"""float_parse level 2 of the device CSV and JSON decoders (qhip_ctx_set_float_parse(ctx, 2); csrc/device/qhip_float.inc inside
k_csv_decode<1>, k_csv_decode<2> and k_json_decode): every Float64 spelling of the strict grammar and Float32
columns against pyarrow on the same bytes under an explicit schema, bit for bit, values and validity. A value the device does not
settle answers UnsupportedError at the low level, naming reason 9's text and the record. Small files only: 200 rows are three
64-row ballot words and a partial fourth. Every input is well formed for the walk; a needs-host input is a normal return."""
import io
import random
import struct

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pyarrow.json as pajson
import pytest

from qurious_amd import datasource
from qurious_amd._ffi import DeviceTable, UnsupportedError

pytestmark = pytest.mark.gpu

NAMES = ["a", "x", "k", "b"]
SCHEMA = pa.schema([("a", pa.float64()), ("x", pa.float32()), ("k", pa.int64()), ("b", pa.float64())])
REASON = "a float outside the exactly convertible spellings"

LONG_ZEROS = "0." + "0" * 400 + "1e+401"
# the named cases that decode (tests/test_float_parse_cpu.py has them against Python's float()): subnormals, both ends of the normal
# range, ties to even, more than 19 digits whose bounds agree, zeros that do not use up the digit budget, signed zeros
CASES = ["5e-324", "2.2250738585072011e-308", "2.2250738585072014e-308", "1.7976931348623157e308", "9007199254740993", "9007199254740995",
         "0.1000000000000000055511151231257827021181583404541015625", LONG_ZEROS, "-0.0", "-0e0", "0e308", "1e-0000000000000000000005", "1.5"]
REFUSED = ["1e400", "2e-324", "9007199254740993.0000000000000000001"]


@pytest.fixture(autouse=True)
def level2(ctx):
    """level 2 for the test, the default level behind it: the context is the process's"""
    ctx.set_float_parse(2)
    yield ctx
    ctx.set_float_parse(1)


def _rand64(rng):
    b = rng.getrandbits(64)
    return struct.unpack("<d", struct.pack("<Q", b & ~(1 << 62) if (b >> 52) & 0x7FF == 0x7FF else b))[0]      # finite


def _rand32(rng):
    b = rng.getrandbits(32)
    return struct.unpack("<f", struct.pack("<I", b & ~(1 << 30) if (b >> 23) & 0xFF == 0xFF else b))[0]


@pytest.fixture(scope="module")
def rows():
    """200 rows of (repr of a random double, %.9g of a random float, an integer, repr of a random double); one field in ten is None"""
    rng = random.Random(20261021)
    out = []
    for _ in range(200):
        row = [repr(_rand64(rng)), "%.9g" % _rand32(rng), str(rng.randint(-10 ** 15, 10 ** 15)), repr(_rand64(rng))]
        out.append([None if rng.random() < 0.1 else v for v in row])
    return out


def _csv(rows, quoted=False):
    if quoted:
        return (",".join('"%s"' % n for n in NAMES) + "\n" + "".join(",".join('"%s"' % v if v is not None else "" for v in r) + "\n" for r in rows)).encode()
    return (",".join(NAMES) + "\n" + "".join(",".join(v or "" for v in r) + "\n" for r in rows)).encode()


def _json(rows):
    return "".join("{" + ", ".join('"%s": %s' % (n, v if v is not None else "null") for n, v in zip(NAMES, r)) + "}\n" for r in rows).encode()


def _host_csv(data, schema=SCHEMA):
    return pacsv.read_csv(io.BytesIO(data), convert_options=pacsv.ConvertOptions(column_types=schema)).combine_chunks()


def _host_json(data, schema=SCHEMA):
    return pajson.read_json(io.BytesIO(data), parse_options=pajson.ParseOptions(explicit_schema=schema)).combine_chunks()


def _assert_bitwise(dev: DeviceTable, host: pa.Table):
    got = pa.Table.from_batches(dev.to_batches()).combine_chunks()
    assert got.schema == host.schema and got.num_rows == host.num_rows
    for name in host.schema.names:
        a, b = got.column(name).chunk(0), host.column(name).chunk(0)
        assert a.null_count == b.null_count, name
        assert a.is_valid().equals(b.is_valid()), name
        if pa.types.is_floating(a.type):
            word = np.uint64 if pa.types.is_float64(a.type) else np.uint32
            bits = [pa.compute.fill_null(c, 0.0).to_numpy(zero_copy_only=False).view(word) for c in (a, b)]
            assert np.array_equal(bits[0], bits[1]), name
        else:
            assert a.equals(b), name


def test_repr_floats_csv(ctx, rows, tmp_path):
    data = _csv(rows)
    host = _host_csv(data)
    assert all(host.column(n).null_count for n in NAMES)
    ctx.set_float_parse(1)
    with pytest.raises(UnsupportedError, match="Float32 is not decoded on the device"):
        DeviceTable.from_csv_bytes(ctx, SCHEMA, data)
    with pytest.raises(UnsupportedError, match=REASON):
        DeviceTable.from_csv_bytes(ctx, SCHEMA, data, columns=[0, 2, 3])     # the 17-digit spellings alone
    ctx.set_float_parse(2)
    _assert_bitwise(DeviceTable.from_csv_bytes(ctx, SCHEMA, data), host)
    _assert_bitwise(DeviceTable.from_csv_bytes(ctx, SCHEMA, data, columns=[3, 1]), host.select(["b", "x"]))
    # ... and through the reader: on the device at level 2, silently on the host at level 1
    path = str(tmp_path / "t.csv")
    with open(path, "wb") as f:
        f.write(data)
    t = datasource.read_csv(path, schema=SCHEMA, device=True)
    assert t.decoded_on_device is True
    _assert_bitwise(t.device_table(), host)
    ctx.set_float_parse(1)
    assert datasource.read_csv(path, schema=SCHEMA, device=True).decoded_on_device is False


def test_repr_floats_json(ctx, rows, tmp_path):
    data = _json(rows)
    host = _host_json(data)
    ctx.set_float_parse(1)
    with pytest.raises(UnsupportedError, match="Float32 is not decoded on the device"):
        DeviceTable.from_json_bytes(ctx, SCHEMA, data)
    ctx.set_float_parse(2)
    _assert_bitwise(DeviceTable.from_json_bytes(ctx, SCHEMA, data), host)
    _assert_bitwise(DeviceTable.from_json_bytes(ctx, SCHEMA, data, columns=[3, 1]), host.select(["b", "x"]))
    path = str(tmp_path / "t.json")
    with open(path, "wb") as f:
        f.write(data)
    t = datasource.read_json(path, schema=SCHEMA, device=True)
    assert t.decoded_on_device is True
    _assert_bitwise(t.device_table(), host)


def test_repr_floats_quoted_csv(ctx, rows):
    data = _csv(rows, quoted=True)
    ctx.set_csv_grammar(2)
    try:
        _assert_bitwise(DeviceTable.from_csv_bytes(ctx, SCHEMA, data), _host_csv(data))
    finally:
        ctx.set_csv_grammar(1)


def _cycle(n=130, at=None, bad=None):
    vals = [CASES[r % len(CASES)] for r in range(n)]
    if bad is not None:
        vals[at] = bad
    return vals


def test_every_outcome_in_one_wavefront(ctx):
    """130 rows cycle through the named cases: the lanes of one wavefront take Clinger's path, the table path, its subnormal
    branch, the tie, the two conversions of a long spelling and the zero shortcut at once, on both sides of a 64-row boundary"""
    schema = pa.schema([("v", pa.float64()), ("w", pa.float32())])
    f32 = ["1.000000059604644776", "1e-45", "3.4028235e38", "16777217", "0.1", "-0.0", "1.000000059604644775"]
    vals = _cycle()
    data = ("v,w\n" + "".join("%s,%s\n" % (v, f32[r % len(f32)]) for r, v in enumerate(vals))).encode()
    host = _host_csv(data, schema)
    assert host.column("w").to_pylist()[:2] == [1.0000001192092896, 2.0 ** -149]      # one rounding: by way of the double it is 1.0
    _assert_bitwise(DeviceTable.from_csv_bytes(ctx, schema, data), host)
    jdata = "".join('{"v": %s, "w": %s}\n' % (v, f32[r % len(f32)]) for r, v in enumerate(vals)).encode()
    _assert_bitwise(DeviceTable.from_json_bytes(ctx, schema, jdata), _host_json(jdata, schema))


@pytest.mark.parametrize("bad", REFUSED)
def test_refusals_name_the_reason_and_the_record(ctx, bad):
    schema = pa.schema([("v", pa.float64())])
    vals = _cycle(at=69, bad=bad)                  # row 70 of 130
    with pytest.raises(UnsupportedError, match="CSV needs the host path: " + REASON + " in record 70$"):
        DeviceTable.from_csv_bytes(ctx, schema, ("v\n" + "".join(v + "\n" for v in vals)).encode())
    with pytest.raises(UnsupportedError, match="JSON needs the host path: " + REASON + " in record 70$"):
        DeviceTable.from_json_bytes(ctx, schema, "".join('{"v": %s}\n' % v for v in vals).encode())


def test_level_one_is_as_before(ctx):
    ctx.set_float_parse(1)
    data = b"f,g\n1.5,2.5\n,1e22\n-0.0,123456.789\n9007199254740992,-2.5E-3\n"
    with pytest.raises(UnsupportedError, match="Float32 is not decoded on the device"):
        DeviceTable.from_csv_bytes(ctx, pa.schema([("f", pa.float64()), ("g", pa.float32())]), data)
    schema = pa.schema([("f", pa.float64()), ("g", pa.float64())])
    _assert_bitwise(DeviceTable.from_csv_bytes(ctx, schema, data), _host_csv(data, schema))
    with pytest.raises(UnsupportedError, match=REASON + " in record 2"):
        DeviceTable.from_csv_bytes(ctx, schema, b"f,g\n1,2\n0.30000000000000004,3\n")
    ctx.set_float_parse(2)      # the same file at level 2: the same bits
    _assert_bitwise(DeviceTable.from_csv_bytes(ctx, schema, data), _host_csv(data, schema))


def test_the_level_is_checked(ctx):
    for bad in (0, 3):
        with pytest.raises(Exception):
            ctx.set_float_parse(bad)
    ctx.set_float_parse(2)
