"""bench.py's command line: a plain run prints the headline only, --dump-outputs writes the last timed step's results."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import qurious_amd as q
from qurious_amd import queries, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Result:
    """Stands in for a plan's device result: to_batches() hands out host Arrow batches."""

    def __init__(self, batches):
        self.batches = batches

    def to_batches(self):
        return self.batches


def _plans():
    li = q.MemoryTable.try_new(synth.LINEITEM_SCHEMA, synth.lineitem(200_000, 65_536))
    c, o, l = synth.q3_tables(0.05)
    q3 = queries.q3(q.MemoryTable.try_new(synth.CUSTOMER_SCHEMA, c), q.MemoryTable.try_new(synth.ORDERS_SCHEMA, o),
                    q.MemoryTable.try_new(synth.LINEITEM_Q3_SCHEMA, l))
    return queries.q1_full(li), q3


def _load(d):
    return {os.path.basename(f): np.load(f) for f in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_dump_outputs_float64_sorted_and_bounded(oracle, tmp_path, monkeypatch):
    q1, q3 = _plans()
    r1, r3 = oracle.execute(q1), oracle.execute(q3)
    bench.dump_outputs(str(tmp_path / "a"), {"q1": (q1, _Result(r1)), "q3": (q3, _Result(r3))})
    bench.dump_outputs(str(tmp_path / "b"), {"q1": (q1, _Result(r1[::-1])), "q3": (q3, _Result(r3[::-1]))})
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == [f"q1_{k:02d}_{f.name}.npy" for k, f in enumerate(q1.schema())] + [f"q3_{k:02d}_{f.name}.npy" for k, f in enumerate(q3.schema())]
    assert all(v.dtype == np.float64 for v in a.values())
    # the groups of a hash aggregate come in no fixed order: the dump does not depend on it
    assert all(np.array_equal(a[n], b[n], equal_nan=True) for n in a)
    rows = sorted((r["l_orderkey"], r["o_orderdate"], r["revenue"]) for t in r3 for r in t.to_pylist())
    assert a["q3_00_l_orderkey.npy"].tolist() == [float(k) for k, _, _ in rows]
    assert a["q3_03_revenue.npy"].tolist() == [float(v) for _, _, v in rows]
    keys = sorted((r["l_returnflag"], r["l_linestatus"]) for t in r1 for r in t.to_pylist())
    assert a["q1_00_l_returnflag.npy"].tolist() == [[float(ord(rf))] for rf, _ in keys]
    assert a["q1_01_l_linestatus.npy"].tolist() == [[float(ord(ls))] for _, ls in keys]
    # over the byte budget: the small result whole, a fixed seeded sample of the big one's sorted rows
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", (1 << 20) + 6000)
    bench.dump_outputs(str(tmp_path / "c"), {"q1": (q1, _Result(r1)), "q3": (q3, _Result(r3))})
    bench.dump_outputs(str(tmp_path / "d"), {"q1": (q1, _Result(r1)), "q3": (q3, _Result(r3[::-1]))})
    c, d = _load(tmp_path / "c"), _load(tmp_path / "d")
    assert sum(v.nbytes for v in c.values()) <= 6000
    assert np.array_equal(c["q1_09_count_order.npy"], a["q1_09_count_order.npy"])
    assert 0 < len(c["q3_00_l_orderkey.npy"]) < len(a["q3_00_l_orderkey.npy"])
    assert np.all(np.diff(c["q3_00_l_orderkey.npy"]) >= 0) and all(np.array_equal(c[n], d[n]) for n in c)


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--workload", "filter", "--dump-outputs", "x"]])
def test_bench_rejects_bad_arguments_before_touching_the_device(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "error" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(ctx, oracle, tmp_path):
    for name, extra in (("q1_full", ["--workload", "q1_full", "--rows", "300000"]), ("q3", ["--workload", "q3", "--sf", "0.05"])):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["higher_is_better"] is True and line["dtype"] == "i128" and line["unit"] == "rows/s"
        assert "records" not in line and "cpu_baseline" not in line and "roofline" not in line   # (--full's)
        # the arrays equal the oracle's result on the same synthetic inputs, dumped the same way
        if name == "q1_full":
            plan = queries.q1_full(q.MemoryTable.try_new(synth.LINEITEM_SCHEMA, [synth.lineitem_batch(0, 300_000)]))
        else:
            c, o, l = synth.q3_tables(0.05)
            plan = queries.q3(q.MemoryTable.try_new(synth.CUSTOMER_SCHEMA, c), q.MemoryTable.try_new(synth.ORDERS_SCHEMA, o),
                              q.MemoryTable.try_new(synth.LINEITEM_Q3_SCHEMA, l))
        bench.dump_outputs(str(tmp_path / f"want_{name}"), {name: (plan, _Result(oracle.execute(plan)))})
        got, want = _load(out), _load(tmp_path / f"want_{name}")
        assert sorted(got) == sorted(want) and len(got) == len(plan.schema())
        assert all(np.array_equal(got[n], want[n], equal_nan=True) for n in want), name
