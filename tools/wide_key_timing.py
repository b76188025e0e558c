"""What the wide-key encoding stage costs (csrc/agg.cpp maybe_encode_wide_key): a Q10-shaped table — GROUP BY c_custkey, c_name,
c_acctbal, c_phone, n_name, c_address, c_comment (seven columns, c_comment up to 117 bytes), SUM / COUNT / MIN / MAX — of
2 M rows and about 200 k groups, aggregated with QHIP_AGG_WIDE_KEYS=1, next to the same rows aggregated with the switch off on
c_custkey alone (a third of the groups) and on a precomputed Int64 group number (the same groups: what the aggregate behind the
stage costs by itself). Per measurement: the median of --runs calls after warm-up, of the host's time for the whole call (HIP
events off) and of the kernel times (HIP events on: build_ms = the stage's memset + kernel, main_kernel_ms = the aggregate
kernel); --repeat alternating measurements of each.

    python tools/wide_key_timing.py [--rows 2000000] [--groups 200000] [--runs 20] [--repeat 3]
"""
import argparse
import decimal
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402

import qurious_amd as q  # noqa: E402
from qurious_amd import ScalarValue as S  # noqa: E402

I64, DEC = pa.int64(), pa.decimal128(15, 2)
SCHEMA = pa.schema([pa.field("c_custkey", I64), pa.field("c_name", pa.string()), pa.field("c_acctbal", DEC), pa.field("c_phone", pa.string()),
                    pa.field("n_name", pa.string()), pa.field("c_address", pa.string()), pa.field("c_comment", pa.string()),
                    pa.field("revenue", DEC), pa.field("qty", I64), pa.field("gid", I64)])
NATIONS = ["ALGERIA", "UNITED KINGDOM", "SAUDI ARABIA", "UNITED STATES", "MOZAMBIQUE", "RUSSIAN FEDERATION", "CHINA", "PERU"]
WORDS = ["quickly", "ironic", "deposits", "blithely", "final", "furiously", "even", "pending", "carefully", "requests", "accounts", "sleep"]


def make_table(n, n_groups, seed=1):
    """Three keys in a row share c_custkey .. c_address and differ in c_comment only."""
    rng = np.random.default_rng(seed)
    keys = [[] for _ in range(7)]
    for g in range(n_groups):
        c = g // 3
        comment = " ".join(WORDS[(c * 7 + j * 5) % len(WORDS)] for j in range(5 + c % 12))[:110] + " #%d" % (g % 3)
        row = (c, "Customer#%09d" % c, decimal.Decimal(c * 37 % 1100000 - 100000).scaleb(-2), "%02d-%03d-%03d-%04d" % (c % 25 + 10, c % 1000, c * 7 % 1000, c % 10000),
               NATIONS[c % len(NATIONS)], ("%d Long Street, Springfield, Block %d" % (c, c % 97))[:40], comment)
        for k in range(7):
            keys[k].append(row[k])
    pick = pa.array(rng.integers(0, n_groups, n), type=I64)
    cols = [pa.array(keys[k], type=SCHEMA.field(k).type).take(pick) for k in range(7)]
    words = np.zeros((n, 2), dtype=np.int64)   # (non-negative Decimal128 values: low word, zero high word)
    words[:, 0] = rng.integers(0, 10**7, n)
    cols.append(pa.Array.from_buffers(DEC, n, [None, pa.py_buffer(words.tobytes())]))
    cols.append(pa.array(rng.integers(1, 51, n), type=I64))
    cols.append(pick)
    batch = pa.RecordBatch.from_arrays(cols, schema=SCHEMA)
    step = 1 << 20
    return q.MemoryTable.try_new(SCHEMA, [batch.slice(a, min(step, n - a)) for a in range(0, n, step)])


def measure(ctx, plan, runs):
    for _ in range(5):
        plan.execute_device()
    ctx.synchronize()
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = plan.execute_device()
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.set_timing(True)
    stage, main = [], []
    for _ in range(runs):
        plan.execute_device()
        st = ctx.last_stats()
        stage.append(st["build_ms"])
        main.append(st["main_kernel_ms"])
    ctx.set_timing(False)
    return out.num_rows, statistics.median(wall), statistics.median(stage), statistics.median(main), st["main_kernel_name"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--groups", type=int, default=200_000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    table = make_table(args.rows, args.groups)
    scan = q.Scan(SCHEMA, table, None, None)
    aggs = [q.SumAggregateExpr(q.Column("revenue", 7), DEC), q.CountAggregateExpr(q.Literal(S.Int64(1))), q.MinAggregateExpr(q.Column("qty", 8), I64),
            q.MaxAggregateExpr(q.Column("qty", 8), I64)]
    wide = q.HashAggregate(None, scan, [q.Column(f.name, k) for k, f in enumerate(SCHEMA)][:7], aggs)
    narrow = q.HashAggregate(None, scan, [q.Column("c_custkey", 0)], aggs)
    by_gid = q.HashAggregate(None, scan, [q.Column("gid", 9)], aggs)
    ctx = q.get_context()
    print(f"device {ctx.device_name()} rows {args.rows} median of {args.runs} calls after 5 warm-up calls", flush=True)
    for rep in range(args.repeat):
        for name, plan, mode in (("seven keys, QHIP_AGG_WIDE_KEYS=1", wide, "1"), ("c_custkey alone, QHIP_AGG_WIDE_KEYS=0", narrow, "0"),
                                 ("group number, QHIP_AGG_WIDE_KEYS=0", by_gid, "0")):
            os.environ["QHIP_AGG_WIDE_KEYS"] = mode
            before = ctx.wide_key_aggregates()
            groups, wall, stage, kern, kname = measure(ctx, plan, args.runs)
            took = ctx.wide_key_aggregates() - before
            print(f"run {rep + 1} {name:38s} groups {groups:7d} whole call {wall:8.3f} ms  encoding stage (memset + kernel) {stage:7.3f} ms = "
                  f"{stage * 1e6 / args.rows:6.3f} ns/row  aggregate kernel {kern:7.3f} ms ({kname})  calls through the stage {took}", flush=True)


if __name__ == "__main__":
    main()
