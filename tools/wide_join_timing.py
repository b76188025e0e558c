"""What the wide join key stage costs (csrc/join.cpp maybe_encode_wide_join_key): a build side of 200 k customers and a probe
side of 2 M rows joined (Inner) on (c_name, c_address, c_comment) — three Utf8 columns, c_comment up to 117 bytes — with
QHIP_JOIN_WIDE_KEYS=1, next to the same rows joined with the switch off on a precomputed Int64 surrogate of the key (the same
pairs: the floor the stage is added to). Per measurement: the median of --runs calls after warm-up, of the host's time for the
whole call (HIP events off) and of the device times (HIP events on: build_ms = the stage's memset + two kernels for the coded
join, the join's own key evaluation + table build for the surrogate; main_kernel_ms = the probe kernel); --repeat alternating
measurements of each, in one process.

    python tools/wide_join_timing.py [--build 200000] [--probe 2000000] [--runs 20] [--repeat 3]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402

import qurious_amd as q  # noqa: E402
from qurious_amd import JoinType  # noqa: E402

I64 = pa.int64()
BUILD = pa.schema([pa.field("c_id", I64), pa.field("c_name", pa.string()), pa.field("c_address", pa.string()), pa.field("c_comment", pa.string()),
                   pa.field("c_nation", I64)])
PROBE = pa.schema([pa.field("o_cid", I64), pa.field("o_name", pa.string()), pa.field("o_address", pa.string()), pa.field("o_comment", pa.string()),
                   pa.field("o_price", I64)])
WORDS = ["quickly", "ironic", "deposits", "blithely", "final", "furiously", "even", "pending", "carefully", "requests", "accounts", "sleep"]


def make_tables(n_build, n_probe, seed=1):
    """Two customers in a row share name and address and differ in the comment only; one probe row in ten names a customer the
    build side does not have."""
    rng = np.random.default_rng(seed)
    total = n_build + n_build // 4   # (the last fifth: keys only the probe side has)
    names, addresses, comments = [], [], []
    for g in range(total):
        c = g // 2
        names.append("Customer#%09d" % c)
        addresses.append(("%d Long Street, Springfield, Block %d" % (c, c % 97))[:40])
        comments.append(" ".join(WORDS[(c * 7 + j * 5) % len(WORDS)] for j in range(5 + c % 12))[:112] + " #%d" % (g % 2))
    keys = [pa.array(v, type=pa.string()) for v in (names, addresses, comments)]
    order = pa.array(rng.permutation(n_build), type=I64)
    build = pa.RecordBatch.from_arrays([order] + [k.take(order) for k in keys] + [pa.array(rng.integers(0, 25, n_build), type=I64)], schema=BUILD)
    pick = np.where(rng.random(n_probe) < 0.9, rng.integers(0, n_build, n_probe), rng.integers(n_build, total, n_probe))
    pick = pa.array(pick, type=I64)
    probe = pa.RecordBatch.from_arrays([pick] + [k.take(pick) for k in keys] + [pa.array(rng.integers(0, 10**6, n_probe), type=I64)], schema=PROBE)
    step = 1 << 20
    return (q.MemoryTable.try_new(BUILD, [build]), q.MemoryTable.try_new(PROBE, [probe.slice(a, min(step, n_probe - a)) for a in range(0, n_probe, step)]),
            max(len(c) for c in comments))


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
    build, probe, total = [], [], []
    for _ in range(runs):
        plan.execute_device()
        st = ctx.last_stats()
        build.append(st["build_ms"])
        probe.append(st["main_kernel_ms"])
        total.append(st["total_device_ms"])
    ctx.set_timing(False)
    return out.num_rows, statistics.median(wall), statistics.median(build), statistics.median(probe), statistics.median(total), st["main_kernel_name"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", type=int, default=200_000)
    ap.add_argument("--probe", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    bt, pt, longest = make_tables(args.build, args.probe)
    left, right = q.Scan(BUILD, bt, None, None), q.Scan(PROBE, pt, None, None)
    wide = q.HashJoinExec.try_new(left, right, JoinType.Inner, [(q.Column("c_name", 1), q.Column("o_name", 1)), (q.Column("c_address", 2), q.Column("o_address", 2)),
                                                                (q.Column("c_comment", 3), q.Column("o_comment", 3))], None)
    surrogate = q.HashJoinExec.try_new(left, right, JoinType.Inner, [(q.Column("c_id", 0), q.Column("o_cid", 0))], None)
    ctx = q.get_context()
    print(f"device {ctx.device_name()} build rows {args.build} probe rows {args.probe} longest c_comment {longest} bytes; median of {args.runs} calls "
          f"after 5 warm-up calls", flush=True)
    for rep in range(args.repeat):
        for name, plan, mode in (("three Utf8 keys, QHIP_JOIN_WIDE_KEYS=1", wide, "1"), ("Int64 surrogate, QHIP_JOIN_WIDE_KEYS=0", surrogate, "0")):
            os.environ["QHIP_JOIN_WIDE_KEYS"] = mode
            before = ctx.wide_key_joins()
            rows, wall, build, probe, total, kname = measure(ctx, plan, args.runs)
            took = ctx.wide_key_joins() - before
            what = "encoding stage (memset + 2 kernels)" if took else "join's own key evaluation + build  "
            print(f"run {rep + 1} {name:40s} pairs {rows:8d} whole call {wall:8.3f} ms  {what} {build * 1e3:8.1f} us = {build * 1e6 / args.probe:6.3f} ns/probe row  "
                  f"join behind it, first launch .. last {total:7.3f} ms  probe kernel {probe:7.3f} ms ({kname})  calls through the stage {took}", flush=True)


if __name__ == "__main__":
    main()
