"""What EXTRACT costs inside the fused aggregate: main_kernel_ms of two queries over synthetic lineitem (SF10 = 60 M rows by
default), each against a baseline that needs nothing new, so that this script runs unchanged on a tree without EXTRACT.

  (a) Q1's aggregate list  WHERE EXTRACT(YEAR FROM l_shipdate) = 1995          baseline: l_shipdate >= 1995-01-01 AND < 1996-01-01
  (b) SUM(l_extendedprice) GROUP BY EXTRACT(YEAR FROM l_shipdate)              baseline: GROUP BY a precomputed Int64 year column

    python tools/extract_timing.py [--baseline] [--rows N] [--runs 20] [--isa]

Prints one line per query: the median, min and max of --runs executions after warm-up. --isa (no GPU needed): VGPRs, SGPR
spills and waves per SIMD of the fused aggregate kernel of all four queries, compiled from the plan-only sources (column
statistics unknown there, so the runtime kernel may read narrower copies of the decimal columns).
"""
import argparse
import glob
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402

import qurious_amd as q  # noqa: E402
from qurious_amd import Operator, queries, synth  # noqa: E402
from qurious_amd import ScalarValue as S  # noqa: E402

SCHEMA = synth.LINEITEM_SCHEMA.append(pa.field("l_year", pa.int64(), False))
DEC = pa.decimal128(15, 2)


def _date(s):
    return q.CastExpr(q.Literal(S.Utf8(s)), pa.date32())


def plans(table, baseline):
    ship = q.Column("l_shipdate", 0)
    year = q.Column("l_year", 7) if baseline else q.Function(q.DatetimeExtract(), [q.Literal(S.Utf8("YEAR")), ship])
    if baseline:
        pred = q.BinaryExpr(q.BinaryExpr(ship, Operator.GtEq, _date("1995-01-01")), Operator.And, q.BinaryExpr(ship, Operator.Lt, _date("1996-01-01")))
    else:
        pred = q.BinaryExpr(year, Operator.Eq, q.Literal(S.Int64(1995)))
    full = queries.q1_full(table)
    a = q.HashAggregate(None, q.Scan(SCHEMA, table, None, pred), full.group_exprs, full.aggregate_exprs)
    b = q.HashAggregate(None, q.Scan(SCHEMA, table, None, None), [year], [q.SumAggregateExpr(q.Column("l_extendedprice", 4), DEC)])
    return {"a_filter_year": (a, pred), "b_group_year": (b, None)}


def isa(baseline_too=True):
    from isa_stats import kernels_of, waves_per_simd
    from qurious_amd import planning
    for bl in ([False, True] if baseline_too else [False]):
        for name, (plan, pred) in plans(None, bl).items():
            src = planning.aggregate_source(SCHEMA, pred, plan.group_exprs, plan.aggregate_exprs)
            with tempfile.TemporaryDirectory() as d:
                planning.compile_to_cache(src, d)
                for obj in glob.glob(os.path.join(d, "*.hsaco")):
                    for kname, k in kernels_of(obj):
                        if kname.startswith("qk_filter_agg"):
                            print(f"isa {'baseline' if bl else 'extract '} {name:14s} {kname:22s} vgprs {k['vgpr_count']:4d} "
                                  f"sgpr_spills {k.get('sgpr_spill_count', 0):3d} waves_per_simd {waves_per_simd(k['vgpr_count'], k['agpr_count'])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--rows", type=float, default=60e6)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--isa", action="store_true")
    args = ap.parse_args()
    if args.isa:
        isa()
        return
    n = int(args.rows)
    batches = []
    for b in synth.lineitem(n):
        days = np.asarray(b.column(0).cast(pa.int32())).astype("datetime64[D]")
        years = days.astype("datetime64[Y]").astype(np.int64) + 1970
        batches.append(pa.RecordBatch.from_arrays(list(b.columns) + [pa.array(years, type=pa.int64())], schema=SCHEMA))
    table = q.MemoryTable.try_new(SCHEMA, batches)
    ctx = q.get_context()
    ctx.set_timing(True)
    for name, (plan, _) in plans(table, args.baseline).items():
        for _ in range(5):
            plan.execute_device()
        ms = []
        for _ in range(args.runs):
            out = plan.execute_device()
            ms.append(ctx.last_stats()["main_kernel_ms"])
        ctx.synchronize()
        print(f"{'baseline' if args.baseline else 'extract '} {name:14s} rows {n} groups {out.num_rows:3d} main_kernel_ms median {statistics.median(ms):.4f} "
              f"min {min(ms):.4f} max {max(ms):.4f} (n={len(ms)}) kernel {ctx.last_stats()['main_kernel_name']}", flush=True)


if __name__ == "__main__":
    main()
