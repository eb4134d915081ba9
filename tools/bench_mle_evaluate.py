"""The evaluations in front of an evalcheck round on the device: (A) ONE bn_mle_evaluate_batch over all columns against (B) the best
route the parent of this change had for the same inputs -- bn_partial_eval_high_batch at a 10-variable split (one call per point), then
one bn_inner_product per column of its 2^10 partial evaluations against the table of the low coordinates.  Shapes: 64 and 256 B1 columns
of 2^20 and 2^22 bits at one point, 16 B32 columns of 2^18 elements, 200 B1 columns of 2^22 bits spread over three points.  JSON lines on
stdout.

Arm A runs once per split bound S of --lo-splits (the low part of a point has min(n_vars // 2, S) coordinates): the sweep that picks
BNH_EVALCHECK_LO_SPLIT.  All arms run in the same process on the same resident inputs, alternating run by run; a run is timed by the
host clock and ends with the device idle (arm A returns with its results, arm B's last call is an inner product that returns with its
result).  Arm A's job and point tables are built once, outside the timed region, as a compiled caller holds them; arm B goes through
the same ctypes binding call by call.  Reported: median, 10th and 90th percentile per arm, the factor between the medians of B and of A
at --report-split, the evaluations compared bit for bit across all arms, the launches of a batch call, the largest number of workgroups
that shared a job, and the column bytes per second of the batch call against 8 TB/s.

    python tools/bench_mle_evaluate.py [--runs 10] [--warmup 2] [--lo-splits 6,8,10] [--report-split 8]
                                       [--shapes 64:20:0:1,256:20:0:1,64:22:0:1,256:22:0:1,16:23:5:1,200:22:0:3]

A shape is n_cols:log2(bits of a column):tower_level:n_points."""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import binius_amd  # noqa: E402
from binius_amd import _ffi as F  # noqa: E402
from binius_amd import synthetic  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
DEFAULT_SHAPES = "64:20:0:1,256:20:0:1,64:22:0:1,256:22:0:1,16:23:5:1,200:22:0:3"
PARENT_SPLIT = 10


def pct(xs):
    a = np.sort(np.asarray(xs))
    return {"median_us": round(float(np.median(a)) * 1e6, 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]) * 1e6, 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]) * 1e6, 2)}


def expansion(hal, alloc, coords):
    t = alloc.alloc(1 << len(coords))
    hal.fill(t.slice(0, 1), 1)
    if coords:
        hal.tensor_expand(0, list(coords), t)
    return t


def bench_shape(hal, n_cols, log_bits, level, n_points, splits, report_split, runs, warmup):
    alloc = hal.dev_alloc()
    n_vars = log_bits - level
    elems = 1 << (log_bits - 7)
    coords = [synthetic.random_scalars(0xBF000 + 64 * p + n_vars, n_vars) for p in range(n_points)]
    cols = []
    for t in range(n_cols):
        c = alloc.alloc(elems)
        hal.copy_h2d(synthetic.random_b128(0xBF100 + t, elems), c)
        cols.append(c)
    point_of = [t % n_points for t in range(n_cols)]

    # ---- arm A, one per split: the tables of a call, built once
    arms, results = [], {}
    for s in splits:
        lo = min(n_vars // 2, s)
        pts = [(expansion(hal, alloc, cs[:lo]), lo, expansion(hal, alloc, cs[lo:]), n_vars - lo) for cs in coords]
        d_pts = (F.MePoint * n_points)(*[F.MePoint(p[0].ptr, p[2].ptr, p[1], p[3]) for p in pts])
        d_jobs = (F.MeJob * n_cols)(*[F.MeJob(c.ptr, level, n_vars, point_of[t], 0) for t, c in enumerate(cols)])
        out = (F.F128 * n_cols)()
        name = "batch_S%d" % s
        results[name] = out

        def arm_batch(d_jobs=d_jobs, d_pts=d_pts, out=out, keep=pts):
            rc = F.lib().bn_mle_evaluate_batch(hal._h, C.cast(d_jobs, C.c_void_p), n_cols, C.cast(d_pts, C.c_void_p), n_points, out)
            assert rc == 0, F.lib().bn_last_error()

        arms.append((name, arm_batch))

    # ---- arm B: per point one partial evaluation call at the 10-variable split, per column one inner product
    b = min(PARENT_SPLIT, n_vars)
    tabs = [(expansion(hal, alloc, cs[:b]), expansion(hal, alloc, cs[b:])) for cs in coords]
    partial = [alloc.alloc(1 << b) for _ in cols]
    out_b = [0] * n_cols

    def arm_parent():
        for p in range(n_points):
            idx = [t for t in range(n_cols) if point_of[t] == p]
            hal.partial_eval_high_batch([(cols[t], level, n_vars) for t in idx], tabs[p][1], n_vars - b, [partial[t] for t in idx])
        for t in range(n_cols):
            out_b[t] = hal.inner_product(partial[t], 7, tabs[point_of[t]][0])

    arms.append(("parent_route", arm_parent))
    times = {name: [] for name, _ in arms}
    before = hal.mle_evaluate_counters()
    for r in range(warmup + runs):
        for name, arm in arms:
            t0 = time.perf_counter()
            arm()
            dt = time.perf_counter() - t0
            if r >= warmup:
                times[name].append(dt)
    now = hal.mle_evaluate_counters()
    same = all([F.from_f128(out[t]) for t in range(n_cols)] == out_b for out in results.values())
    stats = {name: pct(ts) for name, ts in times.items()}
    a, p = stats["batch_S%d" % report_split], stats["parent_route"]
    col_bytes = n_cols * elems * 16
    batch_calls = (warmup + runs) * len(splits)
    return {
        "shape": {"n_cols": n_cols, "log2_bits": log_bits, "tower_level": level, "n_vars": n_vars, "n_points": n_points, "column_bytes": col_bytes},
        "arms": stats, "report_split": report_split,
        "factor_median": round(p["median_us"] / a["median_us"], 2), "not_slower": a["median_us"] <= p["median_us"], "same_outputs": bool(same),
        "launches_per_batch_call": (now["launches"] - before["launches"]) / batch_calls,
        "max_workgroups_sharing_a_job_last_call": now["max_share"],
        "column_bytes_per_s": round(col_bytes / (a["median_us"] * 1e-6), 1),
        "share_of_8TBps": round(col_bytes / (a["median_us"] * 1e-6) / HBM_BYTES_PER_S, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lo-splits", default="6,8,10")
    ap.add_argument("--report-split", type=int, default=8)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    args = ap.parse_args()
    splits = [int(x) for x in args.lo_splits.split(",") if x]
    assert args.report_split in splits
    with binius_amd.Context(0, 1 << 24) as hal:
        for spec in [s for s in args.shapes.split(",") if s]:
            n_cols, log_bits, level, n_points = (int(x) for x in spec.split(":"))
            print(json.dumps(bench_shape(hal, n_cols, log_bits, level, n_points, splits, args.report_split, args.runs, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
