"""Evalcheck's column projection on the device: (a) ONE bn_partial_eval_high_batch over all columns against (b) what the parent of
this change did with the same inputs -- one bn_fold_left per column on the fold_left kernels (BN_FOLD_LEFT_NO_PE=1 keeps bn_fold_left
off the new kernel for that leg; at these shapes that is k_fold: one thread per output, the whole reduction serial in it).  Shapes: 64
and 256 level-0 columns of 2^20 and 2^22 bits at b = 6 (keccak's shifted and packed B1 columns), 16 B64 columns of 2^16 elements at
b = 3.  JSON lines on stdout.

Both arms run in the same process on the same resident inputs, alternating run by run; a run is timed by the host clock and ends with
the device idle.  Reported: median, 10th and 90th percentile, the factor between the medians, the outputs compared bit for bit, the
launches of a batch call and the largest number of workgroups that shared a column (bn_partial_eval_counters), and the column bytes per
second of the batch call against 8 TB/s.

    python tools/bench_evalcheck.py [--runs 10] [--warmup 2] [--shapes 64:20:0:6,256:20:0:6,64:22:0:6,256:22:0:6,16:22:6:3]

A shape is n_cols:log2(bits of a column):tower_level:b."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import binius_amd  # noqa: E402
from binius_amd import synthetic  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
DEFAULT_SHAPES = "64:20:0:6,256:20:0:6,64:22:0:6,256:22:0:6,16:22:6:3"


def pct(xs):
    a = np.sort(np.asarray(xs))
    return {"median_us": round(float(np.median(a)) * 1e6, 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]) * 1e6, 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]) * 1e6, 2)}


def bench_shape(hal, n_cols, log_bits, level, b, runs, warmup):
    alloc = hal.dev_alloc()
    n_vars = log_bits - level
    q = n_vars - b
    elems = 1 << (log_bits - 7)
    vec = alloc.alloc(1 << q)
    hal.fill(vec.slice(0, 1), 1)
    hal.tensor_expand(0, synthetic.random_scalars(0xBE000 + q, q), vec)
    cols, outs_a, outs_b = [], [], []
    for t in range(n_cols):
        c = alloc.alloc(elems)
        hal.copy_h2d(synthetic.random_b128(0xBE100 + t, elems), c)
        cols.append((c, level, n_vars))
        outs_a.append(alloc.alloc(1 << b))
        outs_b.append(alloc.alloc(1 << b))

    def arm_batch():
        hal.partial_eval_high_batch(cols, vec, q, outs_a)
        hal.sync()

    def arm_per_column():
        os.environ["BN_FOLD_LEFT_NO_PE"] = "1"
        try:
            for (c, _, _), o in zip(cols, outs_b):
                hal.fold_left(c, level, vec, o)
            hal.sync()
        finally:
            del os.environ["BN_FOLD_LEFT_NO_PE"]

    ta, tb = [], []
    before = hal.partial_eval_counters()
    for r in range(warmup + runs):
        for arm, ts in ((arm_batch, ta), (arm_per_column, tb)):
            t0 = time.perf_counter()
            arm()
            dt = time.perf_counter() - t0
            if r >= warmup:
                ts.append(dt)
    now = hal.partial_eval_counters()
    same = all(np.array_equal(hal.copy_d2h(x), hal.copy_d2h(y)) for x, y in zip(outs_a, outs_b))
    a, p = pct(ta), pct(tb)
    col_bytes = n_cols * elems * 16
    return {
        "shape": {"n_cols": n_cols, "log2_bits": log_bits, "tower_level": level, "b": b, "query_vars": q, "column_bytes": col_bytes},
        "batch": a, "per_column_fold_left": p,
        "factor_median": round(p["median_us"] / a["median_us"], 2), "not_slower": a["median_us"] <= p["median_us"], "same_outputs": bool(same),
        "launches_per_batch_call": (now["launches"] - before["launches"]) // (warmup + runs),
        "fold_left_calls_routed": now["fold_left_routed"] - before["fold_left_routed"],
        "max_workgroups_sharing_a_column": now["max_share"],
        "column_bytes_per_s": round(col_bytes / (a["median_us"] * 1e-6), 1),
        "share_of_8TBps": round(col_bytes / (a["median_us"] * 1e-6) / HBM_BYTES_PER_S, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    args = ap.parse_args()
    with binius_amd.Context(0, 1 << 24) as hal:
        for spec in [s for s in args.shapes.split(",") if s]:
            n_cols, log_bits, level, b = (int(x) for x in spec.split(":"))
            print(json.dumps(bench_shape(hal, n_cols, log_bits, level, b, args.runs, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
