#!/usr/bin/env python
"""Times the univariate round of the univariate-skip zerocheck (bn_zerocheck_univariate_evals, csrc/kernels_univariate.hip) and its
fold (bn_fold_right of every column at level 0 with the 2^k Lagrange query: evaluate_partial_low, prove/zerocheck.rs:384-434) at the
widths of the tables SURVEY names: keccak (204 one-bit columns of 2^(log_perms + 9) values, 100 constraints of degree 2; BASELINE
config 4 is 2^16 permutations) and u32_add (5 columns of 2^(log_rows + 5) values, constraints of degree 2 and 1), k = 7.

One JSON line per size: device-event times of the evaluations (batched output, as the prover asks for it) and of the fold, their
launches, and the counts the bounds come from -- bytes read (the columns once), GF(2) multiply-adds of the weighted sums in their
bit-plane Gram form (compositions x 8 bit-planes x points x 2^(n-k) x 128 bits), and each bound's least time: bytes at the 8 TB/s
HBM peak, multiply-adds at 5e15/s (the dense FP4 matrix rate, one multiply-add per FP4 MAC).  The columns and the indicator are
synthetic (on-device tensor expansions): the op's cost does not depend on the values.

  python tools/bench_univariate_skip.py [--log-perms 12 14 16] [--u32-log-rows 10] [--reps 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 8.0e12
GF2_MADDS_PER_S = 5.0e15


def measure(hal, name, n_vars, k, n_cols, comps, degrees, reps):
    from binius_amd import synthetic
    from bench_keccak_replay import device_random

    alloc = hal.dev_alloc()
    col_elems = max(1, (1 << n_vars) >> 7)
    cols = [(device_random(hal, alloc, 0x5A00 + i, n_vars - 7), 0) for i in range(n_cols)]
    eq = device_random(hal, alloc, 0x5B00, n_vars - k)
    D = max(degrees) << k
    alpha = synthetic.random_scalars(0x5C00, 1)[0]
    # the fold's query: 2^k values (the Lagrange coefficients L_u(z) in the prover; their values do not change the cost)
    query = device_random(hal, alloc, 0x5D00, k)
    folded = [alloc.alloc(col_elems) for _ in range(n_cols)] if k == 7 else []
    hal.zerocheck_univariate_evals(n_vars, k, cols, comps, degrees, eq, D, alpha)  # warm-up
    for (c, _), out in zip(cols, folded):
        hal.fold_right(c, 0, query, out)
    hal.sync()
    ev_ms, call_ms, fold_ms = [], [], []
    for _ in range(reps):
        hal.sync()
        hal.prof_begin()
        t0 = time.perf_counter()
        hal.zerocheck_univariate_evals(n_vars, k, cols, comps, degrees, eq, D, alpha)  # (returns after a stream synchronisation)
        call_ms.append(1e3 * (time.perf_counter() - t0))
        ev_ms.append(hal.prof_end()["round_eval"][0])  # the two kernels, between device events
        hal.timer_begin()
        for (c, _), out in zip(cols, folded):
            hal.fold_right(c, 0, query, out)
        fold_ms.append(hal.timer_end_ms())
    n_x = 1 << (n_vars - k)
    points = sum((d - 1) << k for d in degrees)
    col_bytes = n_cols * ((1 << n_vars) // 8)
    madds = 8 * points * n_x * 128
    ev, fo = min(ev_ms), min(fold_ms)
    return {
        "table": name, "n_vars": n_vars, "skip_rounds": k, "columns": n_cols, "compositions": len(comps), "max_domain_size": D,
        "evals_ms": ev, "evals_call_ms": min(call_ms), "fold_ms": fo, "evals_plus_fold_ms": ev + fo,
        "launches": {"evals": 2, "fold": len(folded)},
        "bytes_read": col_bytes, "gf2_madds": madds,
        "bound_ms": {"hbm": 1e3 * col_bytes / HBM_BYTES_PER_S, "gf2_fp4": 1e3 * madds / GF2_MADDS_PER_S},
        "share_of_bound": {"hbm": (1e3 * col_bytes / HBM_BYTES_PER_S) / ev, "gf2_fp4": (1e3 * madds / GF2_MADDS_PER_S) / ev},
        "reps": reps,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-perms", type=int, nargs="*", default=[12, 14, 16])
    ap.add_argument("--u32-log-rows", type=int, nargs="*", default=[10])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import binius_amd
    from bench_keccak_replay import table

    k = 7
    lines = []
    for name, sizes, cells in (("keccak", args.log_perms, 9), ("u32_add", args.u32_log_rows, 5)):
        t = table(name)
        comps = [s for s, _ in t["constraints"]]
        for lg in sizes:
            n_vars = lg + cells
            arena = t["n_z"] * 2 * max(1, (1 << n_vars) >> 7) + (1 << (n_vars - k)) + (1 << 20)
            with binius_amd.Context(0, arena) as hal:
                rec = measure(hal, name, n_vars, k, t["n_z"], comps, t["degrees"], args.reps)
            rec["log_size"] = lg
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
