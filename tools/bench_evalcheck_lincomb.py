"""Evalcheck's projection of linear-combination inner columns at keccak's theta shape: c[x], x < 5, each the sum of five B1 state
columns of 2^22 bits, projected at b = 6 (64 outputs under 2^16 rows).  Three legs on the same resident inputs in one process:

  (a) lincomb        ONE bn_partial_eval_high_lincomb_batch: five jobs of five coefficient-ONE terms (five row loops planned)
  (b) parts_on_host  what a caller could do before: ONE bn_partial_eval_high_batch over the 25 columns (25 row loops), one copy of the 25
                     tables to the host, the XOR there
  (c) materialised   the floor: ONE bn_partial_eval_high_batch over five columns that already hold the sums (materialised outside the
                     timed region -- the full-size temporaries the new op exists to avoid)

The argument tables of all three legs are built once, outside the timed region, and the legs call the C entry points on them: what is
timed is the library, not the construction of Python objects (25 terms against 5 columns).  The legs alternate run by run; a run is
`--reps` calls back to back, timed by the host clock, and ends with the device idle ((a) and (c) return with their outputs complete, (b)
ends in its copy).  Reported per leg: median, 10th and 90th percentile of the time of one call;
the factors (b)/(a) and (a)/(c); the three results compared bit for bit; the counters of the new op.  One JSON line on stdout.

    python tools/bench_evalcheck_lincomb.py [--runs 30] [--warmup 3] [--reps 10] [--log-bits 22] [--b 6]"""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import binius_amd  # noqa: E402
from binius_amd import synthetic  # noqa: E402
from binius_amd._ffi import F128, PeColumn, PelJob, PelTerm, _check, lib  # noqa: E402

N_JOBS, N_TERMS = 5, 5


def pct(xs):
    a = np.sort(np.asarray(xs))
    return {"median_us": round(float(np.median(a)) * 1e6, 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]) * 1e6, 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]) * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--log-bits", type=int, default=22)
    ap.add_argument("--b", type=int, default=6)
    args = ap.parse_args()
    n_vars, b = args.log_bits, args.b
    q, elems, out_len = n_vars - b, 1 << (args.log_bits - 7), 1 << b
    with binius_amd.Context(0, 1 << 23) as hal:
        alloc = hal.dev_alloc()
        vec = alloc.alloc(1 << q)
        hal.fill(vec.slice(0, 1), 1)
        hal.tensor_expand(0, synthetic.random_scalars(0xBF000 + q, q), vec)
        state, sums = [], []
        for x in range(N_JOBS):
            acc = np.zeros((elems, 2), dtype=np.uint64)
            for y in range(N_TERMS):
                data = synthetic.random_b128(0xBF100 + N_TERMS * x + y, elems)
                acc ^= data
                c = alloc.alloc(elems)
                hal.copy_h2d(data, c)
                state.append(c)
            s = alloc.alloc(elems)
            hal.copy_h2d(acc, s)
            sums.append(s)
        ptrs = lambda slices: (C.c_void_p * len(slices))(*[s.ptr for s in slices])
        jobs = (PelJob * N_JOBS)(*[PelJob(n_vars, N_TERMS * x, N_TERMS, 0, F128(0, 0)) for x in range(N_JOBS)])
        terms = (PelTerm * len(state))(*[PelTerm(c.ptr, 0, 0, F128(1, 0)) for c in state])
        cols_b = (PeColumn * len(state))(*[PeColumn(c.ptr, 0, n_vars) for c in state])
        cols_c = (PeColumn * len(sums))(*[PeColumn(s.ptr, 0, n_vars) for s in sums])
        outs_a = [alloc.alloc(out_len) for _ in range(N_JOBS)]
        parts = alloc.alloc(N_JOBS * N_TERMS * out_len)  # (contiguous: one copy brings all 25 tables back)
        outs_b = [parts.slice(t * out_len, (t + 1) * out_len) for t in range(N_JOBS * N_TERMS)]
        outs_c = [alloc.alloc(out_len) for _ in range(N_JOBS)]
        p_a, p_b, p_c = ptrs(outs_a), ptrs(outs_b), ptrs(outs_c)
        host_b = [None]

        def leg_a():
            _check(lib().bn_partial_eval_high_lincomb_batch(hal._h, C.cast(jobs, C.c_void_p), N_JOBS, C.cast(terms, C.c_void_p), len(state), vec.ptr, q, p_a))

        def leg_b():
            _check(lib().bn_partial_eval_high_batch(hal._h, C.cast(cols_b, C.c_void_p), len(state), vec.ptr, q, p_b))
            tables = hal.copy_d2h(parts).reshape(N_JOBS, N_TERMS, out_len, 2)
            host_b[0] = np.bitwise_xor.reduce(tables, axis=1)

        def leg_c():
            _check(lib().bn_partial_eval_high_batch(hal._h, C.cast(cols_c, C.c_void_p), len(sums), vec.ptr, q, p_c))

        legs = (("lincomb", leg_a), ("parts_on_host", leg_b), ("materialised", leg_c))
        times = {name: [] for name, _ in legs}
        before = hal.partial_eval_lincomb_counters()
        for r in range(args.warmup + args.runs):
            for name, leg in legs:
                hal.sync()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    leg()
                hal.sync()
                dt = (time.perf_counter() - t0) / args.reps
                if r >= args.warmup:
                    times[name].append(dt)
        now = hal.partial_eval_lincomb_counters()
        calls = now["calls"] - before["calls"]
        got_a = np.stack([hal.copy_d2h(o) for o in outs_a])
        got_c = np.stack([hal.copy_d2h(o) for o in outs_c])
        res = {name: pct(ts) for name, ts in times.items()}
        a, p, c = res["lincomb"]["median_us"], res["parts_on_host"]["median_us"], res["materialised"]["median_us"]
        col_bytes = N_JOBS * N_TERMS * elems * 16
        print(json.dumps({
            "shape": {"jobs": N_JOBS, "terms_per_job": N_TERMS, "log2_bits": args.log_bits, "tower_level": 0, "b": b, "query_vars": q, "column_bytes_read_by_a": col_bytes},
            "runs": args.runs, "warmup": args.warmup, "calls_per_run": args.reps,
            **res,
            "parts_on_host_over_lincomb": round(p / a, 3), "lincomb_over_materialised": round(a / c, 3), "lincomb_beats_parts_on_host": a < p,
            "same_outputs": bool(np.array_equal(got_a, host_b[0]) and np.array_equal(got_a, got_c)),
            "lincomb_counters_per_call": {k: (now[k] - before[k]) // calls for k in ("launches", "jobs", "terms", "classes", "jobs_fallback")},
            "max_workgroups_sharing_a_job": now["max_share"],
            "column_bytes_per_s_of_a": round(col_bytes / (a * 1e-6), 1),
        }), flush=True)


if __name__ == "__main__":
    main()
