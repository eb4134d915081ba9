#!/usr/bin/env python
"""bn_derive_columns_batch on one MI355X beside the two things it is compared with, in one process:

  derive   ONE call that derives every column of the set (plan, table upload, launch and the call's own synchronisation are in it)
  copy     a bn_copy_d2d that moves the same number of bytes as the derive call reads and writes: the yardstick for a streaming kernel
  upload   a bn_copy_h2d of the derived columns' bytes from host memory: the step the op replaces (fill on the host, then this)

Two column sets:

  keccak   B1 columns at the shape of the keccak gadget (m3/src/gadgets/hash/keccak/stacked.rs: rotations of 64-bit words and the
           five-term c[x] sums): 25 given columns of 2^24 bits and 5 of 2^25; derived from them 70 + 10 CircularLeft rotations in
           64-bit blocks (offsets 1 .. 63) and 20 five-term XORs -- 100 columns in one call
  b32      B32 columns of 2^19 values: 8 shifts in blocks of 16 values (all three variants), 4 three-term XORs, 2 repeated and 2
           zero-padded columns -- 16 columns in one call

Every figure: warm-up runs, then the median of the timed runs (host clock between two synchronisations), with min, max and the
interquartile range.  One JSON line per set.

  python tools/bench_derive.py [--runs 15] [--out profiles/r22/derive.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_keccak_replay import device_random  # noqa: E402


def stats(ms):
    ms = sorted(ms)
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [ms[0], ms[len(ms) // 2], ms[-1]]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "iqr_ms": round(q[2] - q[0], 4), "runs": len(ms)}


def timed(hal, fn, runs, warmup=3):
    out = []
    for it in range(warmup + runs):
        hal.sync()
        t0 = time.perf_counter()
        fn()
        hal.sync()
        if it >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def keccak_set(hal, alloc):
    """(jobs, elements read, elements written)"""
    small = [device_random(hal, alloc, 100 + i, 17) for i in range(25)]  # 2^24 bits = 2^17 elements
    large = [device_random(hal, alloc, 200 + i, 18) for i in range(5)]
    jobs, read, written = [], 0, 0
    for i in range(70):
        jobs.append({"kind": "shifted", "level": 0, "n_vars": 24, "inner": small[i % 25], "block_size": 6, "shift_offset": 1 + (11 * i) % 63, "variant": "circular_left",
                     "out": alloc.alloc(1 << 17)})
        read, written = read + (1 << 17), written + (1 << 17)
    for i in range(10):
        jobs.append({"kind": "shifted", "level": 0, "n_vars": 25, "inner": large[i % 5], "block_size": 6, "shift_offset": 1 + (7 * i) % 63, "variant": "circular_left",
                     "out": alloc.alloc(1 << 18)})
        read, written = read + (1 << 18), written + (1 << 18)
    for i in range(20):
        jobs.append({"kind": "xor", "level": 0, "n_vars": 24, "terms": [small[(i + 5 * y) % 25] for y in range(5)], "offset": 0, "out": alloc.alloc(1 << 17)})
        read, written = read + 5 * (1 << 17), written + (1 << 17)
    return jobs, read, written


def b32_set(hal, alloc):
    n_vars, el = 19, 1 << 17  # 2^19 values of 32 bits = 2^17 elements
    given = [device_random(hal, alloc, 300 + i, 17) for i in range(6)]
    short = device_random(hal, alloc, 310, 10)  # 2^12 values
    jobs, read, written = [], 0, 0
    for i in range(8):
        jobs.append({"kind": "shifted", "level": 5, "n_vars": n_vars, "inner": given[i % 6], "block_size": 4, "shift_offset": 1 + (5 * i) % 15,
                     "variant": ("circular_left", "logical_left", "logical_right")[i % 3], "out": alloc.alloc(el)})
        read, written = read + el, written + el
    for i in range(4):
        jobs.append({"kind": "xor", "level": 5, "n_vars": n_vars, "terms": [given[(i + y) % 6] for y in range(3)], "offset": 0x9E3779B9, "out": alloc.alloc(el)})
        read, written = read + 3 * el, written + el
    for i in range(2):
        jobs.append({"kind": "repeating", "level": 5, "n_vars": n_vars, "inner": short, "inner_n_vars": 12, "out": alloc.alloc(el)})
        read, written = read + (1 << 10), written + el
    for i in range(2):
        jobs.append({"kind": "zero_padded", "level": 5, "n_vars": n_vars, "inner": short, "inner_n_vars": 12, "start_index": 6 * i, "nonzero_index": 77,
                     "out": alloc.alloc(el)})
        read, written = read + (1 << 10), written + el
    return jobs, read, written


def measure(hal, np, name, make, runs):
    alloc = hal.dev_alloc()
    jobs, read, written = make(hal, alloc)
    moved = read + written  # elements the call reads and writes, as counted from the shapes
    src, dst = alloc.alloc(moved // 2), alloc.alloc(moved // 2)  # a copy of n elements moves 2 n
    hal.fill(src, 3)
    host = np.frombuffer(np.random.default_rng(1).bytes(16 * written), dtype=np.uint64).reshape(written, 2)
    up = alloc.alloc(written)
    step = 1 << 22

    def upload():
        for off in range(0, written, step):
            hal.copy_h2d(host[off:off + step], up.slice(off, min(written, off + step)))

    table = hal.derive_job_table(jobs)  # marshalled once: the timed call is the C entry point, not the Python that fills its structs
    c0 = hal.derive_counters()
    derive = timed(hal, lambda: hal.derive_columns_raw(*table), runs)
    c1 = hal.derive_counters()
    copy = timed(hal, lambda: hal.copy_d2d(src, dst), runs)
    derive2 = timed(hal, lambda: hal.derive_columns_raw(*table), runs)  # again behind the copy: the two windows bracket it
    h2d = timed(hal, upload, max(5, runs // 3), warmup=1)
    d, c, u = stats(derive + derive2), stats(copy), stats(h2d)
    return {"set": name, "jobs": len(jobs), "launches_per_call": (c1["launches"] - c0["launches"]) // (c1["calls"] - c0["calls"]), "bytes_read": 16 * read,
            "bytes_written": 16 * written, "derive": d, "derive_first_window": stats(derive), "derive_second_window": stats(derive2), "copy_same_bytes": c,
            "upload_derived_bytes": u, "derive_over_copy": round(d["median_ms"] / c["median_ms"], 3), "upload_over_derive": round(u["median_ms"] / d["median_ms"], 2),
            "derive_TBps": round(16 * moved / d["median_ms"] / 1e9, 3), "copy_TBps": round(16 * moved / c["median_ms"] / 1e9, 3),
            "upload_GBps": round(16 * written / u["median_ms"] / 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np

    import binius_amd

    lines = []
    with binius_amd.Context(0, 80 << 20) as hal:  # elements: both sets' columns, the copy's two buffers, the upload's destination
        for name, make in (("keccak", keccak_set), ("b32", b32_set)):
            rec = measure(hal, np, name, make, args.runs)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
