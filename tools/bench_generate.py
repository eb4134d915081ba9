#!/usr/bin/env python
"""bn_generate_columns_batch on one MI355X beside the three things it is compared with, in one process.

The workload is what a table of 2^20 rows needs beside its committed columns, in ONE call:

  bits      the 32 add_selected bit columns of a B1 column with 32 values per row (2^25 bits): bit j of every 32-bit word, 2^20 bits each
  step      one step-down selector of 2^20 bits
  incr      one B32 incrementing column of 2^20 values
  const     one B32 constant column of 2^20 values
  powers    one B64 column of the powers of the field's generator, 2^20 values

and the comparisons

  generate      the call (plan, table upload, launch and the call's own synchronisation are in it)
  host_fill     (a) the same columns filled with numpy on the host -- every column but the powers, which numpy has no product for: that
                column's fill is NOT in the figure --
  upload        ... and a bn_copy_h2d of all the columns' bytes: (a) is host_fill + upload
  copy_out      (b) a bn_copy_d2d of the output byte count
  copy_in_out   (c) a bn_copy_d2d that moves the input plus the output byte count: the projection's real floor, with the inner column
                counted once per job that reads it

then the same figures for the parts of the call alone (the 32 bit columns; the three fills; the powers) and for ONE projection of
2^21 bits out of a 2^26-bit inner column in each regime of the kernel (runs of whole elements; one run per input element; several runs
per input element), each against its own copies (b) and (c).

Every figure: 3 warm-up runs, then the median of the timed runs (host clock between two synchronisations), with min, max and the
interquartile range.  One JSON line per record.

  python tools/bench_generate.py [--runs 20] [--out profiles/r23/generate.jsonl]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_derive import stats, timed  # noqa: E402
from bench_keccak_replay import device_random  # noqa: E402

ROWS = 20  # log2 of the table's rows
B64_GENERATOR = 0x070F870DCD9C1D88


def elems(level, n_vars):
    return 1 << (n_vars + level - 7)


def table_jobs(hal, alloc):
    """{part: [jobs]}, the inner column"""
    words = device_random(hal, alloc, 7, ROWS + 5 - 7)  # 2^25 bits
    parts = {
        "bits": [{"kind": "projected_bits", "level": 0, "n_vars": ROWS, "inner": words, "start_index": 0, "query_size": 5, "query_bits": j, "out": alloc.alloc(elems(0, ROWS))}
                 for j in range(32)],
        "fills": [{"kind": "step_down", "level": 0, "n_vars": ROWS, "index": 1000003, "out": alloc.alloc(elems(0, ROWS))},
                  {"kind": "incrementing", "level": 5, "n_vars": ROWS, "out": alloc.alloc(elems(5, ROWS))},
                  {"kind": "constant", "level": 5, "n_vars": ROWS, "value": 0x9E3779B9, "out": alloc.alloc(elems(5, ROWS))}],
        "powers": [{"kind": "powers", "level": 6, "n_vars": ROWS, "value": B64_GENERATOR, "out": alloc.alloc(elems(6, ROWS))}],
    }
    return parts, words


def moved(jobs):
    """(elements read, elements written), counted from the shapes: an inner column once per job that reads it"""
    read = sum(elems(jb["level"], jb["n_vars"] + jb["query_size"]) for jb in jobs if jb["kind"] == "projected_bits")
    return read, sum(elems(jb["level"], jb["n_vars"]) for jb in jobs)


def host_fill(np, words_host):
    """The columns of the table but the powers, filled as a caller without the op would: numpy on the host, packed as the device wants them."""
    out = []
    w = words_host.view(np.uint32)
    for j in range(32):
        out.append(np.packbits(((w >> np.uint32(j)) & np.uint32(1)).astype(np.uint8), bitorder="little"))
    out.append(np.packbits((np.arange(1 << ROWS) < 1000003).astype(np.uint8), bitorder="little"))
    out.append(np.arange(1 << ROWS, dtype=np.uint32))
    out.append(np.full(1 << ROWS, 0x9E3779B9, dtype=np.uint32))
    return out


def measure(hal, name, jobs, src, dst, runs):
    read, written = moved(jobs)
    tab = hal.generate_job_table(jobs)  # marshalled once: the timed call is the C entry point, not the Python that fills its structs
    c0 = hal.generate_counters()
    gen = timed(hal, lambda: hal.generate_columns_raw(*tab), runs)
    c1 = hal.generate_counters()
    copy_out = timed(hal, lambda: hal.copy_d2d(src.slice(0, max(1, written // 2)), dst.slice(0, max(1, written // 2))), runs)  # a copy of n elements moves 2 n
    both = (read + written) // 2
    copy_io = timed(hal, lambda: hal.copy_d2d(src.slice(0, both), dst.slice(0, both)), runs)
    gen2 = timed(hal, lambda: hal.generate_columns_raw(*tab), runs)  # again behind the copies: the two windows bracket them
    g, b, c = stats(gen + gen2), stats(copy_out), stats(copy_io)
    return {"set": name, "jobs": len(jobs), "launches_per_call": (c1["launches"] - c0["launches"]) // (c1["calls"] - c0["calls"]), "bytes_read": 16 * read,
            "bytes_written": 16 * written, "generate": g, "generate_first_window": stats(gen), "generate_second_window": stats(gen2), "copy_out_bytes": b,
            "copy_in_plus_out_bytes": c, "generate_over_copy_out": round(g["median_ms"] / b["median_ms"], 3),
            "generate_over_copy_in_plus_out": round(g["median_ms"] / c["median_ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np

    import binius_amd

    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    with binius_amd.Context(0, 40 << 20) as hal:  # elements: the table, the regimes' inner columns, the copy's two buffers, the upload's destination
        alloc = hal.dev_alloc()
        parts, words = table_jobs(hal, alloc)
        all_jobs = parts["bits"] + parts["fills"] + parts["powers"]
        read, written = moved(all_jobs)
        half = (read + written) // 2 + 1
        src, dst = alloc.alloc(half), alloc.alloc(half)
        hal.fill(src, 3)
        rec = measure(hal, "table", all_jobs, src, dst, args.runs)
        # (a): fill on the host, then upload
        words_host = np.ascontiguousarray(hal.copy_d2h(words))
        t = []
        for it in range(3 + max(5, args.runs // 2)):
            t0 = time.perf_counter()
            cols = host_fill(np, words_host)
            if it >= 3:
                t.append((time.perf_counter() - t0) * 1e3)
        host = np.frombuffer(b"".join(c.tobytes() for c in cols) + bytes(16 * elems(6, ROWS)), dtype=np.uint64).reshape(-1, 2)  # (the powers' bytes: zeros)
        assert host.shape[0] == written
        up = alloc.alloc(written)
        h2d = timed(hal, lambda: hal.copy_h2d(host, up), max(5, args.runs // 2), warmup=1)
        rec["host_fill_without_powers"], rec["upload_all_bytes"] = stats(t), stats(h2d)
        rec["host_fill_plus_upload_over_generate"] = round((rec["host_fill_without_powers"]["median_ms"] + rec["upload_all_bytes"]["median_ms"]) / rec["generate"]["median_ms"], 1)
        emit(rec)
        for name in ("bits", "fills", "powers"):
            emit(measure(hal, name, parts[name], src, dst, args.runs))
        # one projection per regime: 2^21 bits out of a 2^26-bit inner column (query_size 5), B1
        inner = device_random(hal, alloc, 9, 26 - 7)
        out = alloc.alloc(elems(0, 21))
        for name, start in (("regime_elements(w=9,W=14)", 9), ("regime_one_run_per_input_element(w=3,W=8)", 3), ("regime_runs_inside_an_element(w=0,W=5)", 0)):
            jobs = [{"kind": "projected_bits", "level": 0, "n_vars": 21, "inner": inner, "start_index": start, "query_size": 5, "query_bits": 21, "out": out}]
            emit(measure(hal, name, jobs, src, dst, args.runs))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
