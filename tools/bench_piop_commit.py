#!/usr/bin/env python
"""piop::commit with the merge on the device (bn_merge_multilins, bnh_piop_commit) against the route that existed before it, on one
MI355X.  Two shapes: tools/bench_piop.py's committed sizes [17, 17, 19, 20] and tools/bench_keccak_replay.py's committed set at its
default size (100 multilinears of 2^18).  One JSON line per shape and measurement:

  merge          bn_merge_multilins alone (log_repeats = 0) at tile t, beside a bn_copy_d2d that moves the same number of bytes
                 -- 16 * (sum 2^n_vars + 2^total_vars) -- timed in the same run: the copy is the yardstick.  With --tile-sweep both
                 t = 5 and t = 6 are timed; that needs a measurement build (`make BN_KNOBS=1`), which reads BN_MERGE_T; the tool
                 checks through the counters that the library honours it and says so in the record.
  commit         the commit phase, new route (bnh_piop_commit: merge into the codeword with every repeat, NTT, Merkle) against the
                 old one (host merge_multilins, chunked copy_h2d, commit_interleaved: head copy, repeat copies, NTT, Merkle), the old
                 one once from a message already resident and once with the host merge and the upload counted.

Every figure: warm-up runs, then the median of --runs timed runs (wall clock between two synchronisations), with min, max and the
interquartile range.

  python tools/bench_piop_commit.py [--runs 25] [--tile-sweep] [--out profiles/r19/piop_commit.jsonl]"""
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


def tile_knob_honoured(hal, alloc):
    """A multilinear of 2^10 is a tiled job at t = 5 and a small one at t = 6: the counters tell whether BN_MERGE_T is read."""
    src, msg = alloc.alloc(1 << 10), alloc.alloc(1 << 10)
    hal.fill(src, 1)
    got = {}
    for t in (5, 6):
        os.environ["BN_MERGE_T"] = str(t)
        c0 = hal.merge_counters()
        hal.merge_multilins([src], msg, 10)
        got[t] = hal.merge_counters()["jobs_tiled"] - c0["jobs_tiled"]
    os.environ.pop("BN_MERGE_T", None)
    return got == {5: 1, 6: 0}


def host_merge_and_upload(hal, np, host_mls, total_vars, d_msg):
    """the old route's host part, as tools/bench_keccak_replay.py does it: numpy scatter per multilinear, chunked copy_h2d"""
    msg = np.zeros((1 << total_vars, 2), dtype=np.uint64)
    at = 0
    for x in reversed(host_mls):
        n = x.shape[0]
        v = n.bit_length() - 1
        idx = np.arange(n, dtype=np.int64)
        rev = np.zeros_like(idx)
        for b in range(v):
            rev |= ((idx >> b) & 1) << (v - 1 - b)
        chunk = np.empty_like(x)
        chunk[rev] = x
        msg[at : at + n] = chunk
        at += n
    step = 1 << 22
    for off in range(0, 1 << total_vars, step):
        hal.copy_h2d(msg[off : off + step], d_msg.slice(off, min(1 << total_vars, off + step)))
    hal.sync()


def bench_shape(name, n_varss, args, emit):
    import numpy as np

    import binius_amd
    from binius_amd import synthetic
    from binius_amd._host import FRIParams, FriPlan, PiopCommit, piop_commit_elems, piop_message_layout

    _, total_vars = piop_message_layout(n_varss)
    arities = []
    while sum(arities) + args.arity < total_vars:
        arities.append(args.arity)
    p = FRIParams(total_vars - args.log_batch, args.log_inv_rate, args.log_batch, arities, n_test_queries=3)
    code_elems, tree_elems = piop_commit_elems(p)
    data_elems = sum(1 << v for v in n_varss)
    merge_bytes = 16 * (data_elems + (1 << total_vars))
    base = {"shape": name, "n_multilins": len(n_varss), "max_n_vars": max(n_varss), "total_vars": total_vars, "data_elems": data_elems,
            "fri": {"log_inv_rate": args.log_inv_rate, "log_batch": args.log_batch, "arities": arities}}
    arena = data_elems + (1 << total_vars) + 2 * code_elems + tree_elems + merge_bytes // 16 + (1 << 16)
    with binius_amd.Context(0, arena) as hal:
        alloc = hal.dev_alloc()
        knob = tile_knob_honoured(hal, alloc) if args.tile_sweep else False
        srcs = [device_random(hal, alloc, 0x6E00 + i, v) for i, v in enumerate(n_varss)]
        d_msg = alloc.alloc(1 << total_vars)
        work = alloc.alloc(2 * code_elems + tree_elems)
        copy_src, copy_dst = alloc.alloc(merge_bytes // 32), alloc.alloc(merge_bytes // 32)
        hal.fill(copy_src, 3)

        # ---- 1. the merge alone, beside a copy of the same bytes
        copy = stats(timed(hal, lambda: hal.copy_d2d(copy_src, copy_dst), args.runs))
        for t in ((5, 6) if knob else (binius_amd._ffi.BN_MERGE_TILE_LOG2,)):
            if knob:
                os.environ["BN_MERGE_T"] = str(t)
            c0 = hal.merge_counters()
            m = stats(timed(hal, lambda: hal.merge_multilins(srcs, d_msg, total_vars), args.runs))
            c1 = hal.merge_counters()
            rep = stats(timed(hal, lambda: hal.merge_multilins(srcs, work.slice(0, code_elems), total_vars, args.log_inv_rate), args.runs))
            emit(dict(base, measure="merge", tile_log2=t, tile_knob_honoured=knob, bytes=merge_bytes, merge=m, copy_same_bytes=copy,
                      ratio_to_copy=round(m["median_ms"] / copy["median_ms"], 3), gb_per_s=round(merge_bytes / m["median_ms"] / 1e6, 1),
                      copy_gb_per_s=round(merge_bytes / copy["median_ms"] / 1e6, 1),
                      launches_per_call=(c1["launches"] - c0["launches"]) / max(1, c1["calls"] - c0["calls"]),
                      merge_into_codeword=dict(rep, bytes=16 * (data_elems + code_elems))))
        os.environ.pop("BN_MERGE_T", None)

        # ---- 2. the commit phase: new route, old route from a resident message, old route with the host merge and upload
        commit = PiopCommit(hal, list(zip(n_varss, srcs)), p, work.slice(0, code_elems), work.slice(code_elems, code_elems + tree_elems))
        new_phases = []
        timed(hal, lambda: new_phases.append(commit.run()), args.runs, warmup=0)
        # (the figure to hold against the old route's: one call between two synchronisations, none inside -- taking the phases costs three)
        new_ms = []
        for it in range(3 + args.runs):
            commit.run(phases=False)
            if it >= 3:
                new_ms.append(commit.total_ms)  # (bracketed by synchronisations inside the call, as the old route's figure below)
        new = stats(new_ms)
        new_commitment = commit.commitment
        hal.merge_multilins(srcs, d_msg, total_vars)  # (the message of the old route: the same bytes the host merge makes)
        fri = FriPlan(hal, p, d_msg, work, synthetic.random_scalars(0x7A0 + total_vars, total_vars))
        old_ms = []
        for it in range(3 + args.runs):
            ms = fri.run()[0]  # (phase 0: commit_interleaved alone, bracketed by synchronisations inside the call)
            if it >= 3:
                old_ms.append(ms)
        old = stats(old_ms)
        same_commitment = bytes(fri.roots[0]) == new_commitment
        host_mls = [hal.copy_d2h(s) for s in srcs]
        host = stats(timed(hal, lambda: host_merge_and_upload(hal, np, host_mls, total_vars, d_msg), args.host_runs, warmup=1))
        emit(dict(base, measure="commit", tile_log2=binius_amd._ffi.BN_MERGE_TILE_LOG2, new_route=new,
                  new_route_phases_median_ms=[round(statistics.median(x[i] for x in new_phases), 4) for i in range(3)],
                  old_route_resident_message=old, old_route_host_merge_and_upload=host,
                  old_route_total_median_ms=round(old["median_ms"] + host["median_ms"], 3),
                  new_minus_old_resident_ms=round(new["median_ms"] - old["median_ms"], 4), commitments_equal=same_commitment))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--log-inv-rate", type=int, default=1)
    ap.add_argument("--log-batch", type=int, default=4)
    ap.add_argument("--arity", type=int, default=4)
    ap.add_argument("--tile-sweep", action="store_true", help="time t = 5 and t = 6 (a BN_KNOBS=1 build)")
    ap.add_argument("--shapes", default="piop,keccak")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = {"piop": [17, 17, 19, 20], "keccak": [18] * 100}
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in args.shapes.split(","):
        bench_shape(name, shapes[name], args, emit)


if __name__ == "__main__":
    main()
