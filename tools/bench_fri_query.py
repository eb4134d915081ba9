#!/usr/bin/env python
"""The FRI query phase on one MI355X: FRIFolder::finish_proof through bn_fri_query_openings (every opening of a proof from one
launch) against the route that existed before it -- finalize's copy of the terminate codeword and one FRIQueryProver::prove_query per
index, a copy_d2h and a bn_gather_d2h per opening.  Both on the same resident codewords and trees, in the same process, alternating
(bnh_fri_query_phase_bench: the loop runs in the compiled mirror, so neither route pays for Python).  Two shapes: tools/bench_piop.py's
committed sizes [17, 17, 19, 20] and keccak's committed set (100 multilinears of 2^18); FRI parameters as
make_commit_params_with_optimal_arity chooses them (piop/verify.rs:146-168, fri/common.rs:68-123, 199-250) at --security-bits.

One JSON line per shape: warm-up runs, then the median of --runs timed runs (host clock between two synchronisations) with min and max
for each route, the old route's spread (max - min), and whether the new route is faster by more than that spread.  Not measured here:
the kernel's own time and the share of the PCIe transfer.

  python tools/bench_fri_query.py [--runs 25] [--warmup 3] [--security-bits 96] [--out profiles/r20/fri_query.jsonl]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_keccak_replay import device_random  # noqa: E402


def estimate_optimal_arity(log_block_length, digest_size=32, field_size=16):
    """fri/common.rs:224-250"""
    best, old = None, None
    for arity in range(1, log_block_length + 1):
        cost = ((log_block_length // 2) * digest_size + (1 << arity) * field_size) * (log_block_length - arity) // arity
        if old is not None and cost > old:
            break
        best, old = arity, cost
    return best if best is not None else 1


def optimal_params(total_vars, log_inv_rate, security_bits):
    """make_commit_params_with_optimal_arity -> FRIParams::choose_with_constant_fold_arity with calculate_n_test_queries, F = B128"""
    from binius_amd._host import FRIParams

    arity = estimate_optimal_arity(total_vars + log_inv_rate)
    log_dim, log_batch = max(0, total_vars - arity), min(total_vars, arity)
    field_size = 2.0 ** 128
    per_query_err = 0.5 * (1.0 + 2.0 ** (-log_inv_rate))
    allowed = 2.0 ** (-security_bits) - (2 * log_dim) / field_size - (2.0 ** (log_dim + log_inv_rate)) / field_size
    n_queries = int(math.ceil(math.log(allowed) / math.log(per_query_err)))
    cap_height = max(0, (n_queries - 1).bit_length())
    n_arities = max(0, total_vars - max(0, cap_height - log_inv_rate)) // arity
    return FRIParams(log_dim, log_inv_rate, log_batch, [arity] * n_arities, n_queries)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "runs": len(ms)}


def bench_shape(name, n_varss, args, emit):
    import binius_amd
    from binius_amd import synthetic
    from binius_amd._host import fri_query_phase_bench, piop_message_layout

    _, total_vars = piop_message_layout(n_varss)
    p = optimal_params(total_vars, args.log_inv_rate, args.security_bits)
    code_elems = 1 << (total_vars + args.log_inv_rate)
    with binius_amd.Context(0, (1 << total_vars) + 2 * code_elems + (1 << 16)) as hal:
        alloc = hal.dev_alloc()
        message = device_random(hal, alloc, 0x0F21, total_vars)
        scratch = alloc.alloc(2 * code_elems)
        challenges = synthetic.random_scalars(0x7A0 + total_vars, total_vars)
        top = (1 << p.index_bits()) - 1
        words = synthetic.random_b128(0x1D1CE5 + total_vars, p.n_test_queries)
        indices = [int(words[i, 0]) & top for i in range(p.n_test_queries)]
        c0 = hal.fri_query_counters()
        new_ms, old_ms, advice_elems, same = fri_query_phase_bench(hal, p, message, scratch, challenges, indices, args.warmup, args.runs)
        c1 = hal.fri_query_counters()
    new, old = stats(new_ms), stats(old_ms)
    spread = round(old["max_ms"] - old["min_ms"], 4)
    n_calls = c1["calls"] - c0["calls"]
    emit({"shape": name, "n_multilins": len(n_varss), "total_vars": total_vars,
          "fri": {"log_dim": p.log_dim, "log_inv_rate": p.log_inv_rate, "log_batch": p.log_batch_size, "arities": p.fold_arities, "n_test_queries": p.n_test_queries,
                  "security_bits": args.security_bits, "layer_depths": p.optimal_layer_depths()},
          "advice_bytes": 16 * advice_elems, "openings": p.n_test_queries * len(p.fold_arities),
          "new_route_finish_proof": new, "old_route_per_opening": old, "old_route_spread_ms": spread,
          "speedup": round(old["median_ms"] / new["median_ms"], 2) if new["median_ms"] else None,
          "new_faster_by_more_than_old_spread": old["median_ms"] - new["median_ms"] > spread,
          "launches_per_new_call": (c1["launches"] - c0["launches"]) / max(1, n_calls), "same_bytes": same, "warmup": args.warmup})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log-inv-rate", type=int, default=1)
    ap.add_argument("--security-bits", type=int, default=96)
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
