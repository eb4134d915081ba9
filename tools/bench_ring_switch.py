"""The ring switch end to end, two legs on one device over identical inputs.  One JSON line per shape on stdout.

  batched     RingSwitchPlan (bnh_ring_switch_prove): the partial evaluations of every committed column at its claim's suffix, the
              tensor algebra on the host, and ONE bn_ring_switch_eq_ind_batch for the transparents of all claims
  per_claim   what the parent of this change had for the transparents: per claim fill, fill of the first element, tensor_expand and
              fold_right over the limbs (RingSwitchEqInd, ring_switch/eq_ind.rs:81-147), each claim with buffers of its own as the
              reference allocates them; these kernels are untouched by this change, so this leg is the parent's cost of the phase

The legs alternate run by run in one process on the same resident inputs; a run is timed by the host clock and begins and ends with the
device idle.  Reported per leg: minimum and median over the repetitions; for the batched leg the phases (partial_evals, tensor_algebra,
eq_inds) and the device-op counters of a run; the factor between the per-claim leg and the batched eq_inds phase; the outputs of both
legs compared bit for bit; unique bytes (every distinct suffix table read once, every transparent written once) per second of the
batched eq_inds phase.  The per-claim leg's traffic is the count of its passes: 16 B written by the fill, about 48 B moved by the
expansion, 32 B by the fold, per element.

    python tools/bench_ring_switch.py [--reps 9] [--warmup 2] [--shapes keccak:16,u32_add:20]

keccak:L is the claim graph of the keccak circuit at 2^L permutations: 100 one-bit columns of 2^(L + 9) values, 175 claims at three
points, transparents of 2^(L + 2) elements; u32_add:L is 2^L rows: four one-bit columns of 2^(L + 5) values, five claims at two points."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import binius_amd  # noqa: E402
from binius_amd import synthetic  # noqa: E402
from binius_amd._host import RingSwitchPlan  # noqa: E402


def claim_graph(table, log_size):
    """(n_columns, n_vars, [(column, point id)]): every point is a prefix of 7 and a suffix of n_vars - 7 coordinates."""
    if table == "keccak":
        return 100, log_size + 9, sorted([(c, c % 3) for c in range(100)] + [(c, (c + 1) % 3) for c in range(75)])
    if table == "u32_add":
        return 4, log_size + 5, [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0)]
    raise ValueError(table)


def stats(xs):
    return {"min_ms": round(min(xs) * 1e3, 4), "median_ms": round(float(np.median(xs)) * 1e3, 4)}


def eq_expand_host(r):
    """The tensor expansion of a few coordinates on the host (bn_scalar_mul): the mixing and row-batch coefficients of the per-claim leg."""
    out = [1]
    for x in r:
        hi = [binius_amd.HostField.mul(e, x) for e in out]
        out = [e ^ h for e, h in zip(out, hi)] + hi
    return out


def bench(hal, table, log_size, reps, warmup):
    n_columns, n_vars, claim_points = claim_graph(table, log_size)
    kappa, ln = 7, n_vars - 7
    n_points = 1 + max(p for _c, p in claim_points)
    pool = [x for p in range(n_points) for x in synthetic.random_scalars(0x5200 + p, n_vars)]
    suffixes = [(p * n_vars + kappa, ln, kappa) for p in range(n_points)]
    claims = [(c, p, p) for c, p in claim_points]
    n_claims = len(claims)
    mixing = synthetic.random_scalars(0x5210, max(0, (n_claims - 1).bit_length()))
    row = synthetic.random_scalars(0x5211, kappa)
    alloc = hal.dev_alloc()
    cols = []
    for c in range(n_columns):
        s = alloc.alloc(1 << ln)
        if c < 8:
            hal.copy_h2d(synthetic.random_b128(0x5220 + c, 1 << ln), s)
        else:
            hal.copy_d2d(cols[c % 8][0], s)
        cols.append((s, 0, n_vars))
    scratch = alloc.alloc(RingSwitchPlan.scratch_elems(suffixes, claims))
    plan = RingSwitchPlan(hal, cols, pool, suffixes, [kappa] * n_points, claims, scratch, mixing, row)
    # the per-claim leg: coefficients on the device, buffers per claim
    mixing_coeffs, row_coeffs = eq_expand_host(mixing), eq_expand_host(row)
    d_row = alloc.alloc(len(row_coeffs))
    hal.copy_h2d(np.array([[c & ((1 << 64) - 1), c >> 64] for c in row_coeffs], dtype=np.uint64), d_row)
    evals = [alloc.alloc(1 << ln) for _ in range(n_claims)]
    outs = [alloc.alloc(1 << ln) for _ in range(n_claims)]

    def leg_per_claim():
        for i, (_c, p, _p) in enumerate(claims):
            off = suffixes[p][0]
            hal.fill(evals[i], 0)
            hal.fill(evals[i].slice(0, 1), mixing_coeffs[i])
            hal.tensor_expand(0, pool[off : off + ln], evals[i])
            hal.fold_right(evals[i], 7 - kappa, d_row, outs[i])

    t_a, t_b, phases, counters = [], [], [], None
    for r in range(warmup + reps):
        hal.sync()
        rs0, pe0 = hal.ring_switch_counters(), hal.partial_eval_counters()
        t0 = time.perf_counter()
        plan.run()
        hal.sync()
        dt_a = time.perf_counter() - t0
        rs1, pe1 = hal.ring_switch_counters(), hal.partial_eval_counters()
        t0 = time.perf_counter()
        leg_per_claim()
        hal.sync()
        dt_b = time.perf_counter() - t0
        if r >= warmup:
            t_a.append(dt_a)
            t_b.append(dt_b)
            phases.append(plan.phase_times_ms())
            counters = {"ring_switch": {k: rs1[k] - rs0[k] for k in rs1}, "partial_eval_calls": pe1["calls"] - pe0["calls"],
                        "partial_eval_launches": pe1["launches"] - pe0["launches"]}
    ts = plan.transparents()
    pick = sorted({0, 1, n_claims // 2, n_claims - 1})
    same = all(np.array_equal(hal.copy_d2h(ts[i]), hal.copy_d2h(outs[i])) for i in pick)
    ph = {name: {"min_ms": round(min(p[name] for p in phases), 4), "median_ms": round(float(np.median([p[name] for p in phases])), 4)} for name in RingSwitchPlan.PHASES}
    elem_bytes = 16 << ln
    unique = (n_points + n_claims) * elem_bytes
    b = stats(t_b)
    return {
        "what": "ring switch: RingSwitchPlan vs the per-claim RingSwitchEqInd sequence", "table": table, "log_size": log_size,
        "shape": {"columns": n_columns, "n_vars": n_vars, "claims": n_claims, "suffixes": n_points, "kappa": kappa, "transparent_elems": 1 << ln,
                  "transparent_bytes_total": n_claims * elem_bytes},
        "reps": reps, "warmup": warmup,
        "batched": {"wall": stats(t_a), "phases": ph, "device_ops_per_run": counters,
                    "eq_inds_unique_bytes": unique, "eq_inds_unique_bytes_per_s": round(unique / (ph["eq_inds"]["median_ms"] * 1e-3), 1)},
        "per_claim": {"wall": b, "device_op_calls_per_run": 4 * n_claims, "pass_bytes": 6 * n_claims * elem_bytes,
                      "pass_bytes_per_s": round(6 * n_claims * elem_bytes / (b["median_ms"] * 1e-3), 1)},
        "eq_inds_factor_median": round(b["median_ms"] / ph["eq_inds"]["median_ms"], 2),
        "eq_inds_factor_min": round(b["min_ms"] / ph["eq_inds"]["min_ms"], 2),
        "same_outputs": bool(same),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="keccak:16,u32_add:20")
    args = ap.parse_args()
    for spec in [s for s in args.shapes.split(",") if s]:
        table, log_size = spec.split(":")
        n_columns, n_vars, claim_points = claim_graph(table, int(log_size))
        elems = (n_columns + 3 * len(claim_points) + 4) << (n_vars - 7)
        with binius_amd.Context(0, elems + (1 << 20)) as hal:
            print(json.dumps(bench(hal, table, int(log_size), args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
