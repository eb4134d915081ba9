"""The univariate-skip zerocheck end to end, two measurements on one device.  JSON lines on stdout.

(a) The fold of the univariate round: ONE bn_univariate_fold_batch over all columns against what the parent of this change did with the
same inputs -- one bn_fold_right per column, whose code this change does not touch.  Both arms run in the same process on the same
resident inputs, alternating run by run; a run is timed by the host clock and ends with the device idle.  Reported: median, 10th and
90th percentile of both, the factor between the medians, the outputs compared bit for bit, the launches of a batch call
(bn_univariate_fold_counters), and the algorithmic bytes -- the column bytes read plus 16 bytes per output written -- per second of the
batch call against 8 TB/s.

(b) bnh_zerocheck_batch_prove at the keccak shapes: per phase (univariate round, fold, multilinear rounds, projection, reduction) the
wall time and the device-op calls the phase made itself, median over the repetitions; the witness is random (the prover's work does not
depend on the constraints holding).

(c) --table b32_mul: the table of examples/b32_mul.rs -- three columns of 2^--table-log-rows values at tower level --table-level (5: B32;
7: the same table over B128) and the constraint a b - c, k = 7.  --arm new: bnh_zerocheck_batch_prove_tower end to end with its phases
and the univariate round's share.  --arm parent: the only route a build without that entry point offers for the table -- widening the
columns to B128 (bn_partial_eval_high_batch at query_vars = 0) and bnh_eqind_sumcheck_prove over all the rounds; it uses nothing this
change adds, so the same file runs against a build of the parent commit.  --arm keccak: keccak's B1 table through the old entry point
and through the new one (base 3, forwarded), alternating.  Medians of --reps runs after --warmup.

    python tools/bench_zerocheck_skip.py [--reps 20] [--warmup 3] [--fold-shapes 204:21:0:7,204:23:0:7,204:25:0:7,16:24:3:7,16:24:3:4]
                                         [--prove-log-perms 12 14 16] [--prove-reps 3]
    python tools/bench_zerocheck_skip.py --table b32_mul --arm new|parent|keccak [--table-level 5] [--table-log-rows 20]

A fold shape is n_cols:n_vars:tower_level:k; keccak's table has 204 one-bit columns of 2^(log_perms + 9) values."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import binius_amd  # noqa: E402
from binius_amd import synthetic  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
DEFAULT_FOLD_SHAPES = "204:21:0:7,204:23:0:7,204:25:0:7,16:24:3:7,16:24:3:4"


def pct(xs):
    a = np.sort(np.asarray(xs))
    return {"median_us": round(float(np.median(a)) * 1e6, 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]) * 1e6, 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]) * 1e6, 2)}


def random_columns(hal, alloc, n_cols, elems, seed):
    """n_cols resident columns of `elems` elements: eight distinct random arrays uploaded, the others device copies of them."""
    cols = []
    for t in range(n_cols):
        c = alloc.alloc(elems)
        if t < 8:
            hal.copy_h2d(synthetic.random_b128(seed + t, elems), c)
        else:
            hal.copy_d2d(cols[t % 8], c)
        cols.append(c)
    return cols


def bench_fold(hal, n_cols, n_vars, level, k, reps, warmup):
    alloc = hal.dev_alloc()
    elems = max(1, 1 << (n_vars + level - 7))
    out_len = 1 << (n_vars - k)
    coeffs = synthetic.random_scalars(0xF01D + k, 1 << k)
    d_coeffs = alloc.alloc(1 << k)
    hal.copy_h2d(np.array([[c & ((1 << 64) - 1), c >> 64] for c in coeffs], dtype=np.uint64), d_coeffs)
    cols = [(c, level, n_vars) for c in random_columns(hal, alloc, n_cols, elems, 0xF0100)]
    outs_a = [alloc.alloc(out_len) for _ in range(n_cols)]
    outs_b = [alloc.alloc(out_len) for _ in range(n_cols)]

    def arm_batch():
        hal.univariate_fold_batch(cols, k, coeffs, outs_a)
        hal.sync()

    def arm_per_column():
        for (c, _, _), o in zip(cols, outs_b):
            hal.fold_right(c, level, d_coeffs, o)
        hal.sync()

    ta, tb = [], []
    before = hal.univariate_fold_counters()
    for r in range(warmup + reps):
        for arm, ts in ((arm_batch, ta), (arm_per_column, tb)):
            t0 = time.perf_counter()
            arm()
            dt = time.perf_counter() - t0
            if r >= warmup:
                ts.append(dt)
    now = hal.univariate_fold_counters()
    same = all(np.array_equal(hal.copy_d2h(x), hal.copy_d2h(y)) for x, y in zip(outs_a[:8] + outs_a[-2:], outs_b[:8] + outs_b[-2:]))
    a, p = pct(ta), pct(tb)
    algo_bytes = n_cols * (elems * 16 + out_len * 16)
    return {
        "what": "univariate_fold_batch vs fold_right per column",
        "shape": {"n_cols": n_cols, "n_vars": n_vars, "tower_level": level, "k": k, "column_bytes": n_cols * elems * 16, "output_bytes": n_cols * out_len * 16},
        "batch": a, "per_column_fold_right": p, "reps": reps,
        "factor_median": round(p["median_us"] / a["median_us"], 2), "not_slower": a["median_us"] <= p["median_us"], "same_outputs": bool(same),
        "launches_per_batch_call": (now["launches"] - before["launches"]) / (warmup + reps),
        "algorithmic_bytes": algo_bytes, "algorithmic_bytes_per_s": round(algo_bytes / (a["median_us"] * 1e-6), 1),
        "share_of_8TBps": round(algo_bytes / (a["median_us"] * 1e-6) / HBM_BYTES_PER_S, 4),
    }


def keccak_constraints(n_batches=3):
    """The keccak table's constraint set (m3/src/gadgets/hash/keccak/stacked.rs:142-151, 340-363) as (steps, leading form, degree) over
    per batch 25 state_out, 25 b, 1 round constant; then 25 packed state_out, 25 next_state_in, 1 selector."""
    comps, n = [], 0
    for _ in range(n_batches):
        out0, b0, rc = n, n + 25, n + 50
        n += 51
        for x in range(5):
            for y in range(5):
                o, bb0, bb1, bb2 = out0 + 5 * y + x, b0 + 5 * y + x, b0 + 5 * y + (x + 1) % 5, b0 + 5 * y + (x + 2) % 5
                steps = [("var", bb1), ("const", 1), ("add", 0, 1), ("var", bb2), ("mul", 2, 3), ("var", bb0), ("add", 4, 5), ("var", o), ("add", 6, 7)]
                if (x, y) == (0, 0):
                    steps += [("var", rc), ("add", 8, 9)]
                comps.append((steps, [("var", bb1), ("var", bb2), ("mul", 0, 1)], 2))
    sop, nsi, sel = n, n + 25, n + 50
    n += 51
    for i in range(25):
        prod = [("var", sop + i), ("var", nsi + i), ("add", 0, 1), ("var", sel), ("mul", 2, 3)]
        comps.append((prod, prod, 2))
    return n, comps


MUL = ([("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("add", 2, 3)], [("var", 0), ("var", 1), ("mul", 0, 1)], 2)  # a b - c


def mul_table_columns(hal, alloc, level, n_vars):
    return random_columns(hal, alloc, 3, max(1, 1 << (n_vars + level - 7)), 0xF0400 + level)


def bench_mul_table_new(hal, level, n_vars, reps, warmup):
    from binius_amd._host import ZerocheckBatchPlan

    k = 7
    alloc = hal.dev_alloc()
    tables = [(n_vars, [(c, level) for c in mul_table_columns(hal, alloc, level, n_vars)], [MUL])]
    scratch = alloc.alloc(ZerocheckBatchPlan.scratch_elems(tables, k, tower=True))
    rounds = n_vars - k
    s = synthetic.random_scalars(0xF0500 + level, 2 * rounds + 3 + k)
    args = (s[:rounds], s[rounds:rounds + 1], s[rounds + 1], s[rounds + 2:2 * rounds + 2], s[2 * rounds + 2], s[2 * rounds + 3:])
    walls, phases = [], []
    for r in range(warmup + reps):
        plan = ZerocheckBatchPlan(hal, tables, k, *args, scratch, tower=True)
        t0 = time.perf_counter()
        plan.run()
        hal.sync()
        if r >= warmup:
            walls.append(time.perf_counter() - t0)
            phases.append(plan.phases())
    rec = {"what": "zerocheck_batch_prove_tower, a b - c", "arm": "new", "tower_level": level, "n_vars": n_vars, "k": k, "reps": reps, **pct(walls), "phases": {}}
    for name in ZerocheckBatchPlan.PHASES:
        rec["phases"][name] = {"ms": round(float(np.median([p[name][0] for p in phases])), 3), "device_op_calls": phases[-1][name][1]}
    rec["univariate_share"] = round(rec["phases"]["univariate"]["ms"] * 1e3 / rec["median_us"], 3)
    return rec


def bench_mul_table_parent(hal, level, n_vars, reps, warmup):
    from binius_amd._host import EqIndPlan

    alloc = hal.dev_alloc()
    cols = mul_table_columns(hal, alloc, level, n_vars)
    one = alloc.alloc(1)
    hal.copy_h2d(np.array([[1, 0]], dtype=np.uint64), one)
    widened = [alloc.alloc(1 << n_vars) for _ in cols]
    eq_scratch = alloc.alloc(1 << (n_vars - 1))
    s = synthetic.random_scalars(0xF0600 + level, 2 * n_vars + 1)
    walls, widen = [], []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        hal.partial_eval_high_batch([(c, level, n_vars) for c in cols], one, 0, widened)  # (the prover folds its inputs in place: widened anew per proof)
        hal.sync()
        t1 = time.perf_counter()
        EqIndPlan(hal, n_vars, widened, [MUL[:2]], [0], s[:n_vars], eq_scratch, s[n_vars], s[n_vars + 1:], degrees=[2]).run()
        hal.sync()
        if r >= warmup:
            walls.append(time.perf_counter() - t0)
            widen.append(t1 - t0)
    return {"what": "widen to B128 + eqind_sumcheck_prove over all rounds, a b - c", "arm": "parent", "tower_level": level, "n_vars": n_vars, "reps": reps, **pct(walls),
            "widen_median_us": round(float(np.median(widen)) * 1e6, 2)}


def bench_keccak_forwarding(hal, log_perms, reps, warmup):
    from binius_amd._host import ZerocheckBatchPlan

    k, n_vars = 7, log_perms + 9
    n_cols, comps = keccak_constraints(3)
    alloc = hal.dev_alloc()
    tables = [(n_vars, [(c, 0) for c in random_columns(hal, alloc, n_cols, 1 << (n_vars - 7), 0xF0200)], comps)]
    scratch = alloc.alloc(max(ZerocheckBatchPlan.scratch_elems(tables, k), ZerocheckBatchPlan.scratch_elems(tables, k, tower=True)))
    rounds = n_vars - k
    s = synthetic.random_scalars(0xF0300 + log_perms, 2 * rounds + 3 + k)
    args = (s[:rounds], s[rounds:rounds + 1], s[rounds + 1], s[rounds + 2:2 * rounds + 2], s[2 * rounds + 2], s[2 * rounds + 3:])
    walls, outs = {False: [], True: []}, {}
    for r in range(warmup + reps):
        for tower in (False, True):  # alternating, run by run
            plan = ZerocheckBatchPlan(hal, tables, k, *args, scratch, tower=tower)
            t0 = time.perf_counter()
            outs[tower] = plan.run()
            hal.sync()
            if r >= warmup:
                walls[tower].append(time.perf_counter() - t0)
    return {"what": "keccak's B1 table: old entry point vs the new one (base 3, forwarded)", "arm": "keccak", "log_perms": log_perms, "n_vars": n_vars, "reps": reps,
            "old_entry": pct(walls[False]), "new_entry": pct(walls[True]), "same_outputs": outs[False] == outs[True]}


def bench_prove(hal, log_perms, reps):
    from binius_amd._host import ZerocheckBatchPlan

    k, n_vars = 7, log_perms + 9
    n_cols, comps = keccak_constraints(3)
    alloc = hal.dev_alloc()
    cols = [(c, 0) for c in random_columns(hal, alloc, n_cols, 1 << (n_vars - 7), 0xF0200)]
    tables = [(n_vars, cols, comps)]
    scratch = alloc.alloc(ZerocheckBatchPlan.scratch_elems(tables, k))
    rounds = n_vars - k
    s = synthetic.random_scalars(0xF0300 + log_perms, 2 * rounds + 3 + k)
    args = (s[:rounds], s[rounds:rounds + 1], s[rounds + 1], s[rounds + 2:2 * rounds + 2], s[2 * rounds + 2], s[2 * rounds + 3:])
    walls, phases = [], []
    for r in range(reps + 1):  # (the first run warms up: module load, scratch growth)
        plan = ZerocheckBatchPlan(hal, tables, k, *args, scratch)
        t0 = time.perf_counter()
        plan.run()
        hal.sync()
        if r:
            walls.append(time.perf_counter() - t0)
            phases.append(plan.phases())
    rec = {"what": "zerocheck_batch_prove, keccak", "log_perms": log_perms, "n_vars": n_vars, "k": k, "columns": n_cols, "constraints": len(comps), "reps": reps,
           "wall_ms": round(float(np.median(walls)) * 1e3, 3), "phases": {}}
    for name in ZerocheckBatchPlan.PHASES:
        rec["phases"][name] = {"ms": round(float(np.median([p[name][0] for p in phases])), 3), "device_op_calls": phases[-1][name][1]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fold-shapes", default=DEFAULT_FOLD_SHAPES)
    ap.add_argument("--prove-log-perms", type=int, nargs="*", default=[12, 14, 16])
    ap.add_argument("--prove-reps", type=int, default=3)
    ap.add_argument("--table", choices=["b32_mul"], default=None)
    ap.add_argument("--arm", choices=["new", "parent", "keccak"], default="new")
    ap.add_argument("--table-level", type=int, default=5)
    ap.add_argument("--table-log-rows", type=int, default=20)
    args = ap.parse_args()
    if args.table:
        with binius_amd.Context(0, 15 << 24) as hal:
            if args.arm == "new":
                rec = bench_mul_table_new(hal, args.table_level, args.table_log_rows, args.reps, args.warmup)
            elif args.arm == "parent":
                rec = bench_mul_table_parent(hal, args.table_level, args.table_log_rows, args.reps, args.warmup)
            else:
                rec = bench_keccak_forwarding(hal, args.table_log_rows - 9, args.reps, args.warmup)
            print(json.dumps(rec), flush=True)
        return
    with binius_amd.Context(0, 15 << 24) as hal:
        for spec in [s for s in args.fold_shapes.split(",") if s]:
            n_cols, n_vars, level, k = (int(x) for x in spec.split(":"))
            print(json.dumps(bench_fold(hal, n_cols, n_vars, level, k, args.reps, args.warmup)), flush=True)
        for lp in args.prove_log_perms:
            print(json.dumps(bench_prove(hal, lp, args.prove_reps)), flush=True)


if __name__ == "__main__":
    main()
