#!/usr/bin/env python
"""bn_compute_composite with a tower-typed expression, and the compute plan, on one MI355X beside the two things each is compared with,
in one process.

The shapes are what a table of 2^20 rows shaped like m3's mul gadget computes beside its committed columns:

  select     (a) a + s (a + b) at B1 over 2^26 bits (64 such bit columns of the table side by side): three inputs, one output, level 0
  pack_fp    (b) sum of bit_i 2^i into B32 from 32 B1 columns of 2^20 bits: 127 steps, 32 inputs
  product    (c) a B32 x B32 product column of 2^20 values
  plan       (d) the plan of the table (WitnessCompute): 65 given B1 columns, 32 composites a_k + s (a_k + b_k), pack_fp of them into
             B32, one shifted column of a composite: 33 bn_compute_composite calls and one bn_derive_columns_batch
  plan_batched (e) plan (d) through WitnessComputeBatched: the expression columns of a wave in one launch (bn_expr_compile_tower_batch),
             3 launches.  (d) and (e) run ALTERNATELY in the same process -- d, e, the copy, d, e -- and (e)'s record carries (d)'s
             figures of that session, the call of the wave-1 batch alone (32 composites of 2^20 bits: compile, batch, call, frees as
             the plan does them, and the call by itself on a resident batch) and a copy of the bytes that wave reads plus writes

and the comparisons, per shape

  compute      the call (expression upload at first use, pointer upload and launch are in it; the plan: compile, calls and frees)
  copy         a bn_copy_d2d of the bytes the call reads plus writes: its floor
  host_fill    what a caller does without the op: the same column(s) computed with numpy on the host, on packed words where numpy can
               (select), on unpacked bits where it cannot (pack_fp) -- the product has no numpy form: its fill is NOT in the figure --
  upload       ... and a bn_copy_h2d of the output bytes: the host path is host_fill + upload

Every figure: 3 warm-up runs, then the median of the timed runs (host clock between two synchronisations), with min, max and the
interquartile range.  One JSON line per record.

  python tools/bench_compute_columns.py [--runs 20] [--out profiles/r28/compute_columns.jsonl] [--only select]
  python tools/bench_compute_columns.py --only plan_batched --out profiles/r29/compute_columns.jsonl     (d) and (e), alternately
  python tools/bench_compute_columns.py --only wave1 --runs 5      the wave-1 batch call alone: for a counter run of its kernel"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_derive import stats, timed  # noqa: E402
from bench_keccak_replay import device_random  # noqa: E402

ROWS = 20  # log2 of the table's rows
SELECT = [("var", 0), ("var", 1), ("var", 2), ("add", 0, 1), ("mul", 2, 3), ("add", 0, 4)]


def pack_steps(n_bits):
    steps, acc = [], None
    for i in range(n_bits):
        steps += [("var", i), ("const", 1 << i), ("mul", len(steps), len(steps) + 1)]
        if acc is not None:
            steps.append(("add", acc, len(steps) - 1))
        acc = len(steps) - 1
    return steps


def elems(level, n_vars):
    return 1 << (n_vars + level - 7)


def host_timed(fn, runs):
    t, out = [], None
    for it in range(2 + runs):
        t0 = time.perf_counter()
        out = fn()
        if it >= 2:
            t.append((time.perf_counter() - t0) * 1e3)
    return t, out


def windows(hal, call, read, written, src, dst, runs):
    """(the call, the copy of the bytes it reads plus writes, the call again: the two windows bracket the copies)"""
    both = (read + written) // 2  # (a copy of n elements moves 2 n)
    first = timed(hal, call, runs)
    copy = timed(hal, lambda: hal.copy_d2d(src.slice(0, both), dst.slice(0, both)), runs)
    return first, copy, timed(hal, call, runs)


def finish(hal, alloc, rec, timings, read, written, fill_ms, out_host, runs):
    compute, copy, compute2 = timings
    up = alloc.alloc(written)
    h2d = timed(hal, lambda: hal.copy_h2d(out_host, up), max(5, runs // 2), warmup=1)
    c, f = stats(compute + compute2), stats(copy)
    rec.update({"bytes_read": 16 * read, "bytes_written": 16 * written, "compute": c, "compute_first_window": stats(compute), "compute_second_window": stats(compute2),
                "copy_read_plus_written_bytes": f, "compute_over_copy": round(c["median_ms"] / f["median_ms"], 3), "upload_output_bytes": stats(h2d)})
    if fill_ms is not None:
        rec["host_fill"] = stats(fill_ms)
        rec["host_fill_plus_upload_over_compute"] = round((rec["host_fill"]["median_ms"] + rec["upload_output_bytes"]["median_ms"]) / c["median_ms"], 1)
    else:
        rec["host_fill"] = None  # (numpy has no product of the field: the host path's figure is the upload alone)
        rec["upload_over_compute"] = round(rec["upload_output_bytes"]["median_ms"] / c["median_ms"], 1)
    return rec


def one_call(hal, alloc, np, name, steps, levels, out_level, n_vars, src, dst, runs, host_fn):
    ins = [device_random(hal, alloc, 31 + 7 * i, n_vars + lv - 7) for i, lv in enumerate(levels)]
    out = alloc.alloc(elems(out_level, n_vars))
    expr = hal.expr_compile_tower(steps, levels, out_level)
    c0 = hal.compute_composite_counters()
    call = lambda: hal.compute_composite_tower(ins, out, expr, 1 << n_vars)  # noqa: E731
    read, written = sum(elems(lv, n_vars) for lv in levels), elems(out_level, n_vars)
    timings = windows(hal, call, read, written, src, dst, runs)
    c1 = hal.compute_composite_counters()
    fill_ms, out_host = None, np.zeros((written, 2), dtype=np.uint64)
    if host_fn is not None:
        host_ins = [np.ascontiguousarray(hal.copy_d2h(d)) for d in ins]
        fill_ms, got = host_timed(lambda: host_fn(np, host_ins), max(3, runs // 4))
        out_host = np.ascontiguousarray(got).view(np.uint64).reshape(-1, 2)
        assert np.array_equal(hal.copy_d2h(out), out_host), "%s: the host path and the device disagree" % name
    rec = {"shape": name, "steps": len(steps), "inputs": len(levels), "out_level": out_level, "values": 1 << n_vars,
           "launches_per_call": (c1["launches"] - c0["launches"]) // (c1["calls"] - c0["calls"])}
    return finish(hal, alloc, rec, timings, read, written, fill_ms, out_host, runs)


def host_select(np, ins):
    a, b, s = (x.reshape(-1) for x in ins)
    return a ^ (s & (a ^ b))


def host_pack(np, ins):
    acc = np.zeros(1 << ROWS, dtype=np.uint32)
    for i, col in enumerate(ins):
        acc |= np.unpackbits(col.view(np.uint8).reshape(-1), bitorder="little").astype(np.uint32) << np.uint32(i)
    return acc


def plan_columns(hal, alloc):
    given = [device_random(hal, alloc, 500 + i, ROWS - 7) for i in range(65)]
    cols = [("given", d, 0, ROWS) for d in given]
    cols += [("computed", SELECT, [k, 32 + k, 64], ROWS, 0) for k in range(32)]
    cols.append(("lincomb", [(65 + k, 1 << k) for k in range(32)], 0, ROWS))
    cols.append(("shifted", 65, 5, 3, "logical_left"))
    return cols, given


def host_plan(np, ins):
    a, b, s = ins[:32], ins[32:64], ins[64].reshape(-1)
    sel = [a[k].reshape(-1) ^ (s & (a[k].reshape(-1) ^ b[k].reshape(-1))) for k in range(32)]
    packed = host_pack(np, sel)
    w = sel[0].view(np.uint32)
    return sel, packed, (w << np.uint32(3))  # (logical left by 3 inside blocks of 2^5 values)


def wave1_batch(hal, given, out):
    """(the batch of plan (d)'s wave 1 on a resident handle, its rows): 32 composites a_k + s (a_k + b_k) of 2^20 bits into `out`"""
    e = hal.expr_compile_tower(SELECT, [0, 0, 0], 0)
    n = elems(0, ROWS)
    batch = hal.expr_compile_tower_batch([e], [(0, 3 * k, ROWS, k * n) for k in range(32)])
    rows = [r for k in range(32) for r in (given[k], given[32 + k], given[64])]
    return batch, rows


def wave1_with_a_wide_job(hal, given, out):
    """the same 32 jobs plus ONE 16-slot job of one output element (15 products of bit pairs, all before the first sum): it sets the
    launch's LDS to 64 KiB for every workgroup -- what that costs the two-slot jobs"""
    k = 15
    wide = [("var", i) for i in range(2 * k)] + [("mul", 2 * i, 2 * i + 1) for i in range(k)] + [("add", 2 * k, 2 * k + 1)]
    for i in range(2, k):
        wide.append(("add", len(wide) - 1, 2 * k + i))
    members = [hal.expr_compile_tower(SELECT, [0, 0, 0], 0), hal.expr_compile_tower(wide, [0] * (2 * k), 0)]
    n = elems(0, ROWS)
    batch = hal.expr_compile_tower_batch(members, [(0, 3 * k2, ROWS, k2 * n) for k2 in range(32)] + [(1, 96, 7, 32 * n)])
    rows = [r for k2 in range(32) for r in (given[k2], given[32 + k2], given[64])] + given[: 2 * k]
    return batch, rows


def wave1_as_the_plan_does_it(hal, given, out):
    """compile, batch, call, frees: what one wave of the batched plan costs"""
    batch, rows = wave1_batch(hal, given, out)
    hal.compute_composite_tower_batch(rows, out, batch)
    for e in hal._exprs[-2:]:
        e.free()
    del hal._exprs[-2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one shape (select, pack_fp, product, plan, plan_batched, wave1): for a counter run of that kernel alone")
    args = ap.parse_args()
    import numpy as np

    import binius_amd
    from binius_amd._host import WitnessCompute, WitnessComputeBatched

    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    want = lambda name: args.only in (None, name)  # noqa: E731
    with binius_amd.Context(0, 16 << 20) as hal:
        alloc = hal.dev_alloc()
        half = 2 * elems(0, ROWS + 6) + 1
        src, dst = alloc.alloc(half), alloc.alloc(half)
        hal.fill(src, 3)
        if want("select"):
            emit(one_call(hal, alloc, np, "select", SELECT, [0, 0, 0], 0, ROWS + 6, src, dst, args.runs, host_select))
        if want("pack_fp"):
            emit(one_call(hal, alloc, np, "pack_fp", pack_steps(32), [0] * 32, 5, ROWS, src, dst, args.runs, host_pack))
        if want("product"):
            emit(one_call(hal, alloc, np, "product", [("var", 0), ("var", 1), ("mul", 0, 1)], [5, 5], 5, ROWS, src, dst, args.runs, None))
        if want("plan"):
            cols, given = plan_columns(hal, alloc)
            scratch = alloc.alloc(WitnessCompute.scratch_elems(cols))
            plan = WitnessCompute(hal, cols, scratch)
            # bytes: every computed column reads its inputs and writes itself
            read = 32 * 3 * elems(0, ROWS) + 32 * elems(0, ROWS) + elems(0, ROWS)
            written = 32 * elems(0, ROWS) + elems(5, ROWS) + elems(0, ROWS)
            timings = windows(hal, plan.run, read, written, src, dst, args.runs)
            got = plan.run()
            host_ins = [np.ascontiguousarray(hal.copy_d2h(d)) for d in given]
            fill_ms, (sel, packed, shifted) = host_timed(lambda: host_plan(np, host_ins), max(3, args.runs // 4))
            assert np.array_equal(hal.copy_d2h(got[97][0]).reshape(-1), packed.view(np.uint64)), "plan: the host path and the device disagree (pack_fp)"
            assert np.array_equal(hal.copy_d2h(got[98][0]).reshape(-1), shifted.view(np.uint64)), "plan: the host path and the device disagree (shifted)"
            assert np.array_equal(hal.copy_d2h(got[65 + 31][0]).reshape(-1), sel[31]), "plan: the host path and the device disagree (composite)"
            out_host = np.frombuffer(b"".join(c.tobytes() for c in sel + [packed, shifted]), dtype=np.uint64).reshape(-1, 2)
            assert out_host.shape[0] == written
            rec = {"shape": "plan", "columns": len(cols), "waves": plan.n_waves, "launches_per_run": plan.n_launches}
            emit(finish(hal, alloc, rec, timings, read, written, fill_ms, out_host, args.runs))
        if want("plan_batched") or args.only == "wave1":
            cols, given = plan_columns(hal, alloc)
            n_scratch = WitnessCompute.scratch_elems(cols)
            plan_d, plan_e = WitnessCompute(hal, cols, alloc.alloc(n_scratch)), WitnessComputeBatched(hal, cols, alloc.alloc(n_scratch))
            wave_out = alloc.alloc(32 * elems(0, ROWS) + 1)
            batch, rows = wave1_batch(hal, given, wave_out)
            wave_call = lambda: hal.compute_composite_tower_batch(rows, wave_out, batch)  # noqa: E731
            if args.only == "wave1":
                t = timed(hal, wave_call, args.runs)
                emit({"shape": "wave1", "jobs": 32, "call": stats(t)})
            else:
                read = 32 * 3 * elems(0, ROWS) + 32 * elems(0, ROWS) + elems(0, ROWS)
                written = 32 * elems(0, ROWS) + elems(5, ROWS) + elems(0, ROWS)
                wave_both = (32 * 3 * elems(0, ROWS) + 32 * elems(0, ROWS)) // 2
                d1 = timed(hal, plan_d.run, args.runs)
                e1 = timed(hal, plan_e.run, args.runs)
                both = (read + written) // 2
                copy = timed(hal, lambda: hal.copy_d2d(src.slice(0, both), dst.slice(0, both)), args.runs)
                d2 = timed(hal, plan_d.run, args.runs)
                e2 = timed(hal, plan_e.run, args.runs)
                c0 = hal.compute_composite_batch_counters()
                w_call = timed(hal, wave_call, args.runs)
                c1 = hal.compute_composite_batch_counters()
                w_copy = timed(hal, lambda: hal.copy_d2d(src.slice(0, wave_both), dst.slice(0, wave_both)), args.runs)
                w_plan = timed(hal, lambda: wave1_as_the_plan_does_it(hal, given, wave_out), args.runs)
                wide_batch, wide_rows = wave1_with_a_wide_job(hal, given, wave_out)
                w_wide = timed(hal, lambda: hal.compute_composite_tower_batch(wide_rows, wave_out, wide_batch), args.runs)
                w_call2 = timed(hal, wave_call, args.runs)
                got_d, got_e = plan_d.run(), plan_e.run()
                host_ins = [np.ascontiguousarray(hal.copy_d2h(d)) for d in given]
                sel, packed, shifted = host_plan(np, host_ins)
                for name, got in (("per column", got_d), ("batched", got_e)):
                    assert np.array_equal(hal.copy_d2h(got[97][0]).reshape(-1), packed.view(np.uint64)), "%s plan: the host path and the device disagree (pack_fp)" % name
                    assert np.array_equal(hal.copy_d2h(got[98][0]).reshape(-1), shifted.view(np.uint64)), "%s plan: the host path and the device disagree (shifted)" % name
                    for k in range(32):
                        assert np.array_equal(hal.copy_d2h(got[65 + k][0]).reshape(-1), sel[k]), "%s plan: the host path and the device disagree (composite %d)" % (name, k)
                n = elems(0, ROWS)
                for k in range(32):
                    assert np.array_equal(hal.copy_d2h(wave_out.slice(k * n, (k + 1) * n)).reshape(-1), sel[k]), "the wave-1 batch and the host path disagree (%d)" % k
                d, e, f = stats(d1 + d2), stats(e1 + e2), stats(copy)
                wc, wf = stats(w_call), stats(w_copy)
                emit({"shape": "plan_batched", "columns": len(cols), "waves": plan_e.n_waves, "launches_per_run": plan_e.n_launches, "per_column_launches_per_run": plan_d.n_launches,
                      "bytes_read": 16 * read, "bytes_written": 16 * written, "compute": e, "compute_first_window": stats(e1), "compute_second_window": stats(e2),
                      "per_column_plan_same_session": d, "per_column_first_window": stats(d1), "per_column_second_window": stats(d2),
                      "per_column_over_batched": round(d["median_ms"] / e["median_ms"], 2), "batched_median_below_per_column_min": e["median_ms"] < d["min_ms"],
                      "copy_read_plus_written_bytes": f, "compute_over_copy": round(e["median_ms"] / f["median_ms"], 3),
                      "wave1_bytes": 32 * wave_both, "wave1_call": wc, "wave1_launches_per_call": (c1["launches"] - c0["launches"]) // (c1["calls"] - c0["calls"]),
                      "wave1_copy_read_plus_written_bytes": wf, "wave1_call_over_copy": round(wc["median_ms"] / wf["median_ms"], 3),
                      "wave1_compile_batch_call_free": stats(w_plan), "wave1_call_again": stats(w_call2), "wave1_call_with_one_16_slot_job_64KiB_lds": stats(w_wide)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
