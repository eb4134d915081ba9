"""The flush witnesses on the device: (a) ONE bn_flush_witness_batch for a batch of flushes against (b) what the library offers without
it on the same resident inputs -- per flush one bn_bits_to_b128 for its selectors, one bn_partial_eval_high_batch(query_vars = 0) that
widens its columns to 16 bytes per row, and one bn_compute_composite with 1 + S * L (or L alone without a selector) -- for 1, 8 and
32 flushes of 2^20 and 2^24 rows in four shapes: 2 x B32 + 1 x B8 columns under one selector (a typical lookup), the same with the
selector cut at 3/5 of the table, 6 x B32 columns, 2 x B128 columns.  A second mode times bnh_flush_prodcheck_prove by phase.
JSON lines on stdout.

Both arms run in the same process, alternating call by call; a call is timed by the host clock and ends with the device idle (arm a
synchronises itself, arm b ends in bn_sync).  The ctypes arguments of both arms are marshalled before the timed window; arm b reuses
one set of widened columns for all flushes, arm a and arm b write separate outputs, which are compared bit for bit over the prefix
that arm a writes.  Reported: median, 10th and 90th percentile over the runs, launches per call, and the bytes the op has to move
(columns + selectors read, 16 B per row of the prefix written) per second as a share of 8 TB/s.

    python tools/bench_flush.py [--runs 20] [--sizes 20,24] [--batches 1,8,32] [--prove 16,20]
"""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import binius_amd  # noqa: E402
from binius_amd import synthetic  # noqa: E402
from binius_amd._ffi import F128, DevSlice, PeColumn, lib, to_f128  # noqa: E402
from binius_amd._host import FlushProdcheckPlan  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
SHAPES = {"lookup_2xB32_1xB8_sel": ([5, 5, 3], 1.0), "lookup_sel_cut_3_5": ([5, 5, 3], 0.6), "6xB32": ([5] * 6, None), "2xB128": ([7, 7], None)}


def pct(xs):
    a = np.sort(np.asarray(xs))
    return {"median_us": round(float(np.median(a)) * 1e6, 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]) * 1e6, 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]) * 1e6, 2)}


def col_elems(n, level):
    return max(1, (1 << (n + level)) >> 7)


class Batch:
    """k flushes of 2^n rows of one shape on the device with both arms' arguments ready.  Every column has its own memory; the data
    of all columns are prefixes of one random host buffer."""

    def __init__(self, hal, alloc, host_data, n, levels, sel_frac, k, seed):
        self.hal, self.n, self.k, self.levels = hal, n, k, levels
        rows = 1 << n
        self.has_sel = sel_frac is not None
        coeffs = synthetic.random_scalars(seed, len(levels) + 1)
        coeffs[0] = 1  # the first mixing power
        const_term = coeffs.pop()
        self.cols, self.sels, self.out_a, self.out_b = [], [], [], []
        sel_host = None
        if self.has_sel:
            sel_host = host_data[: col_elems(n, 0)].copy()
            cut = int(rows * sel_frac) >> 7
            sel_host[cut:] = 0  # (whole 16-byte elements: the prefix is 128 * cut; for sel_frac = 1 nothing is cut)
        for _ in range(k):
            cs = []
            for level in levels:
                c = alloc.alloc(col_elems(n, level))
                hal.copy_h2d(host_data[: c.len], c)
                cs.append(c)
            self.cols.append(cs)
            if self.has_sel:
                s = alloc.alloc(col_elems(n, 0))
                hal.copy_h2d(sel_host, s)
                self.sels.append(s)
            self.out_a.append(alloc.alloc(rows))
            self.out_b.append(alloc.alloc(rows))
        m = len(levels)
        self.wide = [alloc.alloc(rows) for _ in range(m + (1 if self.has_sel else 0))]
        self.one = alloc.alloc(1)
        hal.fill(self.one, 1)
        # arm a
        self.a_nv = (C.c_uint32 * k)(*([n] * k))
        self.a_ns = (C.c_uint32 * k)(*([1 if self.has_sel else 0] * k))
        self.a_sp = (C.c_void_p * max(1, len(self.sels)))(*[s.ptr for s in self.sels])
        self.a_nc = (C.c_uint32 * k)(*([m] * k))
        self.a_cp = (C.c_void_p * (k * m))(*[c.ptr for cs in self.cols for c in cs])
        self.a_lv = (C.c_uint32 * (k * m))(*(levels * k))
        self.a_cf = (F128 * (k * m))(*[to_f128(c) for _ in range(k) for c in coeffs])
        self.a_ct = (F128 * k)(*[to_f128(const_term) for _ in range(k)])
        self.a_out = (C.c_void_p * k)(*[o.ptr for o in self.out_a])
        self.a_len = (C.c_uint64 * k)()
        # arm b: L = const + sum coeff_j x_j over the widened columns; with a selector x_m: 1 + x_m * (L + 1)
        steps = [("const", const_term ^ (1 if self.has_sel else 0))]
        acc = 0
        for j, c in enumerate(coeffs):
            steps += [("var", j), ("const", c), ("mul", len(steps), len(steps) + 1)]
            steps.append(("add", acc, len(steps) - 1))
            acc = len(steps) - 1
        if self.has_sel:
            steps += [("var", m), ("mul", len(steps), acc), ("const", 1)]
            steps.append(("add", len(steps) - 1, len(steps) - 2))
        self.expr = hal.compile_expr(steps)
        self.b_calls = []
        self.b_ll = (C.c_uint32 * 1)(n)
        self.b_wide = (C.c_void_p * m)(*[w.ptr for w in self.wide[:m]])
        self.b_rows = (C.c_void_p * len(self.wide))(*[w.ptr for w in self.wide])
        for t in range(k):
            pe = (PeColumn * m)(*[PeColumn(c.ptr, level, n) for c, level in zip(self.cols[t], levels)])
            sel_src = (C.c_void_p * 1)(self.sels[t].ptr) if self.has_sel else None
            sel_dst = (C.c_void_p * 1)(self.wide[m].ptr) if self.has_sel else None
            self.b_calls.append((pe, sel_src, sel_dst, self.out_b[t].ptr))

    def arm_a(self):
        rc = lib().bn_flush_witness_batch(self.hal._h, self.k, self.a_nv, self.a_ns, self.a_sp, self.a_nc, self.a_cp, self.a_lv, self.a_cf, self.a_ct,
                                          self.a_out, self.a_len)
        assert rc == 0, lib().bn_last_error()

    def arm_b(self):
        L, h, rows, m = lib(), self.hal._h, 1 << self.n, len(self.levels)
        for pe, sel_src, sel_dst, dst in self.b_calls:
            if sel_src is not None:
                rc = L.bn_bits_to_b128(h, 1, self.b_ll, sel_src, sel_dst)
                assert rc == 0
            rc = L.bn_partial_eval_high_batch(h, C.cast(pe, C.c_void_p), m, self.one.ptr, 0, self.b_wide)
            assert rc == 0, L.bn_last_error()
            rc = L.bn_compute_composite(h, self.b_rows, len(self.wide), rows, dst, rows, self.expr.handle)
            assert rc == 0, L.bn_last_error()
        self.hal.sync()

    def same_outputs(self):
        for t in range(self.k):
            p = int(self.a_len[t])
            if p and not np.array_equal(self.hal.copy_d2h(DevSlice(self.out_a[t].ptr, p)), self.hal.copy_d2h(DevSlice(self.out_b[t].ptr, p))):
                return False
        return True

    def moved_bytes(self):
        per = sum(16 * col_elems(self.n, level) for level in self.levels) + (16 * col_elems(self.n, 0) if self.has_sel else 0)
        return self.k * per + 16 * sum(int(self.a_len[t]) for t in range(self.k))


def bench_op(hal, host_data, shape, n, k, runs, warmup=3):
    levels, sel_frac = SHAPES[shape]
    alloc = hal.dev_alloc()
    b = Batch(hal, alloc, host_data, n, list(levels), sel_frac, k, 0x7F0A0000 + 64 * n + k)
    c0 = hal.flush_counters()
    b.arm_a()
    c1 = hal.flush_counters()
    b.arm_b()
    same = b.same_outputs()
    for _ in range(warmup):
        b.arm_a()
        b.arm_b()
    ta, tb = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        b.arm_a()
        t1 = time.perf_counter()
        b.arm_b()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    a, pb = pct(ta), pct(tb)
    moved = b.moved_bytes()
    return {"what": "flush_witness_batch vs bits_to_b128 + partial_eval_high_batch + compute_composite per flush", "shape": shape, "n_vars": n, "flushes": k,
            "runs": runs, "op": a, "parent_route": pb, "op_launches": c1["launches"] - c0["launches"], "multipass_flushes": c1["multipass"] - c0["multipass"],
            "prefix_len": int(b.a_len[0]), "speedup_median": round(pb["median_us"] / a["median_us"], 3), "not_slower": a["median_us"] <= pb["median_us"],
            "moved_bytes": moved, "share_of_8TBps": round(moved / HBM_BYTES_PER_S / (a["median_us"] * 1e-6), 4), "same_outputs": same}


def bench_prove(hal, host_data, n, runs):
    """A lookup-shaped system: one composite flush (2 x B32 + B8 under a selector cut at 3/5), one linear flush over the same columns
    and one non-zero B16 oracle, all of 2^n rows.  (The non-zero column is all ones: random data has zero rows.)"""
    alloc = hal.dev_alloc()
    rows = 1 << n

    def put(level, data=None):
        c = alloc.alloc(col_elems(n, level))
        hal.copy_h2d(host_data[: c.len] if data is None else data, c)
        return c

    sel_host = host_data[: col_elems(n, 0)].copy()
    sel_host[(rows * 3 // 5) >> 7 :] = 0
    a, b, c, s = put(5), put(5), put(3), put(0, sel_host)
    ones = np.zeros((col_elems(n, 4), 2), dtype=np.uint64)
    ones[:] = 0x0001000100010001
    nzc = put(4, ones)
    flushes = [{"channel": 0, "n_vars": n, "selectors": [(9, s)], "entries": [("oracle", 1, a, 5), ("oracle", 2, b, 5), ("const", 5), ("oracle", 3, c, 3)]},
               {"channel": 1, "n_vars": n, "selectors": [], "entries": [("oracle", 1, a, 5), ("oracle", 2, b, 5), ("oracle", 3, c, 3)]}]
    nonzero = [(4, nzc, 4, n)]
    scratch = alloc.alloc(FlushProdcheckPlan.scratch_elems(flushes, nonzero))
    S = synthetic.random_scalars
    plan = FlushProdcheckPlan(hal, flushes, nonzero, S(0x7F0B, 1)[0], S(0x7F0C, 2), scratch, S(0x7F0D, n), [S(0x7F10 + j, max(1, j))[:j] for j in range(n)],
                              S(0x7F0E, n), S(0x7F0F, 1), [S(0x7F11, n)])
    plan.run()  # warm-up
    total, phases = [], []
    for _ in range(runs):
        hal.sync()
        t0 = time.perf_counter()
        plan.run()
        total.append(time.perf_counter() - t0)
        phases.append(plan.phase_times_ms())
    mid = int(np.argsort(total)[len(total) // 2])
    return {"what": "bnh_flush_prodcheck_prove", "n_vars": n, "system": "one composite flush (2 x B32 + B8, selector cut at 3/5), one linear flush, one non-zero B16 oracle",
            "runs": runs, "total_ms_median": round(total[mid] * 1e3, 3), "total_ms_min": round(min(total) * 1e3, 3), "total_ms_max": round(max(total) * 1e3, 3),
            "phase_ms": {key: round(v, 3) for key, v in phases[mid].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--prove", default="16,20")
    ap.add_argument("--prove-runs", type=int, default=5)
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes.split(",") if v]
    batches = [int(v) for v in args.batches.split(",") if v]
    shapes = [v for v in args.shapes.split(",") if v]
    prove = [int(v) for v in args.prove.split(",") if v]
    top = max(sizes + prove + [10])
    # per flush: its columns (at most 2 x 2^n elements: two B128 columns, or six B32 ones), a selector, two outputs; seven widened columns
    per_flush = (2 << top) + (2 << top) + (1 << top >> 7) + 64
    need = max([max(batches + [1]) * per_flush + (8 << top)] + [40 << p for p in prove]) + (1 << 20)
    host_data = synthetic.random_b128(0x7F000001, 1 << top)
    with binius_amd.Context(0, need) as hal:
        for shape in shapes:
            for n in sizes:
                for k in batches:
                    print(json.dumps(bench_op(hal, host_data, shape, n, k, args.runs)), flush=True)
        for n in prove:
            print(json.dumps(bench_prove(hal, host_data, n, args.prove_runs)), flush=True)


if __name__ == "__main__":
    main()
