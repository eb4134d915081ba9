"""The GKR exponentiation witness on the device: (a) bn_exp_circuit_layers against (b) the route that produces the same layers without
it -- the bit columns expanded to 16 bytes per row (here by ONE bn_bits_to_b128 call for all columns of a witness, the cheapest form
of that step; its time counts) and one bn_compute_composite per layer and witness -- for single witnesses of 2^12, 2^16 and 2^20
rows at widths 8, 32 and 64, static and dynamic, and for a batch of 64 witnesses of 2^10 rows; and the whole bnh_gkr_exp_prove at
width 32 with its wall time per layer and its launch counters.  JSON lines on stdout.

Both arms run in the same process on the same resident inputs, alternating call by call; a call is timed by the host clock and ends
with the device idle (arm a synchronises itself, arm b ends in bn_sync).  The ctypes arguments of both arms are marshalled before the
timed window.  Reported: median, 10th and 90th percentile over the runs, the layers compared bit for bit, the op's share of the time
the arena write alone would take (width x 16 B x rows at 8 TB/s: a bandwidth bound, which the op -- bound by VALU -- is far from).

    python tools/bench_gkr_exp.py [--runs 30] [--sizes 12,16,20] [--widths 8,32,64] [--prove 16,20] [--no-batch]
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
from binius_amd._ffi import F128, lib, to_f128  # noqa: E402
from binius_amd._host import GkrExpPlan  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def pct(xs):
    a = np.sort(np.asarray(xs))
    return {"median_us": round(float(np.median(a)) * 1e6, 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]) * 1e6, 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]) * 1e6, 2)}


def random_bit_column(seed, rows):
    """A packed bit column: rows bits in max(1, rows / 128) elements."""
    return synthetic.random_b128(seed, max(1, rows >> 7))


def mul_host(a, b):
    from binius_amd._ffi import HostField

    return HostField.mul(a, b)


class Witnesses:
    """k witnesses of 2^n rows and `width` bits on the device with both arms' arguments ready."""

    def __init__(self, hal, alloc, n, width, dynamic, k, seed):
        self.hal, self.n, self.w, self.k, self.dynamic = hal, n, width, k, dynamic
        rows = 1 << n
        self.cols, self.bases, self.arenas_a, self.arenas_b, self.expanded = [], [], [], [], []
        g = synthetic.random_scalars(seed, 1)[0]
        for t in range(k):
            cs = []
            for j in range(width):
                c = alloc.alloc(max(1, rows >> 7))
                hal.copy_h2d(random_bit_column(seed + 1000 * t + j, rows), c)
                cs.append(c)
            self.cols.append(cs)
            if dynamic:
                b = alloc.alloc(rows)
                hal.copy_h2d(synthetic.random_b128(seed + 1000 * t + 999, rows), b)
                self.bases.append(b)
            else:
                self.bases.append(g)
            self.arenas_a.append(alloc.alloc(width * rows))
            self.arenas_b.append(alloc.alloc(width * rows))
            self.expanded.append(alloc.alloc(width * rows))
        # arm a
        self.nv = (C.c_uint32 * k)(*([n] * k))
        self.wd = (C.c_uint32 * k)(*([width] * k))
        self.kd = (C.c_uint32 * k)(*([1 if dynamic else 0] * k))
        self.cp = (C.c_void_p * (k * width))(*[c.ptr for cs in self.cols for c in cs])
        self.sb = (F128 * k)(*[to_f128(0 if dynamic else g) for _ in range(k)])
        self.db = (C.c_void_p * k)(*[(b.ptr if dynamic else None) for b in self.bases])
        self.outs = (C.c_void_p * k)(*[a.ptr for a in self.arenas_a])
        # arm b: one expansion call per witness, then one compute_composite per layer
        self.exp_ll = (C.c_uint32 * width)(*([n] * width))
        self.exp_calls, self.calls, self.exprs = [], [], []
        sel = lambda c: [("var", 1), c, ("mul", 0, 1), ("const", 1), ("add", 3, 0), ("add", 4, 2)]  # (1 + x1) + x1 c
        for t in range(k):
            srcs = (C.c_void_p * width)(*[c.ptr for c in self.cols[t]])
            dsts = (C.c_void_p * width)(*[self.expanded[t].ptr + 16 * rows * j for j in range(width)])
            self.exp_calls.append((srcs, dsts))
            power = g
            for layer in range(width):
                bit = (width - 1 - layer) if dynamic else layer
                e_ptr = self.expanded[t].ptr + 16 * rows * bit
                dst = self.arenas_b[t].ptr + 16 * rows * layer
                prev = self.arenas_b[t].ptr + 16 * rows * (layer - 1)
                if dynamic:
                    if layer == 0:
                        steps = [("var", 1), ("var", 2), ("mul", 0, 1), ("const", 1), ("add", 3, 0), ("add", 4, 2)]
                    else:
                        steps = [("var", 1), ("var", 2), ("mul", 0, 1), ("const", 1), ("add", 3, 0), ("add", 4, 2), ("var", 0), ("pow", 6, 2), ("mul", 7, 5)]
                    rows_p = (C.c_void_p * 3)(prev if layer else e_ptr, e_ptr, self.bases[t].ptr)
                    n_rows = 3
                else:
                    steps = sel(("const", power))
                    if layer:
                        steps = steps + [("var", 0), ("mul", 6, 5)]
                    rows_p = (C.c_void_p * 2)(prev if layer else e_ptr, e_ptr)
                    n_rows = 2
                    power = mul_host(power, power)
                expr = hal.compile_expr(steps)
                self.exprs.append(expr)
                self.calls.append((rows_p, n_rows, dst, expr.handle))

    def arm_a(self):
        rc = lib().bn_exp_circuit_layers(self.hal._h, self.k, self.nv, self.wd, self.kd, self.cp, self.sb, self.db, self.outs)
        assert rc == 0

    def arm_b(self):
        L, h, rows = lib(), self.hal._h, 1 << self.n
        for srcs, dsts in self.exp_calls:
            rc = L.bn_bits_to_b128(h, self.w, self.exp_ll, srcs, dsts)
            assert rc == 0
        for rows_p, n_rows, dst, e in self.calls:
            rc = L.bn_compute_composite(h, rows_p, n_rows, rows, dst, rows, e)
            assert rc == 0
        self.hal.sync()

    def same_layers(self):
        return all(np.array_equal(self.hal.copy_d2h(a), self.hal.copy_d2h(b)) for a, b in zip(self.arenas_a, self.arenas_b))


def bench_op(hal, n, width, dynamic, k, runs, warmup=5):
    alloc = hal.dev_alloc()
    ws = Witnesses(hal, alloc, n, width, dynamic, k, 0x7E0A0000 + 4096 * n + 16 * width + int(dynamic))
    c0 = hal.exp_counters()
    ws.arm_a()
    launches = hal.exp_counters()["launches"] - c0["launches"]
    for _ in range(warmup):
        ws.arm_a()
        ws.arm_b()
    ta, tb = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        ws.arm_a()
        t1 = time.perf_counter()
        ws.arm_b()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    a, b = pct(ta), pct(tb)
    write_bytes = k * width * 16 * (1 << n)
    return {"what": "exp_circuit_layers vs per-layer compute_composite over expanded bit columns", "n_vars": n, "width": width,
            "kind": "dynamic" if dynamic else "static", "witnesses": k, "runs": runs, "op": a, "per_layer": b, "op_launches": launches,
            "per_layer_launches": k * (width + 1), "speedup_median": round(b["median_us"] / a["median_us"], 3),
            "not_slower": a["median_us"] <= b["median_us"], "arena_write_bytes": write_bytes,
            "write_bound_share_of_call": round(write_bytes / HBM_BYTES_PER_S / (a["median_us"] * 1e-6), 4), "same_layers": ws.same_layers()}


def bench_prove(hal, n, width, runs):
    """One static and one dynamic claim of 2^n rows; the claims' evaluations are taken from a first run's layers on the device."""
    alloc = hal.dev_alloc()
    rows = 1 << n
    cols, bases, arenas = [], [], []
    for t, dynamic in enumerate((False, True)):
        cs = []
        for j in range(width):
            c = alloc.alloc(max(1, rows >> 7))
            hal.copy_h2d(random_bit_column(0x7E0B0000 + 1000 * t + j, rows), c)
            cs.append(c)
        cols.append(cs)
        if dynamic:
            b = alloc.alloc(rows)
            hal.copy_h2d(synthetic.random_b128(0x7E0B9999, rows), b)
            bases.append(b)
        else:
            bases.append(synthetic.random_scalars(0x7E0B8888, 1)[0])
        arenas.append(alloc.alloc(width * rows))
    point = synthetic.random_scalars(0x7E0C, n)
    # the claims: the result layers' evaluations at the point (tensor expansion + inner product on the device)
    hal.exp_circuit_layers([n, n], cols, bases, arenas)
    eq = alloc.alloc(rows)
    hal.fill(eq.slice(0, 1), 1)
    hal.tensor_expand(0, point, eq)
    evals = [hal.inner_product(a.slice((width - 1) * rows, width * rows), 7, eq) for a in arenas]
    scratch = alloc.alloc(GkrExpPlan.scratch_elems([n, n], [False, True]))
    bc = [synthetic.random_scalars(0x7E0D + L, 2) for L in range(width)]
    ch = [synthetic.random_scalars(0x7E0E + L, n) for L in range(width)]
    plan = GkrExpPlan(hal, [n, n], cols, bases, arenas, [point, point], evals, scratch, bc, ch)
    plan.run()  # warm-up (every layer's shapes)
    total, layers = [], []
    c0 = hal.exp_counters()
    for _ in range(runs):
        hal.sync()
        t0 = time.perf_counter()
        plan.run()
        total.append(time.perf_counter() - t0)
        layers.append(plan.layer_times_ms())
    c1 = hal.exp_counters()
    mid = int(np.argsort(total)[len(total) // 2])
    return {"what": "bnh_gkr_exp_prove", "n_vars": n, "width": width, "claims": "one static, one dynamic", "runs": runs,
            "total_ms_median": round(total[mid] * 1e3, 3), "total_ms_min": round(min(total) * 1e3, 3), "total_ms_max": round(max(total) * 1e3, 3),
            "witness_ms": round(total[mid] * 1e3 - sum(layers[mid]), 3), "layer_ms": [round(x, 3) for x in layers[mid]],
            "exp_circuit_launches_per_prove": (c1["launches"] - c0["launches"]) // runs, "bits_to_b128_launches_per_prove": (c1["bits_launches"] - c0["bits_launches"]) // runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--widths", default="8,32,64")
    ap.add_argument("--prove", default="16,20")
    ap.add_argument("--prove-runs", type=int, default=5)
    ap.add_argument("--no-batch", action="store_true")
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes.split(",") if v]
    widths = [int(v) for v in args.widths.split(",") if v]
    prove = [int(v) for v in args.prove.split(",") if v]
    biggest = max([3 * w << n for n in sizes for w in widths] + [64 * 3 * 64 << 10] + [(2 * 32 + 8) << n for n in prove] + [1 << 20])
    with binius_amd.Context(0, biggest + (8 << max(sizes + prove + [10])) + (1 << 22)) as hal:
        for n in sizes:
            for w in widths:
                for dynamic in (False, True):
                    print(json.dumps(bench_op(hal, n, w, dynamic, 1, args.runs)), flush=True)
        if not args.no_batch:
            for dynamic in (False, True):
                print(json.dumps(bench_op(hal, 10, 32, dynamic, 64, args.runs)), flush=True)
        for n in prove:
            print(json.dumps(bench_prove(hal, n, 32, args.prove_runs)), flush=True)


if __name__ == "__main__":
    main()
