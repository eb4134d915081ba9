"""The GKR grand-product argument on the device: (a) bn_product_tree_layers against (b) the path that produces the same layers
without it -- log n calls of compute_composite on the halves, exactly as ProductCircuitLayers::compute issues them
(binius_amd/host/callers.hpp: one launch per layer, then the product read back) -- for single trees and for a batch of 64 trees of
2^14; and the whole bnh_gkr_gpa_prove for 8 trees with its per-step wall time.  JSON lines on stdout.

Both arms run in the same process on the same resident inputs, alternating call by call; a call is timed by the host clock and
ends with the product on the host (arm a: the result mailbox; arm b: a one-element copy_d2h), i.e. with the device idle.  The
ctypes arguments of both arms are marshalled before the timed window.  Reported: median, 10th and 90th percentile over the runs.

    python tools/bench_gkr_gpa.py [--runs 30] [--sizes 12,16,20,24] [--prove 16,20,22] [--no-batch]
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
from binius_amd._ffi import F128, lib  # noqa: E402
from binius_amd._host import GkrGpaPlan  # noqa: E402


def pct(xs):
    a = np.sort(np.asarray(xs))
    return {"median_us": round(float(np.median(a)) * 1e6, 2), "p10_us": round(float(a[int(0.1 * (len(a) - 1))]) * 1e6, 2),
            "p90_us": round(float(a[int(round(0.9 * (len(a) - 1)))]) * 1e6, 2)}


class Trees:
    """k trees of 2^n on the device with both arms' arguments ready."""

    def __init__(self, hal, alloc, n, k, seed):
        self.hal, self.n, self.k = hal, n, k
        self.inputs, self.arenas_a, self.arenas_b = [], [], []
        for t in range(k):
            d = alloc.alloc(1 << n)
            hal.copy_h2d(synthetic.random_b128(seed + t, 1 << n), d)
            self.inputs.append(d)
            self.arenas_a.append(alloc.alloc(1 << n))
            self.arenas_b.append(alloc.alloc(1 << n))
        self.nv = (C.c_uint32 * k)(*([n] * k))
        self.ins = (C.c_void_p * k)(*[x.ptr for x in self.inputs])
        self.lens = (C.c_uint64 * k)(*[x.len for x in self.inputs])
        self.outs = (C.c_void_p * k)(*[a.ptr for a in self.arenas_a])
        self.prod = (F128 * k)()
        self.expr = hal.compile_expr([("var", 0), ("var", 1), ("mul", 0, 1)])
        # arm b: per tree, layer j = halves of layer j + 1 (the input for j = n - 1), into the heap-ordered arena
        self.calls = []
        for t in range(k):
            src = self.inputs[t].ptr
            for j in range(n - 1, -1, -1):
                half = 1 << j
                rows = (C.c_void_p * 2)(src, src + 16 * half)
                dst = self.arenas_b[t].ptr + 16 * half
                self.calls.append((rows, half, dst))
                src = dst
        self.top = np.zeros((1, 2), dtype=np.uint64)

    def arm_a(self):
        rc = lib().bn_product_tree_layers(self.hal._h, self.k, self.nv, self.ins, self.lens, self.outs, self.prod)
        assert rc == 0

    def arm_b(self):
        L, h, e = lib(), self.hal._h, self.expr.handle
        for rows, half, dst in self.calls:
            rc = L.bn_compute_composite(h, rows, 2, half, dst, half, e)
            assert rc == 0
        for t in range(self.k):  # (the product of every tree, as ProductCircuitLayers::compute reads it)
            rc = L.bn_copy_d2h(h, self.arenas_b[t].ptr + 16, 1, self.top.ctypes.data, 1)
            assert rc == 0

    def same_layers(self):
        for a, b in zip(self.arenas_a, self.arenas_b):
            if not np.array_equal(self.hal.copy_d2h(a)[1:], self.hal.copy_d2h(b)[1:]):
                return False
        return True


def bench_op(hal, n, k, runs, warmup=5):
    alloc = hal.dev_alloc()
    tr = Trees(hal, alloc, n, k, 0x6B9A0000 + 256 * n)
    for _ in range(warmup):
        tr.arm_a()
        tr.arm_b()
    ta, tb = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        tr.arm_a()
        t1 = time.perf_counter()
        tr.arm_b()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    a, b = pct(ta), pct(tb)
    spread_b = b["p90_us"] - b["p10_us"]
    return {"what": "product_tree_layers vs per-level compute_composite", "n_vars": n, "trees": k, "runs": runs, "op": a, "per_level": b,
            "per_level_launches": n * k, "speedup_median": round(b["median_us"] / a["median_us"], 3), "per_level_spread_us": round(spread_b, 2),
            "not_slower_within_spread": a["median_us"] <= b["median_us"] + spread_b, "faster": a["median_us"] < b["median_us"],
            "same_layers": tr.same_layers()}


def bench_prove(hal, n, k, runs):
    alloc = hal.dev_alloc()
    inputs, arenas = [], []
    for t in range(k):
        d = alloc.alloc(1 << n)
        hal.copy_h2d(synthetic.random_b128(0x6B9B0000 + 256 * n + t, 1 << n), d)
        inputs.append(d)
        arenas.append(alloc.alloc(1 << n))
    nv = [n] * k
    scratch = alloc.alloc(GkrGpaPlan.scratch_elems(nv))
    bc, gc = synthetic.random_scalars(0x6B9C, n), synthetic.random_scalars(0x6B9D, n)
    flat = synthetic.random_scalars(0x6B9E, n * (n - 1) // 2 + 1)
    sc, off = [], 0
    for j in range(n):
        sc.append(flat[off : off + j])
        off += j
    plan = GkrGpaPlan(hal, nv, inputs, arenas, scratch, bc, sc, gc)
    plan.run()  # warm-up (every step's shapes)
    total, steps = [], []
    for _ in range(runs):
        hal.sync()
        t0 = time.perf_counter()
        plan.run()
        total.append(time.perf_counter() - t0)
        steps.append(plan.step_times_ms())
    mid = int(np.argsort(total)[len(total) // 2])
    return {"what": "bnh_gkr_gpa_prove", "n_vars": n, "trees": k, "runs": runs, "total_ms_median": round(total[mid] * 1e3, 3),
            "total_ms_min": round(min(total) * 1e3, 3), "total_ms_max": round(max(total) * 1e3, 3),
            "witness_and_padding_ms": round(total[mid] * 1e3 - sum(steps[mid]), 3), "step_ms": [round(x, 3) for x in steps[mid]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--sizes", default="12,16,20,24")
    ap.add_argument("--prove", default="16,20,22")
    ap.add_argument("--prove-runs", type=int, default=5)
    ap.add_argument("--no-batch", action="store_true")
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes.split(",") if v]
    prove = [int(v) for v in args.prove.split(",") if v]
    elems = max([3 << n for n in sizes] + [64 * 3 << 14] + [8 * 3 << n for n in prove] + [1 << 20]) + (1 << 22)
    with binius_amd.Context(0, elems) as hal:
        for n in sizes:
            print(json.dumps(bench_op(hal, n, 1, args.runs)), flush=True)
        if not args.no_batch:
            print(json.dumps(bench_op(hal, 14, 64, args.runs)), flush=True)
        for n in prove:
            print(json.dumps(bench_prove(hal, n, 8, args.prove_runs)), flush=True)


if __name__ == "__main__":
    main()
