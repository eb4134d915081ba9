#!/usr/bin/env python
"""What the live-transcript seam costs: piop::prove with the FRI query phase (bnh_piop_prove_committed_open) timed through four routes,
interleaved run by run so that drift hits all of them alike:

  parent   the array entry point of another checkout of this repository (--parent DIR: its built tree, usually the parent commit)
  array    the array entry point of this tree
  replay   the _live entry point over the library's array-backed transcript (bnh_transcript_replay_*): the callbacks are C
  python   the _live entry point over a Python challenger (SHA-256 over everything written): a ctypes callback per write and draw

  python tools/bench_live_transcript.py [--shape piop|keccak] [--runs 10] [--warmup 2] [--parent DIR]

Shapes: piop -- committed multilinears of 17, 17, 19 and 20 variables, two transparents per size, a claim per pair of equal size
(tools/bench_piop.py piop --n 20); keccak -- tools/bench_piop.py's keccak claim graph at n = 18: eight committed columns of 18 variables
against three transparents.  Every route runs in a process of its own (the parent's library cannot share one with this tree's), on the
same device, one run at a time on request of the driver; a run is the wall time of the call between two synchronisations.  One JSON
line: per route median, min and max in ms, and whether the array route and the replay route stay inside the parent's max - min spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def keccak_claims(c, t=3):
    return [(i, i % t) for i in range(c)] + [(i, (i + 1) % t) for i in range(0, c, 2)] + [(i, (i + 2) % t) for i in range(0, c, 4)]


def worker(route, shape, root):
    """one route, driven over stdin/stdout: 'run' -> one timed prove, its ms on a line; 'quit'"""
    sys.path.insert(0, root)
    import hashlib
    import time

    import binius_amd
    from binius_amd import _host as H
    from binius_amd import synthetic

    if shape == "piop":
        n_varss, t_sizes = [17, 17, 19, 20], [17, 17, 19, 19, 20, 20]
        pairs = [(i, j) for i, v in enumerate(n_varss) for j, tv in enumerate(t_sizes) if v == tv]
    else:
        n_varss, t_sizes = [18] * 8, [18] * 3
        pairs = keccak_claims(8)
    total_vars = (sum(1 << v for v in n_varss) - 1).bit_length()
    arities = []
    while sum(arities) + 4 < total_vars:
        arities.append(4)
    p = H.FRIParams(total_vars - 4, 1, 4, arities, n_test_queries=232)
    sizes = sorted(set(n_varss))
    code_elems, tree_elems = H.piop_commit_elems(p)
    ml_elems = sum(1 << v for v in n_varss) + sum(1 << v for v in t_sizes)
    hal = binius_amd.Context(0, code_elems + tree_elems + 4 * code_elems + 2 * ml_elems + (1 << 16))
    alloc = hal.dev_alloc()

    def device_random(seed, n_vars):
        out = alloc.alloc(1 << n_vars)
        hal.fill(out.slice(0, 1), 1 + seed)
        hal.tensor_expand(0, synthetic.random_scalars(seed, n_vars), out)
        return out

    d_c = [(v, device_random(0x9100 + i, v)) for i, v in enumerate(n_varss)]
    d_t = [(v, device_random(0xA100 + j, v)) for j, v in enumerate(t_sizes)]
    claims = [(n_varss[i], i, j, hal.inner_product(d_c[i][1], 7, d_t[j][1])) for i, j in pairs]
    codeword, tree = alloc.alloc(code_elems), alloc.alloc(tree_elems)
    H.PiopCommit(hal, d_c, p, codeword, tree).run()
    stream = synthetic.random_scalars(0x7A0 + total_vars, len(sizes) + total_vars)
    bcs, chs = stream[: len(sizes)], stream[len(sizes):]
    top = (1 << p.index_bits()) - 1
    idx = [(0x9E3779B97F4A7C15 * (q + 1)) & top for q in range(p.n_test_queries)]
    scratch = alloc.alloc(3 * code_elems + ml_elems + (1 << 14))
    plan = H.PiopCommittedOpenPlan(hal, d_c, d_t, claims, p, codeword, tree, scratch, bcs, chs, idx)

    if route == "python":
        class Challenger(H.Transcript):
            def __init__(self):
                H.Transcript.__init__(self)
                self.h, self.draws = hashlib.sha256(), 0

            def write(self, channel, data):
                if channel == H.TR_MESSAGE:
                    self.h.update(data)

            def block(self):
                h = self.h.copy()
                h.update(self.draws.to_bytes(8, "little"))
                self.draws += 1
                return h.digest()

            def sample(self, n):
                return [int.from_bytes(self.block()[:16], "little") for _ in range(n)]

            def sample_bits(self, bits, n):
                return [int.from_bytes(self.block()[:8], "little") & ((1 << bits) - 1) for _ in range(n)]

    def once():
        tr = None
        if route == "replay":
            tr = H.ReplayTranscript(list(bcs) + list(chs), idx)
        elif route == "python":
            tr = Challenger()
        hal.sync()
        t0 = time.perf_counter()
        if tr is None:
            plan.run()
        else:
            tr.prove(plan)
        hal.sync()
        ms = (time.perf_counter() - t0) * 1e3
        if route == "replay":
            tr.close()
        return ms

    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() == "quit":
            break
        print("%.6f" % once(), flush=True)
    hal.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="piop", choices=["piop", "keccak"])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent", default=None, help="the built tree of the commit to compare with; without it the parent route is left out")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.shape, args.root)
    routes = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("array", ROOT), ("replay", ROOT), ("python", ROOT)]
    procs = {}
    try:
        for name, root in routes:
            procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "array" if name == "parent" else name, "--shape", args.shape, "--root", root],
                                           stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root)
        for name, pr in procs.items():
            line = pr.stdout.readline().strip()
            if line != "ready":
                raise RuntimeError("route %s did not start (%r)" % (name, line))
        ms = {name: [] for name, _ in routes}
        for i in range(args.warmup + args.runs):
            for name, _ in routes:  # interleaved: one run of every route, then the next
                procs[name].stdin.write("run\n")
                procs[name].stdin.flush()
                line = procs[name].stdout.readline().strip()
                if not line:
                    raise RuntimeError("route %s ended early" % name)
                if i >= args.warmup:
                    ms[name].append(float(line))
    finally:
        for pr in procs.values():
            try:
                pr.stdin.write("quit\n")
                pr.stdin.flush()
            except (BrokenPipeError, OSError):
                pass
        for pr in procs.values():
            try:
                pr.wait(timeout=60)
            except subprocess.TimeoutExpired:
                pr.kill()
    rec = {"bench": "live_transcript", "shape": args.shape, "runs": args.runs,
           "routes": {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for name, v in ms.items()}}
    if "parent" in ms:
        lo, hi = min(ms["parent"]), max(ms["parent"])
        rec["parent_spread_ms"] = round(hi - lo, 4)
        for name in ("array", "replay"):
            rec["%s_median_minus_parent_median_ms" % name] = round(statistics.median(ms[name]) - statistics.median(ms["parent"]), 4)
            rec["%s_inside_parent_spread" % name] = bool(abs(statistics.median(ms[name]) - statistics.median(ms["parent"])) <= hi - lo)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
