"""The caller-owned stream contract of bn_ctx_set_stream.

A context put on a stream the caller also enqueues on must (A) run in strict call order, (B) keep its launches ordered with
the caller's own work on that stream, (C) defer again under BN_LAZY_ON_SHARED_STREAM=1 with bn_sync / bn_ctx_get_stream as
the flush points, (D) flush what is pending when the stream is switched, in either direction and in the middle of a prover,
and come back from a round trip with the behaviour it was created with.

The stream, the caller's buffers and the caller's work come from tests/caller_stream.py: ctypes on the HIP runtime, calls the
library cannot see through.  Every expected value comes from the oracle, computed on the host; nothing is compared with the
device's own output.  The stream is created in the HIP runtime image the library itself is bound to (caller_stream.runtime),
so it is the library's own runtime's stream however many images the process maps.  A stream that torch made is not tested:
where torch maps a runtime image of its own beside the library's, its handle means nothing to the library.
"""
import os
import time

import numpy as np
import pytest

import caller_stream as CS

pytestmark = pytest.mark.gpu

DET = ("two_round", "ht_started", "ht_rounds", "shadow_created", "shadow_rounds")  # counters that do not depend on host timing
ALL_PATHS = ("hits", "hosted") + DET
CANARY = 0xC5
THREADS = min(8, os.cpu_count() or 1)


@pytest.fixture(autouse=True, scope="module")
def _runtime():
    try:
        rt = CS.runtime()
    except CS.AmbiguousRuntime as e:
        pytest.skip(str(e))
    print("caller streams come from %s (mapped: %s)" % (rt.path, ", ".join(CS.mapped_hip_images())))


@pytest.fixture()
def cs():
    s = CS.CallerStream()
    yield s
    s.close()
    assert s.destroyed == 1


@pytest.fixture(scope="module")
def delay(_runtime):
    owner = CS.CallerStream()
    yield CS.Delay(owner)
    owner.close()


@pytest.fixture()
def opt_in(monkeypatch):
    monkeypatch.delenv("BN_NO_LAZY_FOLD", raising=False)
    monkeypatch.setenv("BN_LAZY_ON_SHARED_STREAM", "1")  # read by bn_ctx_set_stream


@pytest.fixture()
def strict(monkeypatch):
    monkeypatch.delenv("BN_LAZY_ON_SHARED_STREAM", raising=False)


def context(arena_log2, stream=None):
    import binius_amd

    assert arena_log2 <= 20
    hal = binius_amd.Context(0, 1 << arena_log2)
    if stream is not None:
        hal.set_stream(stream.handle)
    return hal


def upload(hal, alloc, arr):
    d = alloc.alloc(arr.shape[0])
    hal.copy_h2d(arr, d)
    return d


def folded(oracle, x, z):
    f = x[: len(x) // 2].copy()
    assert oracle.extrapolate_line(f, x[len(x) // 2 :].copy(), z) == 0
    return f


def delta(c1, c0, keys):
    return {k: c1[k] - c0[k] for k in keys}


# ---------------------------------------------------------------- the chains and their oracle values (computed once, never changed)
_REFS = {}


def chain_ref(oracle, n_vars, seed=0xC5710000):
    """The bivariate sumcheck chain of tests/test_gpu_sumcheck.py::_rounds_with_oracle: inputs, challenges, every round's
    (y_1, y_inf) and the final arrays, from the oracle."""
    key = ("biv", n_vars, seed)
    if key not in _REFS:
        mls = [oracle.random_b128(seed + 16 * n_vars + j, 1 << n_vars) for j in range(2)]
        zs = oracle.random_scalars(seed ^ 0x55 ^ n_vars, n_vars)
        cur, want = [x.copy() for x in mls], []
        for r in range(n_vars):
            rc, w = oracle.round_evals(cur, n_vars - r, [(0, 1)], 1, threads=THREADS)
            assert rc == 0
            want.append(w)
            cur = [folded(oracle, x, zs[r]) for x in cur]
        _REFS[key] = {"n_vars": n_vars, "mls": mls, "zs": zs, "want": want, "final": cur}
    return _REFS[key]


class Chain:
    """evaluate -> fold -> evaluate ... one round per step(); the context that evaluates and the one that folds may differ
    (two contexts on one stream) and may change their stream between the steps."""

    def __init__(self, hal, ref):
        self.ref, self.r, self.exprs = ref, 0, {}
        alloc = hal.dev_alloc()
        self.d = [upload(hal, alloc, x) for x in ref["mls"]]

    def expr(self, hal):
        from binius_amd.sumcheck import bivariate_product_expr

        if id(hal) not in self.exprs:
            self.exprs[id(hal)] = bivariate_product_expr(hal, 0, 1)
        return self.exprs[id(hal)]

    def step(self, hal, hal_fold=None):
        from binius_amd.sumcheck import calculate_round_evals

        r, ref = self.r, self.ref
        got = calculate_round_evals(hal, ref["n_vars"] - r, [1], self.d, [self.expr(hal)])
        assert got == ref["want"][r], "round %d" % r
        halves = [x.split_half() for x in self.d]
        (hal_fold or hal).extrapolate_line_batch([lo for lo, _ in halves], [hi for _, hi in halves], ref["zs"][r])
        self.d = [lo for lo, _ in halves]
        self.r += 1

    def run(self, hal, upto=None):
        while self.r < (self.ref["n_vars"] if upto is None else upto):
            self.step(hal)

    def finish(self, hal):
        assert self.r == self.ref["n_vars"]
        for dd, x in zip(self.d, self.ref["final"]):
            assert np.array_equal(hal.copy_d2h(dd), x)


def mle_ref(oracle, n_vars, seed=0xC5720000):
    """The literal MLE-check sequence (a * b * eq, fold of (a, b), table fold) down to arrays of 16 elements."""
    key = ("mle", n_vars, seed)
    if key not in _REFS:
        a, b = (oracle.random_b128(seed + j, 1 << n_vars) for j in range(2))
        eq = oracle.arr(1 << (n_vars - 1))
        eq[0] = (1, 0)
        oracle.tensor_expand(eq, 0, oracle.random_scalars(seed ^ 0xE9, n_vars - 1))
        zs = oracle.random_scalars(seed ^ 0x56, n_vars)
        ref = {"n_vars": n_vars, "a": a.copy(), "b": b.copy(), "eq": eq.copy(), "zs": zs, "want": [], "rounds": n_vars - 4}
        for r in range(ref["rounds"]):
            rc, w = oracle.round_evals_eq([a.copy(), b.copy()], n_vars - r, eq.copy(), [(0, 1)], 1)
            assert rc == 0
            ref["want"].append(w)
            a, b = folded(oracle, a, zs[r]), folded(oracle, b, zs[r])
            h = len(eq) // 2
            eq = eq[:h] ^ eq[h:]
        ref["final"] = (a, b, eq)
        _REFS[key] = ref
    return _REFS[key]


def run_mle_chain(hal, ref):
    from binius_amd.sumcheck import bivariate_product_eq_expr, calculate_round_evals

    alloc = hal.dev_alloc()
    da, db, deq = (upload(hal, alloc, ref[k]) for k in ("a", "b", "eq"))
    e3 = bivariate_product_eq_expr(hal, 0, 1, 2)
    cur, eq_len = 1 << ref["n_vars"], 1 << (ref["n_vars"] - 1)
    for r in range(ref["rounds"]):
        got = calculate_round_evals(hal, ref["n_vars"] - r, [1], [da.slice(0, cur), db.slice(0, cur)], [e3], eq_ind=deq.slice(0, eq_len))
        assert got == ref["want"][r], "MLE-check round %d" % r
        half, h = cur // 2, eq_len // 2
        hal.extrapolate_line_batch([da.slice(0, half), db.slice(0, half)], [da.slice(half, cur), db.slice(half, cur)], ref["zs"][r])

        def k(ke, log_chunks, bufs, h=h):
            ke.add_assign(int(np.log2(h)) - log_chunks, bufs[1].to_ref(), bufs[0])

        hal.map_kernels(k, [("chunked_mut", deq.slice(0, h), 0), ("chunked", deq.slice(h, eq_len), 0)])
        cur, eq_len = half, h
    for d, x in zip((da, db, deq), ref["final"]):
        assert np.array_equal(hal.copy_d2h(d.slice(0, len(x))), x)


_OWN = {}


def own_stream_counters(oracle, kind, n_vars):
    """What a fresh context on its private stream counts for the same chain (which is checked against the oracle there too),
    and, for the bivariate chain, the counters after every round.  (Cached per setting of the BN_* variables: a context reads
    most of them when it is created.)"""
    key = (kind, n_vars, tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("BN_"))))
    if key not in _OWN:
        hal = context(20 if n_vars > 14 else 16)
        try:
            c0, snaps = hal.arm_counters(), []
            if kind == "biv":
                ch = Chain(hal, chain_ref(oracle, n_vars))
                while ch.r < n_vars:
                    ch.step(hal)
                    snaps.append(hal.arm_counters())
                ch.finish(hal)
            else:
                run_mle_chain(hal, mle_ref(oracle, n_vars))
            _OWN[key] = (delta(hal.arm_counters(), c0, ALL_PATHS + ("cancels", "expired")), snaps)
        finally:
            hal.close()
    return _OWN[key]


# ---------------------------------------------------------------- A. strict call order is the default on a caller stream
@pytest.mark.parametrize("probe", ["fold", "copy", "copy_then_fold"])
def test_a_deferrable_calls_run_at_once(cs, oracle, strict, probe):
    """Neither bn_sync nor a library read follows the call: the caller's own asynchronous read on the stream, enqueued right
    after it, must see its effect.  (With the deferral left on, the fold / copy would still be waiting for the next call.)"""
    n = 1 << 10
    x, y = oracle.random_b128(0xC5A10000, n), oracle.random_b128(0xC5A10001, n)
    z = oracle.random_scalars(0xC5A1, 1)[0]
    hal = context(14, cs)
    try:
        alloc = hal.dev_alloc()
        dx, dy = upload(hal, alloc, x), upload(hal, alloc, y)
        (lo, hi), half = dx.split_half(), n // 2
        if probe == "fold":
            hal.extrapolate_line_batch([lo], [hi], z)
            got, want = cs.read_async(lo.ptr, half), folded(oracle, x, z)
        elif probe == "copy":
            hal.copy_d2d(dx, dy)
            got, want = cs.read_async(dy.ptr, n), x
        else:  # the first fold of a prover: evals_0 copied into a fresh buffer that the fold then writes (the absorbed copy)
            fresh = dy.slice(0, half)
            hal.copy_d2d(lo, fresh)
            hal.extrapolate_line_batch([fresh], [hi], z)
            got, want = cs.read_async(fresh.ptr, half), folded(oracle, x, z)
        cs.synchronize()
        assert np.array_equal(got, want)
        if probe != "fold":
            assert np.array_equal(hal.copy_d2h(dx), x)  # (the source of the copy is untouched)
    finally:
        hal.close()


def test_a_whole_chain_in_strict_order(cs, oracle, strict):
    """n_vars = 13 crosses the sizes of the two-round kernels, the armed rounds and the host tail: none of them may run."""
    hal = context(15, cs)
    try:
        c0 = hal.arm_counters()
        ch = Chain(hal, chain_ref(oracle, 13))
        ch.run(hal)
        ch.finish(hal)
        assert delta(hal.arm_counters(), c0, ALL_PATHS) == {k: 0 for k in ALL_PATHS}
    finally:
        hal.close()


# ---------------------------------------------------------------- B. the library's launches are ordered with the caller's work
def _ordering_case(name, oracle, hal, alloc):
    """inputs: (DevSlice, array the caller writes); outputs: (DevSlice, oracle value); call: the one library op."""
    import binius_amd

    rnd = lambda k, n: oracle.random_b128(0xC5B00000 + 256 * sum(map(ord, name)) + k, n)  # noqa: E731
    z = oracle.random_scalars(0xC5B0 + len(name), 1)[0]
    if name == "extrapolate_line_batch":
        x, d = rnd(0, 1 << 10), alloc.alloc(1 << 10)
        lo, hi = d.split_half()
        return [(d, x)], [(lo, folded(oracle, x, z))], lambda: hal.extrapolate_line_batch([lo], [hi], z)
    if name == "fill":  # (no input: what the caller writes is what the fill must come after)
        x, d = rnd(0, 1 << 10), alloc.alloc(1 << 10)
        want = oracle.arr(1 << 10)
        want[:] = (z & ((1 << 64) - 1), z >> 64)
        return [(d, x)], [(d, want)], lambda: hal.fill(d, z)
    if name == "copy_d2d":
        x, src, dst = rnd(0, 1 << 10), alloc.alloc(1 << 10), alloc.alloc(1 << 10)
        return [(src, x)], [(dst, x)], lambda: hal.copy_d2d(src, dst)
    if name == "tensor_expand":
        k = 12
        x, d, coords = oracle.arr(1 << k), alloc.alloc(1 << k), oracle.random_scalars(0xC5B4, k)
        x[0] = rnd(0, 1)[0]
        want = x.copy()
        assert oracle.tensor_expand(want, 0, coords) == 0
        return [(d, x)], [(d, want)], lambda: hal.tensor_expand(0, coords, d)
    if name == "fold_right":
        level, log_q, log_out = 5, 3, 10
        mat, vec = rnd(0, (1 << (log_out + log_q)) >> (7 - level)), rnd(1, 1 << log_q)
        dm, dv, do = alloc.alloc(len(mat)), alloc.alloc(len(vec)), alloc.alloc(1 << log_out)
        want = oracle.arr(1 << log_out)
        assert oracle.fold_right(mat, level, vec, want) == 0
        return [(dm, mat), (dv, vec)], [(do, want)], lambda: hal.fold_right(dm, level, dv, do)
    if name == "compute_composite":
        a, b = rnd(0, 1 << 10), rnd(1, 1 << 10)
        da, db, do = (alloc.alloc(1 << 10) for _ in range(3))
        expr = hal.compile_expr([("var", 0), ("var", 1), ("mul", 0, 1)])
        return [(da, a), (db, b)], [(do, oracle.mul_vec(a, b))], lambda: hal.compute_composite([da, db], do, expr)
    if name == "pairwise_product_reduce":
        log_n = 12
        x, dx = rnd(0, 1 << log_n), alloc.alloc(1 << log_n)
        outs = [alloc.alloc((1 << log_n) >> (r + 1)) for r in range(log_n)]
        want = [oracle.arr(o.len) for o in outs]
        assert oracle.pairwise_product_reduce(x, want) == 0
        return [(dx, x)], list(zip(outs, want)), lambda: hal.pairwise_product_reduce(dx, outs)
    if name == "ntt_forward":
        log_y = 12
        x, d, s = rnd(0, 1 << log_y), alloc.alloc(1 << log_y), binius_amd.ntt_s_evals(5, log_y)
        want = x.copy()
        assert oracle.ntt_forward(want, 7, 5, s, log_y, 0, log_y, 0) == 0
        return [(d, x)], [(d, want)], lambda: hal.ntt_forward(d.ptr, 7, 5, s, log_y, 0, log_y, 0)
    assert name == "merkle_build"
    leaves, batch = 1 << 10, 2
    x, d, nodes = rnd(0, leaves * batch), alloc.alloc(leaves * batch), alloc.alloc(2 * (2 * leaves - 1))
    rc, want = oracle.merkle_build(x, batch)
    assert rc == 0
    return [(d, x)], [(nodes, np.ascontiguousarray(want).view(np.uint64).reshape(-1, 2))], lambda: hal.merkle_build(d, batch, nodes)


@pytest.mark.parametrize("name", ["extrapolate_line_batch", "fill", "copy_d2d", "tensor_expand", "fold_right", "compute_composite",
                                  "pairwise_product_reduce", "ntt_forward", "merkle_build"])
def test_b_launches_are_ordered_with_the_callers_work(cs, delay, oracle, strict, name):
    """On the stream: [delay] [the caller writes the inputs over a canary] [ONE library op] [the caller reads the outputs], and one
    synchronisation by the caller at the end.  The op is issued while the delay still runs, so a launch on any other stream
    reads the canary.  The delay is measured with events, the host time from the first enqueue to the start of the final
    synchronisation with the clock: delay >= 5 x host time, or the test FAILS ("delay too short") -- a call that waited for
    the stream on the host would fail it too."""
    hal = context(16, cs)
    try:
        inputs, outputs, call = _ordering_case(name, oracle, hal, hal.dev_alloc())
        staged = [cs.staged(x) for _, x in inputs]
        landing = [cs.malloc(o.len) for o, _ in outputs]
        call()  # once beforehand, on whatever the buffers hold: code objects, scratch and tables are in place for the measured call
        hal.sync()
        for sl in [d for d, _ in inputs] + [o for o, _ in outputs]:
            cs.memset(sl.ptr, CANARY, sl.len)
        for b in landing:
            cs.memset(b.ptr, CANARY, b.len)
        cs.synchronize()
        # ---- the measured sequence: nothing below waits for the device before the final synchronisation
        t0 = delay.enqueue(cs)
        for (d, _), st in zip(inputs, staged):
            cs.copy_d2d(d.ptr, st.ptr, d.len)
        call()
        for (o, _), b in zip(outputs, landing):
            cs.copy_d2d(b.ptr, o.ptr, o.len)
        host_ms = (time.perf_counter() - t0) * 1e3
        cs.synchronize()
        CS.require_delay_covers(delay.ms(), host_ms, name)
        got = [cs.read_async(b.ptr, b.len) for b in landing]
        cs.synchronize()
        for g, (_, want) in zip(got, outputs):
            assert np.array_equal(g, want), "%s ran out of order with the caller's work on its stream" % name
    finally:
        hal.close()


# ---------------------------------------------------------------- C. the opt-in: BN_LAZY_ON_SHARED_STREAM=1
@pytest.mark.parametrize("kind,n_vars", [("biv", 13), ("biv", 18), ("mle", 10)])
def test_c_opt_in_turns_the_deferral_back_on(cs, oracle, opt_in, kind, n_vars):
    """biv 18: the fused fold + evaluate is on the matrix-core kernel from 2^17 points.  mle 10: tables of 2^9 entries, the
    smallest size at which tests/test_gpu_mlecheck_shadow.py sees shadow rounds."""
    own, _ = own_stream_counters(oracle, kind, n_vars)
    hal = context(20 if n_vars > 14 else 16, cs)
    try:
        c0 = hal.arm_counters()
        if kind == "biv":
            ch = Chain(hal, chain_ref(oracle, n_vars))
            ch.run(hal)
            ch.finish(hal)
        else:
            run_mle_chain(hal, mle_ref(oracle, n_vars))
        got = delta(hal.arm_counters(), c0, ALL_PATHS)
        print("opt-in %s n_vars=%d: shared stream %r, own stream %r" % (kind, n_vars, got, own))
        assert {k: got[k] for k in DET} == {k: own[k] for k in DET}  # (hits and hosted depend on the host's timing: not compared)
        assert sum(own[k] for k in DET) > 0, "the chain exercised none of the deferred paths"
    finally:
        hal.close()


@pytest.mark.parametrize("flush", ["sync", "get_stream"])
def test_c_sync_and_get_stream_flush_before_the_caller_reads(cs, delay, oracle, opt_in, flush):
    """[delay] [the caller writes X over a canary] fold (deferred under the opt-in), then the flush point, then the caller's read.
    The fold is issued while the delay still runs (checked as in B), so a flush that launched it anywhere but on S, behind
    the caller's write, folds the canary."""
    n = 1 << 10
    x, z = oracle.random_b128(0xC5C20000, n), oracle.random_scalars(0xC5C2, 1)[0]
    hal = context(14, cs)
    try:
        d = hal.dev_alloc().alloc(n)
        lo, hi = d.split_half()
        st = cs.staged(x)
        cs.memset(d.ptr, CANARY, n)
        cs.synchronize()
        t0 = delay.enqueue(cs)
        cs.copy_d2d(d.ptr, st.ptr, n)
        hal.extrapolate_line_batch([lo], [hi], z)
        host_ms = (time.perf_counter() - t0) * 1e3  # (up to the flush point: bn_sync waits for the stream)
        if flush == "sync":
            hal.sync()
        else:
            assert hal.get_stream() == cs.handle
        got = cs.read_async(lo.ptr, n // 2)
        cs.synchronize()
        CS.require_delay_covers(delay.ms(), host_ms, "deferred fold, then " + flush)
        assert np.array_equal(got, folded(oracle, x, z))
    finally:
        hal.close()


@pytest.mark.parametrize("seed", [0, 3, 5, 8])
def test_c_random_call_sequences_lazy_on_a_shared_stream(cs, oracle, monkeypatch, seed):
    """The differential fuzz of tests/test_gpu_lazy_vs_eager.py: deferral on a caller-owned stream against eager execution."""
    import binius_amd
    from test_gpu_lazy_vs_eager import random_call_sequence

    monkeypatch.delenv("BN_LAZY_ON_SHARED_STREAM", raising=False)
    monkeypatch.setenv("BN_NO_LAZY_FOLD", "1")
    eager = binius_amd.Context(0, 1 << 16)
    monkeypatch.delenv("BN_NO_LAZY_FOLD")
    monkeypatch.setenv("BN_LAZY_ON_SHARED_STREAM", "1")
    lazy = context(16, cs)
    try:
        random_call_sequence(oracle, eager, lazy, seed, False)
    finally:
        eager.close()
        lazy.close()


# ---------------------------------------------------------------- D. switching
@pytest.mark.parametrize("pending", ["fold", "copy", "copy_then_fold"])
def test_d_own_to_caller_flushes_what_is_pending(cs, oracle, strict, pending):
    """Deferred on the private stream at the moment of set_stream(S): a fold; a copy no fold has absorbed; a copy absorbed into
    a fold.  (A fold behind an unabsorbed copy launches the copy, so the two are never deferred together.)  When set_stream
    returns nothing is pending: the caller's own read on S sees the result, and the library's read afterwards shows that it was
    applied exactly once."""
    n = 1 << 10
    x, y = oracle.random_b128(0xC5D10000, n), oracle.random_b128(0xC5D10001, n)
    z = oracle.random_scalars(0xC5D1, 1)[0]
    hal = context(14)
    try:
        alloc = hal.dev_alloc()
        dx, dy = upload(hal, alloc, x), upload(hal, alloc, y)
        (lo, hi), half = dx.split_half(), n // 2
        if pending == "fold":
            hal.extrapolate_line_batch([lo], [hi], z)
            target, want = lo, folded(oracle, x, z)
        elif pending == "copy":
            hal.copy_d2d(dx, dy)
            target, want = dy, x
        else:
            target, want = dy.slice(0, half), folded(oracle, x, z)
            hal.copy_d2d(lo, target)
            hal.extrapolate_line_batch([target], [hi], z)
        hal.set_stream(cs.handle)
        got = cs.read_async(target.ptr, target.len)
        cs.synchronize()
        assert np.array_equal(got, want), "set_stream left deferred work behind"
        assert np.array_equal(hal.copy_d2h(target), want), "applied more than once"
        if pending != "fold":
            assert np.array_equal(hal.copy_d2h(dx), x)
    finally:
        hal.close()


def _placement(oracle, what):
    """The round of the n_vars = 13 chain after which, by the counters of a run on a private stream, an armed kernel is waiting
    (it is used, expires or is cancelled in the next round) / the sums a two-round launch computed ahead are live / the host
    tail has taken the arrays over."""
    _, snaps = own_stream_counters(oracle, "biv", 13)
    zero = {k: 0 for k in snaps[0]}
    for r in range(len(snaps) - 1):
        prev, cur, nxt = (snaps[r - 1] if r else zero), snaps[r], snaps[r + 1]
        if what == "armed" and sum(nxt[k] - cur[k] for k in ("hits", "cancels", "expired")) > 0:
            return r
        if what == "two_round" and cur["two_round"] > prev["two_round"]:
            return r
        if what == "host_tail" and cur["ht_started"] > prev["ht_started"]:
            return r
    pytest.fail("the chain on a private stream never had %s state: %r" % (what, snaps))


@pytest.mark.parametrize("what", ["armed", "two_round", "host_tail"])
@pytest.mark.parametrize("direction", ["to_caller", "to_own"])
def test_d_switch_in_the_middle_of_a_prover(cs, oracle, monkeypatch, what, direction):
    """set_stream in the middle of the chain, at the rounds where the most state is live; every round and the final arrays
    still equal the oracle.  to_own starts on the caller's stream under the opt-in (the same deferred paths) and returns
    to the private stream with set_stream(None).  At n_vars = 13 the host tail takes the arrays over as soon as they are
    down to 2^12 elements and nothing is ever armed, so the `armed` placement runs on contexts created with BN_HOST_TAIL=0:
    there the small rounds are the armed two-round launches."""
    if what == "armed":
        monkeypatch.setenv("BN_HOST_TAIL", "0")
    r_switch = _placement(oracle, what)
    print("switch %s with %s state live: after round %d" % (direction, what, r_switch))
    monkeypatch.delenv("BN_LAZY_ON_SHARED_STREAM", raising=False)
    if direction == "to_own":
        monkeypatch.setenv("BN_LAZY_ON_SHARED_STREAM", "1")
    hal = context(15, cs if direction == "to_own" else None)
    try:
        ch = Chain(hal, chain_ref(oracle, 13))
        ch.run(hal, upto=r_switch + 1)
        hal.set_stream(cs.handle if direction == "to_caller" else None)
        if direction == "to_caller":  # nothing is pending behind the switch: the caller sees the folded arrays on its stream
            m = min(4, ch.d[0].len)
            got = [cs.read_async(dd.ptr, m) for dd in ch.d]
            cs.synchronize()
            cur = [x.copy() for x in ch.ref["mls"]]
            for r in range(ch.r):
                cur = [folded(oracle, x, ch.ref["zs"][r]) for x in cur]
            for g, x in zip(got, cur):
                assert np.array_equal(g, x[:m])
        ch.run(hal)
        ch.finish(hal)
    finally:
        hal.close()


def test_d_round_trip_restores_the_private_streams_behaviour(cs, oracle, strict):
    own, _ = own_stream_counters(oracle, "biv", 13)
    hal = context(15)
    try:
        hal.set_stream(cs.handle)
        hal.set_stream(None)
        c0 = hal.arm_counters()
        ch = Chain(hal, chain_ref(oracle, 13))
        ch.run(hal)
        ch.finish(hal)
        got = delta(hal.arm_counters(), c0, DET)
        assert got == {k: own[k] for k in DET}
    finally:
        hal.close()


def _tail_launches(hal, oracle):
    """Launches of profile class `tail` (the resident kernel of BN_TAIL_MAX_LOG2) during the n_vars = 13 chain."""
    hal.prof_begin()
    ch = Chain(hal, chain_ref(oracle, 13))
    ch.run(hal)
    prof = hal.prof_end()
    ch.finish(hal)
    return prof["tail"][1]


def test_d_round_trip_keeps_the_resident_tail(cs, oracle, strict, monkeypatch):
    """A context created under BN_TAIL_MAX_LOG2=12 runs its small rounds in the resident tail kernel; on a caller's stream
    without the opt-in it does not (nothing is deferred); back on its private stream it does again."""
    import binius_amd

    monkeypatch.setenv("BN_TAIL_MAX_LOG2", "12")
    fresh, hal = binius_amd.Context(0, 1 << 15), binius_amd.Context(0, 1 << 15)
    monkeypatch.delenv("BN_TAIL_MAX_LOG2")
    try:
        want = _tail_launches(fresh, oracle)
        assert want >= 1, "the resident tail did not run on a fresh context"
        hal.set_stream(cs.handle)
        assert _tail_launches(hal, oracle) == 0
        hal.set_stream(None)
        assert _tail_launches(hal, oracle) == want, "the round trip lost the resident tail"
        assert hal.arm_counters()["two_round"] == 0  # (the two-round kernels stay off while the tail is configured)
    finally:
        fresh.close()
        hal.close()


def test_d_handle_zero_selects_the_private_stream(cs, oracle, strict):
    """set_stream(None) and handle 0 are the same call: the null stream is never adopted."""
    hal = context(14, cs)
    try:
        hal.set_stream(0)
        private = hal.get_stream()
        assert private not in (0, cs.handle)
        hal.set_stream(None)
        assert hal.get_stream() == private  # (already private: nothing changes)
    finally:
        hal.close()


def test_d_close_leaves_the_callers_stream_usable(cs, oracle, strict):
    n = 1 << 10
    x, z = oracle.random_b128(0xC5D40000, n), oracle.random_scalars(0xC5D4, 1)[0]
    hal = context(14, cs)
    hal.set_stream(cs.handle)  # twice: harmless
    assert hal.get_stream() == cs.handle
    d = upload(hal, hal.dev_alloc(), x)
    lo, hi = d.split_half()
    hal.extrapolate_line_batch([lo], [hi], z)
    got = cs.read_async(lo.ptr, n // 2)
    cs.synchronize()
    assert np.array_equal(got, folded(oracle, x, z))
    hal.close()
    # the stream outlives the context: a copy of the caller's own on it succeeds (the fixture destroys it, once)
    src, dst = cs.staged(x), cs.malloc(n)
    cs.copy_d2d(dst.ptr, src.ptr, n)
    back = cs.read_async(dst.ptr, n)
    cs.synchronize()
    assert np.array_equal(back, x)


def test_d_two_contexts_share_one_stream(cs, oracle, strict):
    """The n_vars = 13 chain split between two contexts on the same caller's stream: they take turns, one evaluates a round,
    the other folds (on the arrays in the first one's arena); the stream alone orders them."""
    a, b = context(15, cs), context(12, cs)
    try:
        ch = Chain(a, chain_ref(oracle, 13))
        while ch.r < 13:
            ev, fo = (a, b) if ch.r % 2 == 0 else (b, a)
            ch.step(ev, fo)
        ch.finish(b)
    finally:
        a.close()
        b.close()
