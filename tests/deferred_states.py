"""The four states a bn_extrapolate_line_batch call can leave a context in, reached on purpose (a helper, not a test module).

  S1  the fold is pending in the single-claim state (ctx->pend)
  S2  the fold is parked as a claim-group fold (ctx->grp.folds)
  S3  a hosted session holds the prover's arrays on the host, nothing pending (h_levels == 0)
  S4  the host has folded its copies; the device is one write-back launch behind (h_levels >= 1)
  S4x2  S4 one round later: execute and a second, in-place fold on the host (h_levels == 2)

One small prover on the device and a host model of it.  The model is NumPy memory folded with oracle.extrapolate_line and evaluated
with oracle.round_evals: never the device's own output, never an eager context's.  Every buffer of a case lies in ONE region of the
arena, mirrored by ONE array (`mem`): a case applies every foreign call to both, and at the end the region is compared byte for
byte.

The prover of S2 .. S4 has m = 3 multilinears under k = 2 product claims, (0, 1) and (1, 2): k >= 2 sends calculate_round_evals down
the group path.  Its fold is the reference's PreFold step: copy_d2d of evals_0 into fresh buffers, then extrapolate_line_batch with
the upper halves of the inputs as x1.

S1 is the single-claim shape: TWO multilinears under ONE claim.  A batch of one array is not that shape -- group_fold_applies() sends
every batch whose count is not 2 to the claim groups, so a lone array's fold parks in ctx->grp.folds, which is S2 -- and only the
lone two-array batch is left in ctx->pend.  No execute() precedes that fold: at this size the single-claim machinery's own host tail
would take the instance over, a fifth state that is not the subject here.

Sizes: 2^8 elements per multilinear.  Every state is reached at that size: the fold of S2 is deferred at any size, and a hosted
session starts once an array is at most 2^BN_GROUP_HT_MAX_LOG2 = 2^8 elements (3 x 2^8 elements and (2 + 2) x 2^8 products are far
inside the hand-over's other limits).

Layout of the region (elements; `in` the PreFold inputs, `f` the fresh buffers the first fold writes):

    pre_in | in_0 .. in_{m-1} | post_in | pre_f | f_0 .. f_{m-1} | post_f | work

After a first fold the live arrays are f_j[:2^7] (x0), their dead upper halves in_j[2^7:] (x1), their PreFold sources in_j[:2^7]
(src0).  In S3 nothing is folded: the live arrays are in_j, x1 names their upper halves, and there is no src0.  The spare buffers
share a boundary with the first / last array of a row, so a range can end exactly where an array begins.

Why S4x2.  After ONE hosted fold the memory the owed write-back covers (f_j[:2^7]) is exactly the memory of the current arrays, and
every range-scoped entry point asks as a writer: the "write into a current array" clause of session_touches() answers for the
"pending write-back" clause, whichever of the two is broken.  After a second, in-place fold the current arrays are f_j[:2^6] and the
write-back still covers f_j[:2^7]: x1 = f_j[2^6:2^7] is memory only the pending write-back clause knows about.  There the row of live
arrays ends where x1 begins (ISOLATED says which boundaries a spare buffer isolates)."""
import os

import numpy as np
import pytest

LOG_N = 8
PAD = 1024
WORK = 1 << 13
STATES = ("S1", "S2", "S3", "S4", "S4x2")
HOSTED = ("S3", "S4", "S4x2")
HT_LOG2 = {"S1": None, "S2": 0, "S3": 8, "S4": 8, "S4x2": 8}  # BN_GROUP_HT_MAX_LOG2 of the context a state is reached on (None: default settings)


def region_elems(m, log_n):
    """elements of a case's region: four spare buffers, m inputs, m fresh buffers, the work area"""
    return 4 * PAD + m * (1 << log_n) + m * (1 << (log_n - 1)) + max(WORK, 4 << log_n)


ARENA = region_elems(3, LOG_N) + 4096
# state -> row -> (a spare buffer ends where the row's first array begins, a spare buffer begins where its last array ends)
ISOLATED = {s: {"live": (True, True), "x1": (False, True), "src0": (True, False)} for s in ("S1", "S2", "S4")}
ISOLATED["S3"] = {"live": (True, True), "x1": (False, True)}
ISOLATED["S4x2"] = {"live": (True, False), "x1": (False, True)}
NO_HOST_TAIL = "hosted sessions need the host tail: this host has no PCLMULQDQ or BN_HOST_TAIL=0 is set (arm_counters()['ht_max'] == 0)"


class env:
    """environment switches that bn_ctx_create reads, for the contexts created inside the block (as in test_gpu_group.py)"""

    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_context(state, arena=ARENA):
    """a context with the settings `state` is reached under"""
    import binius_amd

    with env(BN_GROUP_HT_MAX_LOG2=HT_LOG2[state]):
        return binius_amd.Context(0, arena)


class Contexts:
    """one context per BN_GROUP_HT_MAX_LOG2 value, created on first use (a module-scoped fixture closes them)"""

    def __init__(self):
        self.by_ht = {}

    def get(self, state):
        ht = HT_LOG2[state]
        if ht not in self.by_ht:
            self.by_ht[ht] = make_context(state)
        return self.by_ht[ht]

    def close(self):
        for h in self.by_ht.values():
            h.close()
        self.by_ht = {}


class Buf:
    """[off, off + n) of a case's region: the device slice and the model's view of the same elements"""

    def __init__(self, st, off, n, name=""):
        assert 0 <= off and off + n <= st.total, "a range outside the case's region"
        self.st, self.off, self.n, self.name = st, off, n, name

    @property
    def dev(self):
        return self.st.region.slice(self.off, self.off + self.n)

    @property
    def host(self):
        return self.st.mem[self.off : self.off + self.n]

    @property
    def end(self):
        return self.off + self.n

    def sub(self, a, b):
        assert 0 <= a <= b <= self.n
        return Buf(self.st, self.off + a, b - a, self.name)

    def __repr__(self):
        return "Buf(%s %d+%d)" % (self.name, self.off, self.n)


def moved(before, after):
    return {k: after[k] - before[k] for k in before if after[k] != before[k]}


class Prover:
    """The prover and its model.  hal = None: the model alone (the preview a case stages its own inputs from)."""

    def __init__(self, hal, oracle, state, seed, mem=None, log_n=LOG_N):
        assert state in STATES
        self.hal, self.oracle, self.state, self.log_n = hal, oracle, state, log_n
        self.m, self.comps = (2, [(0, 1)]) if state == "S1" else (3, [(0, 1), (1, 2)])
        m = self.m
        o = 0
        names = [("pre_in", PAD)] + [("in%d" % j, 1 << log_n) for j in range(m)] + [("post_in", PAD), ("pre_f", PAD)] + \
            [("f%d" % j, 1 << (log_n - 1)) for j in range(m)] + [("post_f", PAD), ("work", max(WORK, 4 << log_n))]
        self.total = sum(n for _, n in names)
        assert self.total == region_elems(m, log_n)
        self.named = {}
        for name, n in names:
            self.named[name] = Buf(self, o, n, name)
            o += n
        self.inputs = [self.named["in%d" % j] for j in range(m)]
        self.fresh = [self.named["f%d" % j] for j in range(m)]
        self.pre_in, self.post_in, self.pre_f, self.post_f, self.work = (self.named[k] for k in ("pre_in", "post_in", "pre_f", "post_f", "work"))
        self.mem = oracle.random_b128(0xDEF00000 + seed, self.total) if mem is None else mem
        stream = oracle.random_scalars(0xDEF1 + seed, 8)
        self.bc, self.challenges, self.zs = stream[0], stream[1:], iter(stream[1:])  # (challenges[i]: the z of the prover's fold i)
        self.coeffs, pw = [], 1
        for _ in self.comps:
            self.coeffs.append(pw)
            pw = oracle.mul(pw, self.bc)
        self.n_rem, self.pre_fold = log_n, True
        self.last_x1 = self.last_src0 = None  # of the last fold
        self.work_top = 0
        self.region = None
        self.reached = None  # the counter deltas that proved the state

    # ---- the prover's arrays as they are now
    @property
    def live(self):
        """the current arrays (a deferred fold's x0)"""
        return [(self.inputs[j] if self.pre_fold else self.fresh[j]).sub(0, 1 << self.n_rem) for j in range(self.m)]

    @property
    def x1(self):
        """the upper halves the last fold read (S3: of the arrays the next fold will read)"""
        return [x.sub(x.n // 2, x.n) for x in self.live] if self.last_x1 is None else self.last_x1

    @property
    def src0(self):
        """the PreFold sources of a first fold (None in S3: nothing is folded; None after an in-place fold)"""
        return self.last_src0

    def row(self, kind):
        """(the arrays of a row, the spare buffer that ends where the first begins or None, the one that begins where the last ends or None)"""
        arrays = {"live": self.live, "x1": self.x1, "src0": self.src0}[kind]
        spares = [self.named[k] for k in ("pre_in", "post_in", "pre_f", "post_f")]
        before = [b for b in spares if b.end == arrays[0].off]
        after = [b for b in spares if b.off == arrays[-1].end]
        assert (bool(before), bool(after)) == ISOLATED[self.state][kind]
        return arrays, (before[0] if before else None), (after[0] if after else None)

    def take(self, n, name="out"):
        """n elements of the work area"""
        b = self.work.sub(self.work_top, self.work_top + n)
        b.name = name
        self.work_top += n
        return b

    # ---- the prover's steps, on the device and on the model
    def upload(self):
        self.hal.sync()
        self.region = self.hal.dev_alloc().alloc(self.total)
        self.hal.copy_h2d(self.mem, self.region)

    def _exprs(self):
        from binius_amd.sumcheck import bivariate_product_expr

        cache = self.hal.__dict__.setdefault("_deferred_states_exprs", {})
        key = tuple(self.comps)
        if key not in cache:
            cache[key] = [bivariate_product_expr(self.hal, i, j) for i, j in self.comps]
        return cache[key]

    def execute(self, what="execute"):
        """calculate_round_evals of the current arrays: the device's values must be the oracle's on the model"""
        rc, want = self.oracle.round_evals([b.host.copy() for b in self.live], self.n_rem, self.comps, self.bc)
        assert rc == 0
        if self.hal is not None:
            from binius_amd.sumcheck import calculate_round_evals

            got = calculate_round_evals(self.hal, self.n_rem, self.coeffs, [b.dev for b in self.live], self._exprs())
            assert list(got) == list(want), "%s (%d variables left): the round values are not the oracle's" % (what, self.n_rem)
        return want

    def fold(self):
        z = next(self.zs)
        half = 1 << (self.n_rem - 1)
        src = self.live
        dst = [f.sub(0, half) for f in self.fresh]
        e1 = [s.sub(half, 2 * half) for s in src]
        if self.hal is not None:
            if self.pre_fold:  # allocate a new buffer for the folded evaluations and copy in evals_0
                for s, d in zip(src, dst):
                    self.hal.copy_d2d(s.sub(0, half).dev, d.dev)
            self.hal.extrapolate_line_batch([d.dev for d in dst], [e.dev for e in e1], z)
        for s, d, e in zip(src, dst, e1):
            lo = s.sub(0, half).host.copy()
            assert self.oracle.extrapolate_line(lo, e.host.copy(), z) == 0
            d.host[:] = lo
        self.last_x1, self.last_src0 = e1, ([s.sub(0, half) for s in src] if self.pre_fold else None)
        self.pre_fold = False
        self.n_rem -= 1

    def drive(self):
        """the prover's steps up to the state"""
        if self.state != "S1":
            self.execute("the execute() on the way to the state")
        if self.state != "S3":
            self.fold()
        if self.state == "S4x2":
            self.execute("the second execute() on the way to the state")
            self.fold()

    # ---- what a case asserts after its foreign call
    def continuation(self):
        """one more execute, fold, execute: a stale host copy or a stale sum computed ahead would answer here"""
        self.execute("continuation, first execute")
        self.fold()
        self.execute("continuation, second execute")

    def check_bytes(self):
        """after sync(), every buffer of the case equals the model byte for byte"""
        self.hal.sync()
        got = self.hal.copy_d2h(self.region)
        if not np.array_equal(got, self.mem):
            at = int(np.nonzero((got != self.mem).any(axis=1))[0][0])
            name = [b.name + "[%d]" % (at - b.off) for b in self.named.values() if b.off <= at < b.end][0]
            raise AssertionError("device memory differs from the model at element %d (%s)" % (at, name))


def reach(hal, oracle, state, seed=0, stage=None, log_n=LOG_N):
    """Drive the prover into `state` on `hal` (a context of make_context(state) / Contexts.get(state)) and prove from the counters
    that it is there; the case FAILS otherwise.  stage(preview, st): called before anything is uploaded, with the model alone driven
    to the state (preview) and the prover about to start (st): what the case needs on the device beforehand -- an upload would flush
    the state -- it writes into buffers of st.take(), reading preview.mem for what the arrays WILL hold.  log_n: another size for the
    multilinears (S1 and S2 are reached at any; the hosted states only up to the context's BN_GROUP_HT_MAX_LOG2).  Returns the Prover."""
    if state in HOSTED and hal.arm_counters()["ht_max"] == 0:
        pytest.skip(NO_HOST_TAIL)
    st = Prover(hal, oracle, state, seed, log_n=log_n)
    if stage is not None:
        preview = Prover(None, oracle, state, seed, mem=st.mem.copy(), log_n=log_n)
        preview.drive()
        stage(preview, st)
    st.upload()
    before = hal.group_counters()
    st.drive()
    d = moved(before, hal.group_counters())
    hosted = [k for k in d if k.startswith("hosted")]
    if state == "S1":
        # (a fold that is not the claim groups' and, the context being lazy, has not run: nothing of the group path moved; that it is
        # pending and not performed shows when the case's forced call leaves the group counters alone, too)
        assert not d and "BN_NO_LAZY_FOLD" not in os.environ, ("S1 not reached", d)
    elif state == "S2":
        assert d.get("evals", 0) >= 1 and "flushed_folds" not in d and not hosted, ("S2 not reached", d)
    elif state == "S3":
        assert d.get("hosted_started", 0) == 1 and "hosted_folds" not in d and "hosted_writebacks" not in d, ("S3 not reached", d)
    else:
        folds = 2 if state == "S4x2" else 1
        assert d.get("hosted_started", 0) == 1 and d.get("hosted_folds", 0) == folds and "hosted_writebacks" not in d and "flushed_folds" not in d, (state + " not reached", d)
    st.reached = d
    return st
