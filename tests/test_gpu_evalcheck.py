"""GPU parity of evalcheck's column projection and bivariate prover: bn_partial_eval_high_batch (binius_amd/csrc/kernels_partial_eval.hip
+ abi_partial_eval.cpp; reference: evaluate_partial_high under collect_projected_mles, evalcheck/subclaims.rs:356-439) against
oracle.fold_left, and bnh_evalcheck_bivariate_prove (binius_amd/host/evalcheck.hpp; reference: subclaims.rs:52-145, 549-586) against
tests/evalcheck_ref.py (pinned by tests/test_evalcheck_oracle.py).  Everything is bit-exact and nothing is compared with the device's own
output.  Inputs and outputs of the op sit between canary frames at bases that are odd multiples of 16 bytes (inputs at leads 1, 3, 5, ..,
outputs at leads 9, 11, 13, .. modulo 16: their offsets modulo 256 bytes differ); an output's body holds the canary before the call, so a result also pins that outputs are overwritten, not accumulated.  One context per module."""
import functools

import numpy as np
import pytest

import adversarial as A
import evalcheck_ref as R

pytestmark = pytest.mark.gpu

ARENA_ELEMS = 1 << 23


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, ARENA_ELEMS)
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def random_column(seed, level, n_vars):
    """2^n_vars random values of the level, packed: 2^(n_vars + level - 7) elements."""
    import oracle

    return oracle.random_b128(seed, 1 << (n_vars + level - 7))


@functools.lru_cache(maxsize=None)
def random_query(seed, q):
    import oracle

    return R.eq_expand(oracle.random_scalars(seed, q))


def expected(col, level, n_vars, vec):
    import oracle

    q = vec.shape[0].bit_length() - 1
    out = oracle.arr(1 << (n_vars - q))
    assert oracle.fold_left(np.ascontiguousarray(col), level, vec, out) == 0
    return out


def delta(hal, before):
    now = hal.partial_eval_counters()
    return {k: now[k] - before[k] for k in now if k != "max_share"}, now["max_share"]


def run_batch(hal, cols, vec):
    """cols: [(packed array, tower_level, n_vars)]; vec: the 2^q query.  One call for all columns, every output against the oracle and
    against Context.fold_left of the same column, frames intact, inputs unchanged.  Returns the counter deltas of the batch call."""
    alloc = hal.dev_alloc()
    q = vec.shape[0].bit_length() - 1
    checks, lead = [], 1
    d_vec, chk = A.place(hal, alloc, vec, lead)
    checks.append(chk)
    d_cols, d_outs, out_checks = [], [], []
    for col, level, n_vars in cols:
        lead += 2
        s, chk = A.place(hal, alloc, col, lead)
        checks.append(chk)
        d_cols.append((s, level, n_vars))
        o, ochk = A.place(hal, alloc, 1 << (n_vars - q), lead + 8)
        d_outs.append(o)
        out_checks.append(ochk)
    before = hal.partial_eval_counters()
    hal.partial_eval_high_batch(d_cols, d_vec, q, d_outs)
    got = delta(hal, before)
    wants = [expected(col, level, n_vars, vec) for col, level, n_vars in cols]
    for t, (ochk, want) in enumerate(zip(out_checks, wants)):
        try:
            ochk(want)
        except AssertionError as e:
            raise AssertionError("column %d (level %d, n_vars %d, query_vars %d): %s" % (t, cols[t][1], cols[t][2], q, e))
    for chk in checks:
        chk()
    single = alloc.alloc(max(w.shape[0] for w in wants))
    for (s, level, n_vars), want in zip(d_cols, wants):
        o = single.slice(0, want.shape[0])
        hal.fill(o, A.CANARY)
        hal.fold_left(s, level, d_vec, o)
        assert np.array_equal(hal.copy_d2h(o), want), "fold_left differs (level %d, n_vars %d)" % (level, n_vars)
    return got


ONE_COLUMN = (
    [(0, 7, 6), (0, 13, 6), (0, 20, 6)]
    + [(0, 16, b) for b in (0, 1, 5, 7, 10)]
    + [(0, 7, 7), (0, 10, 10)]  # query_vars == 0: the column widened to B128
    + [(level, 12 + level % 3, b) for level in (3, 4, 5, 6, 7) for b in (0, 3, 6)]
    + [(5, 4, 4), (7, 0, 0), (6, 9, 9)]  # query_vars == 0 at the other levels; the smallest columns
)


@pytest.mark.parametrize("level,n_vars,b", ONE_COLUMN)
def test_one_column(hal, level, n_vars, b):
    col = random_column(0xE1000 + 64 * n_vars + level, level, n_vars)
    (d, share) = run_batch(hal, [(col, level, n_vars)], random_query(0xE1100 + n_vars - b, n_vars - b))
    assert d == {"calls": 1, "launches": 2, "cols_kernel": 1, "cols_fallback": 0, "fold_left_routed": 0}
    if (level, n_vars, b) == (0, 20, 6):
        # 2^14 rows of 64 bits: a unit takes at most 1024 rows, so at least 16 workgroups share the column and are XOR-combined
        assert share >= 16
    if n_vars == b:
        assert share == 1


def mixed_batch():
    cols = []
    for t in range(40):
        level = (0, 3, 4, 5, 6, 7, 0, 0)[t % 8]
        b = (6, 3, 0, 5, 1, 7, 2, 6, 4, 10)[t % 10]
        n_vars = 9 + b  # one query of 9 variables
        cols.append((random_column(0xE2000 + t, level, n_vars), level, n_vars))
    return cols


def test_mixed_batch_shares_the_launches_of_its_largest_column(hal):
    cols = mixed_batch()
    assert {c[1] for c in cols} == {0, 3, 4, 5, 6, 7}
    vec = random_query(0xE2100, 9)
    d, share = run_batch(hal, cols, vec)
    assert d["calls"] == 1 and d["cols_kernel"] == 40 and d["cols_fallback"] == 0
    assert share >= 2
    largest = max(cols, key=lambda c: c[0].shape[0])
    d1, _ = run_batch(hal, [largest], vec)
    assert d["launches"] == d1["launches"]


def test_wide_column_falls_back_inside_the_call(hal):
    cols = [(random_column(0xE3000, 0, 17), 0, 17), (random_column(0xE3001, 4, 17), 4, 17), (random_column(0xE3002, 0, 12), 0, 12),
            (random_column(0xE3003, 6, 17), 6, 17)]
    d, _ = run_batch(hal, cols, random_query(0xE3100, 6))  # outputs of 2048, 2048, 64 and 2048 elements
    assert d == {"calls": 1, "launches": 2, "cols_kernel": 1, "cols_fallback": 3, "fold_left_routed": 0}


@pytest.mark.parametrize("kind", ["zero", "ones", "single_bit", "last_bit"])
def test_adversarial_columns(hal, kind):
    def make(level, n_vars):
        n = 1 << (n_vars + level - 7)
        a = np.zeros((n, 2), dtype=np.uint64)
        if kind == "ones":
            a[:] = np.uint64(A.M64)
        elif kind == "single_bit":
            a[n // 3, 1] = np.uint64(1 << 37)
        elif kind == "last_bit":
            a[n - 1, 1] = np.uint64(1 << 63)
        return a

    cols = [(make(level, n_vars), level, n_vars) for level, n_vars in ((0, 16), (0, 15), (0, 20), (3, 13), (5, 12), (7, 10))]
    run_batch(hal, cols, random_query(0xE4000, 10))


def test_query_of_zeros_and_ones(hal):
    import oracle

    vec = oracle.arr(1 << 10)
    vec[:, 0] = (oracle.splitmix_words(0xE5000, 1 << 10) & np.uint64(1))
    cols = [(random_column(0xE5001 + t, level, 10 + b), level, 10 + b) for t, (level, b) in enumerate(((0, 6), (0, 2), (0, 8), (4, 3), (6, 6), (7, 1)))]
    run_batch(hal, cols, vec)
    run_batch(hal, cols, np.zeros((1 << 10, 2), dtype=np.uint64))


def test_fold_left_is_routed_at_evalcheck_shapes(hal):
    alloc = hal.dev_alloc()
    for level, n_vars, q, routed in ((0, 18, 12, 1), (5, 15, 12, 1), (0, 17, 11, 0), (0, 24, 13, 0)):
        alloc = hal.dev_alloc()
        col, vec = random_column(0xE6000 + n_vars, level, n_vars), random_query(0xE6100 + q, q)
        s, chk = A.place(hal, alloc, col, 3)
        v, vchk = A.place(hal, alloc, vec, 5)
        out, ochk = A.place(hal, alloc, 1 << (n_vars - q), 7)
        before = hal.partial_eval_counters()
        hal.fold_left(s, level, v, out)
        d, _ = delta(hal, before)
        assert d["fold_left_routed"] == routed and d["calls"] == 0 and d["launches"] == 2 * routed, (level, n_vars, q, d)
        ochk(expected(col, level, n_vars, vec))
        chk()
        vchk()


def test_validation_rejects_and_counts_nowhere(hal):
    from binius_amd._ffi import BnError

    alloc = hal.dev_alloc()
    col, vec, out = alloc.alloc(1 << 6), alloc.alloc(1 << 7), alloc.alloc(1 << 6)
    hal.fill(col, 1)
    hal.fill(vec, 1)
    hal.fill(out, A.CANARY)
    before = hal.partial_eval_counters()
    good = (col, 0, 13)
    hal.partial_eval_high_batch([], vec, 7, [])  # n_cols == 0: a no-op
    bad_calls = [
        ([(None, 0, 13)], vec, 7, [out]),
        ([good], None, 7, [out]),
        ([good], vec, 7, [None]),
        ([(col, 1, 13)], vec, 7, [out]),
        ([(col, 2, 13)], vec, 7, [out]),
        ([(col, 8, 13)], vec, 7, [out]),
        ([(col, 0, 6)], vec, 7, [out]),       # query_vars > n_vars
        ([good, (col, 0, 5)], vec, 7, [out, out]),  # the second column is rejected: nothing runs
        ([(col, 0, 6)], vec, 0, [out]),       # less than one 128-bit element
        ([good], vec, 7, []),                  # fewer outputs than columns
    ]
    for args in bad_calls:
        with pytest.raises(BnError):
            hal.partial_eval_high_batch(*args)
    d, _ = delta(hal, before)
    assert all(v == 0 for v in d.values()), d
    got = hal.copy_d2h(out)
    assert (got[:, 0] == np.uint64(A.CANARY & A.M64)).all(), "a rejected call wrote to its output"


# ------------------------------------------------------------------------------------------------ the prover
def run_prover(hal, provers, pool, seed):
    """provers in the form of tests/evalcheck_ref.py (numpy columns, sums filled in here).  Transcript against the restatement, the
    restatement's transcript against its verifier, columns unchanged, a second run repeats the transcript."""
    import oracle
    from binius_amd._host import EvalcheckPlan

    tables = R.resolve(provers, pool)
    provers = [(b, mls, comps, R.claim_sums(tabs, comps)) for (b, mls, comps, _), tabs in zip(provers, tables)]
    bcs = oracle.random_scalars(seed, len(provers))
    chs = oracle.random_scalars(seed + 1, max(p[0] for p in provers))
    want_proofs, want_evals = R.prove(provers, pool, bcs, chs, tables=tables)
    assert R.verify(provers, pool, bcs, chs, want_proofs, want_evals)

    alloc = hal.dev_alloc()
    placed, checks, lead = {}, [], 1
    dev = []
    for b, mls, comps, sums in provers:
        dmls = []
        for ml in mls:
            if ml[0] == "proj":
                if id(ml[1]) not in placed:
                    placed[id(ml[1])], chk = A.place(hal, alloc, ml[1], lead)
                    checks.append(chk)
                    lead += 2
                dmls.append(("proj", placed[id(ml[1])]) + tuple(ml[2:]))
            else:
                dmls.append(ml)
        dev.append((b, dmls, comps, sums))
    scratch = alloc.alloc(EvalcheckPlan.scratch_elems(dev))
    for _ in range(2):
        hal.fill(scratch, A.CANARY)
        before = hal.partial_eval_counters()
        plan = EvalcheckPlan(hal, dev, pool, scratch, bcs, chs)
        plan.run()
        assert plan.round_proofs() == want_proofs, "round proofs differ from the restatement"
        assert plan.final_evals() == want_evals, "final evaluations differ from the restatement"
        d, _ = delta(hal, before)
        for chk in checks:
            chk()
    return d, dev


def test_prover_u32_add_like(hal):
    import oracle

    pool = oracle.random_scalars(0xE7000, 15)  # [0:5) the low coordinates, [5:15) the suffix
    cols = [random_column(0xE7100 + t, 0, 15) for t in range(4)]
    mls, comps = [], []
    for c in cols:
        comps.append((len(mls), len(mls) + 1))
        mls += [("proj", c, 0, 15, 5, 10), ("shift", 5, 1, R.LOGICAL_LEFT, 0, 5)]
    d, _ = run_prover(hal, [(5, mls, comps, None)], pool, 0xE7200)
    assert d["calls"] == 1 and d["cols_kernel"] == 4  # one suffix: one batch call


def test_prover_keccak_like(hal):
    import oracle

    pool = oracle.random_scalars(0xE8000, 36)  # [0:6) r, [6:16) its suffix; [16:26) the packed claims' point; [26:29) r of B64, [29:36) suffix
    c1 = [random_column(0xE8100 + t, 0, 16) for t in range(30)]
    c64 = [random_column(0xE8200 + t, 6, 10) for t in range(5)]
    shifts, comps_s = [], []
    for t, c in enumerate(c1):
        comps_s.append((len(shifts), len(shifts) + 1))
        shifts += [("proj", c, 0, 16, 6, 10), ("shift", 6, (1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14, 63)[t % 25], R.CIRCULAR_LEFT, 0, 6)]
    packed, comps_p = [("basis", 6, 0)], []
    for c in c1[:8]:
        comps_p.append((len(packed), 0))
        packed.append(("proj", c, 0, 16, 16, 10))
    right, comps_r = [("shift", 3, 1, R.LOGICAL_RIGHT, 26, 3)], []
    for c in c64:
        comps_r.append((len(right), 0))
        right.append(("proj", c, 6, 10, 29, 7))
    d, _ = run_prover(hal, [(3, right, comps_r, None), (6, shifts, comps_s, None), (6, packed, comps_p, None)], pool, 0xE8300)
    # three suffixes: three batch calls; 30 + 8 + 5 projections
    assert d["calls"] == 3 and d["cols_kernel"] == 43 and d["launches"] == 6


def test_prover_projects_duplicates_once_and_takes_an_empty_suffix(hal):
    import oracle

    pool = oracle.random_scalars(0xE9000, 20)
    a, b_ = random_column(0xE9100, 0, 14), random_column(0xE9101, 0, 14)
    whole = random_column(0xE9102, 6, 3)  # exactly b = 3 variables: the widened column itself
    p3 = (3, [("proj", whole, 6, 3, 0, 0), ("shift", 3, 5, R.CIRCULAR_LEFT, 0, 3), ("proj", whole, 6, 3, 0, 0), ("basis", 3, 3)], [(0, 1), (2, 3), (0, 2)], None)
    p6 = (6, [("proj", a, 0, 14, 6, 8), ("shift", 6, 9, R.LOGICAL_RIGHT, 0, 6), ("proj", a, 0, 14, 6, 8), ("shift", 6, 1, R.LOGICAL_LEFT, 0, 6), ("proj", b_, 0, 14, 6, 8),
              ("proj", a, 0, 14, 12, 8), ("proj", a, 3, 11, 6, 5)], [(0, 1), (2, 3), (4, 1), (5, 3), (6, 1)], None)
    d, _ = run_prover(hal, [p3, p6], pool, 0xE9200)
    # projections: (whole, empty) once; (a, [6:14)) once, (b, [6:14)), (a, [12:20)); the bytes of a read as B8 values at [6:11): its own table
    assert d["calls"] == 4 and d["cols_kernel"] == 5


def test_prover_rejects_invalid_shift_arguments(hal):
    import oracle
    from binius_amd._ffi import BnError
    from binius_amd._host import EvalcheckPlan

    pool = oracle.random_scalars(0xEA000, 16)
    alloc = hal.dev_alloc()
    col = alloc.alloc(1 << 6)
    hal.fill(col, 0)
    for shift in (("shift", 6, 0, 0, 0, 6), ("shift", 6, 64, 0, 0, 6), ("shift", 6, 1, 0, 0, 5), ("shift", 6, 1, 3, 0, 6), ("shift", 5, 1, 0, 0, 5)):
        dev = [(6, [("proj", col, 0, 13, 6, 7), shift], [(0, 1)], [0])]
        plan = EvalcheckPlan(hal, dev, pool, alloc.alloc(1 << 12), [1], oracle.random_scalars(1, 6))
        with pytest.raises(BnError):
            plan.run()
