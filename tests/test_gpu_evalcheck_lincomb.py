"""GPU parity of the projection of linear-combination inner columns: bn_partial_eval_high_lincomb_batch (binius_amd/csrc/
kernels_partial_eval_lincomb.hip + abi_partial_eval_lincomb.cpp; reference: try_build_partial_eval, evalcheck/subclaims.rs:305-346) and
bnh_evalcheck_bivariate_prove_lc (binius_amd/host/evalcheck.hpp) against tests/evalcheck_lincomb_ref.py (pinned by
tests/test_evalcheck_lincomb_oracle.py).  Everything is bit-exact and nothing is compared with the device's own output.  As in
tests/test_gpu_evalcheck.py, inputs and outputs sit between canary frames at bases that are odd multiples of 16 bytes and an output's body
holds the canary before the call, so a result also pins that outputs are overwritten, not accumulated.  One context per module."""
import functools

import numpy as np
import pytest

import adversarial as A
import evalcheck_lincomb_ref as L
import evalcheck_ref as R

pytestmark = pytest.mark.gpu

ARENA_ELEMS = 1 << 23
GENERATOR = 0x2E895399AF449ACE499596F6E5FCCAFA  # the multiplicative generator of B128 (tests/golden/field_kats.json, pinned by the oracle test)
SUBFIELD_GENERATOR = 0x2  # the generator of the tower's second level: a coefficient beside the five below
B8_ELEMENT = 0x53
# the generator of B128, all ones, the top basis element, an element of B8, zero
COEFFS = (GENERATOR, A.ALL_ONES, 1 << 127, B8_ELEMENT, 0)
PEL_ZERO = {"calls": 0, "launches": 0, "jobs": 0, "terms": 0, "classes": 0, "jobs_fallback": 0}


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, ARENA_ELEMS)
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def random_column(seed, level, n_vars):
    import oracle

    return oracle.random_b128(seed, 1 << (n_vars + level - 7))


@functools.lru_cache(maxsize=None)
def random_query(seed, q):
    import oracle

    return R.eq_expand(oracle.random_scalars(seed, q))


def delta(hal, before):
    now = hal.partial_eval_lincomb_counters()
    return {k: now[k] - before[k] for k in now if k != "max_share"}, now["max_share"]


def n_classes(jobs):
    """Row loops the plan must make: distinct (tower level, non-zero coefficient) pairs per job."""
    return sum(len({(level, coeff) for _c, level, coeff in terms if coeff}) for _n, terms, _o in jobs)


def run_batch(hal, jobs, vec):
    """jobs: [(n_vars, [(packed array, tower_level, coeff)], offset)]; vec: the 2^q query.  One call for all jobs, every output against the
    restatement, frames intact, inputs unchanged, the BN_PE_* counters unmoved.  Returns the counter deltas and the outputs."""
    alloc = hal.dev_alloc()
    q = vec.shape[0].bit_length() - 1
    placed, checks, lead = {}, [], 1
    d_vec, chk = A.place(hal, alloc, vec, lead)
    checks.append(chk)
    d_jobs, d_outs, out_checks = [], [], []
    for n_vars, terms, offset in jobs:
        d_terms = []
        for col, level, coeff in terms:
            if id(col) not in placed:
                lead += 2
                placed[id(col)], chk = A.place(hal, alloc, col, lead)
                checks.append(chk)
            d_terms.append((placed[id(col)], level, coeff))
        d_jobs.append((n_vars, d_terms, offset))
        o, ochk = A.place(hal, alloc, 1 << (n_vars - q), len(d_outs) * 2 + 9)
        d_outs.append(o)
        out_checks.append(ochk)
    before, pe_before = hal.partial_eval_lincomb_counters(), hal.partial_eval_counters()
    hal.partial_eval_high_lincomb_batch(d_jobs, d_vec, q, d_outs)
    got = delta(hal, before)
    assert hal.partial_eval_counters() == pe_before, "the BN_PE_* counters moved"
    bodies = []
    for j, (ochk, (n_vars, terms, offset)) in enumerate(zip(out_checks, jobs)):
        want = L.project_lincomb(terms, offset, n_vars, None, query=vec)
        try:
            bodies.append(ochk(want))
        except AssertionError as e:
            raise AssertionError("job %d (n_vars %d, levels %s, query_vars %d): %s" % (j, n_vars, [t[1] for t in terms], q, e))
    for chk in checks:
        chk()
    d, share = got
    assert d["calls"] == 1 and d["jobs"] == len(jobs) and d["terms"] == sum(len(j[1]) for j in jobs) and d["classes"] == n_classes(jobs), d
    return d, share, bodies


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("level,n_vars,b", [(0, 7, 6), (0, 16, 0), (0, 16, 5), (0, 16, 7), (0, 16, 10), (0, 10, 10), (5, 14, 3), (7, 0, 0)])
def test_one_term_agrees_with_the_plain_op(hal, level, n_vars, b):
    col = random_column(0xD1000 + 64 * n_vars + level, level, n_vars)
    vec = random_query(0xD1100 + n_vars - b, n_vars - b)
    d, share, bodies = run_batch(hal, [(n_vars, [(col, level, 1)], 0)], vec)
    assert d == {"calls": 1, "launches": 2, "jobs": 1, "terms": 1, "classes": 1, "jobs_fallback": 0}
    if n_vars == b:
        assert share == 1
    alloc = hal.dev_alloc()
    s, _ = A.place(hal, alloc, col, 3)
    v, _ = A.place(hal, alloc, vec, 5)
    o, ochk = A.place(hal, alloc, 1 << b, 7)
    hal.partial_eval_high_batch([(s, level, n_vars)], v, n_vars - b, [o])
    assert np.array_equal(ochk(bodies[0]), bodies[0]), "bn_partial_eval_high_batch gives another table"


@pytest.mark.parametrize("b", [3, 6, 7])
@pytest.mark.parametrize("T", [2, 5, 9, 64])
def test_terms_of_one_class_share_a_row_loop(hal, T, b):
    n_vars = 13
    cols = [random_column(0xD2000 + t, 0, n_vars) for t in range(T)]
    vec = random_query(0xD2100 + b, n_vars - b)
    d, _, _ = run_batch(hal, [(n_vars, [(c, 0, 1) for c in cols], 0)], vec)
    assert d["classes"] == 1 and d["terms"] == T and d["launches"] == 2


@pytest.mark.parametrize("b", [3, 6, 7])
def test_a_column_listed_twice_cancels(hal, b):
    n_vars = 13
    cols = [random_column(0xD2000 + t, 0, n_vars) for t in range(5)]
    vec = random_query(0xD2100 + b, n_vars - b)
    d, _, twice = run_batch(hal, [(n_vars, [(c, 0, 1) for c in cols + [cols[2]]], 0)], vec)
    assert d["classes"] == 1 and d["terms"] == 6
    _, _, without = run_batch(hal, [(n_vars, [(c, 0, 1) for c in cols[:2] + cols[3:]], 0)], vec)
    assert np.array_equal(twice[0], without[0])


@pytest.mark.parametrize("b", [0, 3, 6])
def test_mixed_classes(hal, b):
    n_vars = 10
    vec = random_query(0xD3100 + b, n_vars - b)
    ones = [(random_column(0xD3000 + t, level, n_vars), level, 1) for t, level in enumerate((0, 3, 0, 3))]
    d, _, _ = run_batch(hal, [(n_vars, ones, 0)], vec)
    assert d["classes"] == 2
    terms = list(ones)
    for k, level in enumerate((3, 4, 5, 6, 7)):
        terms += [(random_column(0xD3010 + 4 * k + i, level, n_vars), level, COEFFS[(k + i) % 5]) for i in range(3)]
    assert {t[2] for t in terms} == set(COEFFS) | {1}
    terms.append((random_column(0xD3030, 3, n_vars), 3, SUBFIELD_GENERATOR))
    d, _, _ = run_batch(hal, [(n_vars, terms, 0x0123456789ABCDEF_FEDCBA9876543210)], vec)
    assert d["classes"] == 2 + 15 - 3 + 1 and d["launches"] == 2  # three of the fifteen coefficients are zero: they plan nothing


def test_degenerate_shapes(hal):
    import oracle

    offset = 0xA5A5 << 100
    # no terms: the offset alone
    d, _, bodies = run_batch(hal, [(9, [], offset)], random_query(0xD4000, 3))
    assert d == {"calls": 1, "launches": 2, "jobs": 1, "terms": 0, "classes": 0, "jobs_fallback": 0}
    assert oracle.arr_to_ints(bodies[0]) == [offset] * 64
    mixed = lambda n_vars, seed: [(random_column(seed, 0, n_vars), 0, 1), (random_column(seed + 1, 0, n_vars), 0, 1), (random_column(seed + 2, 4, n_vars), 4, GENERATOR)]
    # query_vars = 0: the combination widened to B128
    d, share, _ = run_batch(hal, [(8, mixed(8, 0xD4100), offset), (7, [(random_column(0xD4110, 0, 7), 0, B8_ELEMENT)], 0)], oracle.ints_to_arr([1]))
    assert share == 1 and d["launches"] == 2
    # query_vars = n_vars: one element
    run_batch(hal, [(11, mixed(11, 0xD4200), offset), (11, [], 1)], random_query(0xD4201, 11))
    # a zero coefficient beside nothing else
    d, _, bodies = run_batch(hal, [(9, [(random_column(0xD4300, 0, 9), 0, 0)], offset)], random_query(0xD4000, 3))
    assert d["classes"] == 0 and oracle.arr_to_ints(bodies[0]) == [offset] * 64


def test_workgroups_of_one_job_are_combined_after_the_scaling(hal):
    # 2^14 rows of 64 bits: a unit takes at most 1024 rows; the coefficient is applied by every workgroup before the XOR atomics
    cols = [random_column(0xD5000 + t, 0, 20) for t in range(5)]
    d, share, _ = run_batch(hal, [(20, [(c, 0, GENERATOR) for c in cols], 0xFF), (20, [(c, 0, 1) for c in cols], 0)], random_query(0xD5100, 14))
    assert share >= 2 and d["classes"] == 2 and d["launches"] == 2


@functools.lru_cache(maxsize=None)
def mixed_jobs():
    jobs = []
    for t in range(40):
        b = (6, 3, 0, 5, 1, 7, 2, 6, 4, 10)[t % 10]
        n_vars = 9 + b  # one query of 9 variables
        terms = []
        for i in range(1 + t % 4):
            # (the widest jobs stay at the narrow levels: the CPU restatement of a 2^19-element column of B64 costs a second)
            level = (0, 3, 4, 5, 6, 7, 0, 0)[(t + 3 * i) % 8] if b < 7 else (0, 3, 0, 4)[(t + i) % 4]
            # three columns per (level, n_vars): shared between the jobs of a shape and listed more than once in some
            terms.append((random_column(0xD6000 + (t + i) % 3, level, n_vars), level, ((1, 1) + COEFFS[:4])[(t + i) % 6]))
        jobs.append((n_vars, terms, t * 0x1_0000_0001))
    return jobs


def test_mixed_batch_shares_the_launches_of_its_largest_job(hal):
    jobs = mixed_jobs()
    assert {t[1] for j in jobs for t in j[1]} == {0, 3, 4, 5, 6, 7}
    assert len({id(t[0]) for j in jobs for t in j[1]}) < 0.75 * sum(len(j[1]) for j in jobs)  # columns are shared
    vec = random_query(0xD6100, 9)
    d, share, _ = run_batch(hal, jobs, vec)
    assert d["jobs"] == 40 and d["jobs_fallback"] == 0 and share >= 2
    largest = max(jobs, key=lambda j: (j[0], len(j[1])))
    d1, _, _ = run_batch(hal, [largest], vec)
    assert d["launches"] == d1["launches"] == 2


def test_wide_job_falls_back_inside_the_call(hal):
    vec = random_query(0xD6100, 9)
    wide = (21, [(random_column(0xD7000, 0, 21), 0, 1), (random_column(0xD7001, 0, 21), 0, 1), (random_column(0xD7002, 3, 21), 3, B8_ELEMENT)], 0x77 << 64)
    d, _, _ = run_batch(hal, mixed_jobs()[:6] + [wide], vec)  # the last job has 4096 outputs
    assert d["jobs_fallback"] == 1 and d["launches"] == 3
    d1, _, _ = run_batch(hal, [wide], vec)  # alone: nothing to clear and no unit to run, its own launch only
    assert d1["jobs_fallback"] == 1 and d1["launches"] == 1


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

    jobs = []
    for t, (level, n_vars) in enumerate(((0, 16), (0, 15), (0, 20), (3, 13), (5, 12), (7, 10))):
        adv = make(level, n_vars)
        jobs.append((n_vars, [(adv, level, 1), (random_column(0xD8000 + t, level, n_vars), level, 1), (adv, level, COEFFS[t % 4])], A.ALL_ONES))
    run_batch(hal, jobs, random_query(0xD8100, 10))


def test_query_of_zeros_and_ones(hal):
    import oracle

    vec = oracle.arr(1 << 10)
    vec[:, 0] = oracle.splitmix_words(0xD9000, 1 << 10) & np.uint64(1)
    jobs = [(10 + b, [(random_column(0xD9001 + t, level, 10 + b), level, 1), (random_column(0xD9011 + t, level, 10 + b), level, COEFFS[t % 4])], t)
            for t, (level, b) in enumerate(((0, 6), (0, 2), (0, 8), (4, 3), (6, 6), (7, 1)))]
    run_batch(hal, jobs, vec)
    run_batch(hal, jobs, np.zeros((1 << 10, 2), dtype=np.uint64))


def test_validation_rejects_and_counts_nowhere(hal):
    import ctypes as C

    from binius_amd._ffi import BnError, DevSlice, F128, PelJob, PelTerm

    alloc = hal.dev_alloc()
    col, cchk = A.place(hal, alloc, random_column(0xDA000, 0, 13), 3)  # 64 elements
    vec, vchk = A.place(hal, alloc, random_query(0xDA001, 7), 5)
    out, ochk = A.place(hal, alloc, 1 << 6, 9)
    out2, ochk2 = A.place(hal, alloc, 1 << 6, 11)
    before, pe_before = hal.partial_eval_lincomb_counters(), hal.partial_eval_counters()
    hal.partial_eval_high_lincomb_batch([], vec, 7, [])  # n_jobs == 0: a no-op
    hal.partial_eval_high_lincomb_batch([], None, 7, [])
    odd = lambda s: DevSlice(s.ptr + 8, s.len)
    good = (13, [(col, 0, 1)], 0)
    bad_calls = [
        ([(13, [(None, 0, 1)], 0)], vec, 7, [out]),
        ([good], None, 7, [out]),
        ([good], vec, 7, [None]),
        ([(13, [(odd(col), 0, 1)], 0)], vec, 7, [out]),
        ([good], odd(vec), 7, [out]),
        ([good], vec, 7, [odd(out)]),
        ([(13, [(col, 1, 1)], 0)], vec, 7, [out]),
        ([(13, [(col, 2, 1)], 0)], vec, 7, [out]),
        ([(13, [(col, 8, 1)], 0)], vec, 7, [out]),
        ([(6, [(col, 3, 1)], 0)], vec, 7, [out]),         # n_vars < query_vars
        ([(41, [(col, 0, 1)], 0)], vec, 7, [out]),        # n_vars > BN_PE_MAX_VARS
        ([(6, [(col, 0, 1)], 0)], vec, 0, [out]),         # less than one 128-bit element
        ([good, (13, [(col, 0, 1), (col, 1, 1)], 0)], vec, 7, [out, out2]),  # the second job is rejected: nothing runs
        ([(13, [(col, 0, 1)] * 65, 0)], vec, 7, [out]),  # more than BN_PEL_MAX_TERMS terms
        ([good], vec, 7, [col]),                           # the output is the column
        ([good], vec, 7, [vec.slice(0, 64)]),              # the output lies in the query
        ([good], vec, 7, [DevSlice(col.ptr + 16 * 63, 64)]),  # the output's first element is the column's last
        ([good, good], vec, 7, [out, out]),                # two jobs, one output
        ([good, good], vec, 7, [out, DevSlice(out.ptr + 16 * 63, 64)]),
        ([good, (13, [(out, 0, 1)], 0)], vec, 7, [out, out2]),  # an output is another job's column
        ([good], vec, 7, []),                              # fewer outputs than jobs
    ]
    for args in bad_calls:
        with pytest.raises(BnError) as e:
            hal.partial_eval_high_lincomb_batch(*args)
        assert e.value.kind == "InputValidation", args
    # what the list form cannot say: a nonzero reserved field, a term range outside the term table, no array of outputs, an array of
    # outputs that ends in a null before the last job's
    outs = (C.c_void_p * 1)(out.ptr)
    term = lambda reserved=0: (PelTerm * 1)(PelTerm(col.ptr, 0, reserved, F128(1, 0)))
    job = lambda first=0, n=1, reserved=0: (PelJob * 1)(PelJob(13, first, n, reserved, F128(0, 0)))
    for jobs, terms, n_terms in ((job(reserved=1), term(), 1), (job(), term(reserved=1), 1), (job(first=1), term(), 1), (job(n=2), term(), 1),
                                 (job(first=0xFFFFFFFF, n=2), term(), 1), (job(), None, 1), (None, term(), 1)):
        with pytest.raises(BnError) as e:
            hal.partial_eval_high_lincomb_raw(jobs, 1, terms, n_terms, vec, 7, outs)
        assert e.value.kind == "InputValidation"
    two = (PelJob * 2)(PelJob(13, 0, 1, 0, F128(0, 0)), PelJob(13, 0, 1, 0, F128(0, 0)))
    for jobs, n, d_outs in ((job(), 1, None), (job(), 1, (C.c_void_p * 1)(None)), (two, 2, (C.c_void_p * 2)(out.ptr, None))):
        with pytest.raises(BnError) as e:
            hal.partial_eval_high_lincomb_raw(jobs, n, term(), 1, vec, 7, d_outs)
        assert e.value.kind == "InputValidation"
    d, _ = delta(hal, before)
    assert d == PEL_ZERO and hal.partial_eval_counters() == pe_before
    cchk()
    vchk()
    ochk(None)
    ochk2(None)
    hal.partial_eval_high_lincomb_raw(job(), 1, term(), 1, vec, 7, outs)  # (the arrays above were well-formed but for the field named)
    ochk(L.project_lincomb([(random_column(0xDA000, 0, 13), 0, 1)], 0, 13, None, query=random_query(0xDA001, 7)))


# ------------------------------------------------------------------------------------------------ the prover
def run_prover(hal, provers, pool, seed):
    """provers in the form of tests/evalcheck_lincomb_ref.py (numpy columns, sums filled in here).  Transcript against the restatement,
    the restatement's transcript against its verifier, columns unchanged, a second run repeats the transcript.  Returns the deltas of
    the BN_PEL_* and BN_PE_* counters over one run."""
    import oracle
    from binius_amd._host import EvalcheckPlan

    tables = L.resolve(provers, pool)
    provers = [(b, mls, comps, R.claim_sums(tabs, comps)) for (b, mls, comps, _), tabs in zip(provers, tables)]
    bcs = oracle.random_scalars(seed, len(provers))
    chs = oracle.random_scalars(seed + 1, max(p[0] for p in provers))
    want_proofs, want_evals = L.prove(provers, pool, bcs, chs, tables=tables)
    assert L.verify(provers, pool, bcs, chs, want_proofs, want_evals)

    alloc = hal.dev_alloc()
    placed, checks, lead = {}, [], [1]

    def put(col):
        if id(col) not in placed:
            placed[id(col)], chk = A.place(hal, alloc, col, lead[0])
            checks.append(chk)
            lead[0] += 2
        return placed[id(col)]

    dev = []
    for b, mls, comps, sums in provers:
        dmls = []
        for ml in mls:
            if ml[0] == "proj":
                dmls.append(("proj", put(ml[1])) + tuple(ml[2:]))
            elif ml[0] == "lincomb":
                dmls.append(("lincomb", [(put(c), level, coeff) for c, level, coeff in ml[1]]) + tuple(ml[2:]))
            else:
                dmls.append(ml)
        dev.append((b, dmls, comps, sums))
    scratch = alloc.alloc(EvalcheckPlan.scratch_elems(dev))
    for _ in range(2):
        hal.fill(scratch, A.CANARY)
        before, pe_before = hal.partial_eval_lincomb_counters(), hal.partial_eval_counters()
        plan = EvalcheckPlan(hal, dev, pool, scratch, bcs, chs)
        plan.run()
        assert plan.round_proofs() == want_proofs, "round proofs differ from the restatement"
        assert plan.final_evals() == want_evals, "final evaluations differ from the restatement"
        d, _ = delta(hal, before)
        pe_now = hal.partial_eval_counters()
        pe = {k: pe_now[k] - pe_before[k] for k in pe_now if k != "max_share"}
        for chk in checks:
            chk()
    return d, pe


ROTATIONS = (1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14, 63)


def test_prover_keccak_like(hal):
    import oracle

    pool = oracle.random_scalars(0xDB000, 36)  # [0:6) r, [6:16) its suffix; [16:26) the packed claims' point; [26:29) r of B64, [29:36) suffix
    state = [random_column(0xDB100 + t, 0, 16) for t in range(25)]
    c64 = [random_column(0xDB200 + t, 6, 10) for t in range(3)]
    c = [[(state[5 * y + x], 0, 1) for y in range(5)] for x in range(5)]  # c[x]: the sum of five state columns
    shifts, comps_s = [], []
    for x in range(5):  # c_shift[x]: a rotation of c[x]
        comps_s.append((len(shifts), len(shifts) + 1))
        shifts += [("lincomb", c[x], 0, 16, 6, 10), ("shift", 6, 1, R.CIRCULAR_LEFT, 0, 6)]
    for t in range(6):  # rho rotations of plain columns beside them
        comps_s.append((len(shifts), len(shifts) + 1))
        shifts += [("proj", state[4 * t], 0, 16, 6, 10), ("shift", 6, ROTATIONS[t + 1], R.CIRCULAR_LEFT, 0, 6)]
    comps_s.append((len(shifts), len(shifts) + 1))  # c[0] written again, under another indicator: projected once
    shifts += [("lincomb", list(c[0]), 0, 16, 6, 10), ("shift", 6, 5, R.LOGICAL_LEFT, 0, 6)]
    packed, comps_p = [("basis", 6, 0)], []
    for x in range(2):
        comps_p.append((len(packed), 0))
        packed.append(("lincomb", c[x], 0, 16, 16, 10))  # the same combinations at a second suffix
    comps_p.append((len(packed), 0))
    packed.append(("proj", state[7], 0, 16, 16, 10))
    right, comps_r = [("shift", 3, 1, R.LOGICAL_RIGHT, 26, 3)], []
    for col in c64:
        comps_r.append((len(right), 0))
        right.append(("proj", col, 6, 10, 29, 7))
    d, pe = run_prover(hal, [(3, right, comps_r, None), (6, shifts, comps_s, None), (6, packed, comps_p, None)], pool, 0xDB300)
    # two of the three suffixes carry combinations: two calls of the new op, 5 + 2 jobs of five terms in one class each
    assert d == {"calls": 2, "launches": 4, "jobs": 7, "terms": 35, "classes": 7, "jobs_fallback": 0}
    assert pe["calls"] == 3 and pe["cols_kernel"] == 6 + 1 + 3


def test_prover_two_level_combination_with_offset_at_twelve_variables(hal):
    import oracle

    pool = oracle.random_scalars(0xDC000, 19)  # [0:12) r, [12:16) the suffix, [16:19) a second one
    bits, bytes_ = random_column(0xDC100, 0, 16), random_column(0xDC101, 3, 16)
    terms = [(bits, 0, GENERATOR), (bytes_, 3, 1), (bits, 0, 1)]
    small = [(random_column(0xDC102, 0, 15), 0, 1), (random_column(0xDC103, 3, 15), 3, A.ALL_ONES)]
    mls = [("lincomb", terms, 0x5A << 120, 16, 12, 4), ("shift", 12, 77, R.LOGICAL_LEFT, 0, 12), ("lincomb", terms, 0x5A << 120, 16, 12, 4),
           ("lincomb", terms, 0, 16, 12, 4), ("lincomb", small, 9, 15, 16, 3)]
    d, pe = run_prover(hal, [(12, mls, [(0, 1), (2, 1), (3, 1), (4, 1)], None)], pool, 0xDC200)
    # one call per distinct suffix; the identical (terms, offset, suffix) once; 4096 outputs each: the one-thread-per-output form, and
    # that launch alone
    assert d == {"calls": 2, "launches": 2, "jobs": 3, "terms": 3 + 3 + 2, "classes": 3 + 3 + 2, "jobs_fallback": 3}
    assert pe["calls"] == 0


def test_prover_without_combinations_leaves_the_new_op_alone(hal):
    import oracle

    pool = oracle.random_scalars(0xDD000, 15)
    cols = [random_column(0xDD100 + t, 0, 15) for t in range(4)]
    mls, comps = [], []
    for col in cols:
        comps.append((len(mls), len(mls) + 1))
        mls += [("proj", col, 0, 15, 5, 10), ("shift", 5, 1, R.LOGICAL_LEFT, 0, 5)]
    d, pe = run_prover(hal, [(5, mls, comps, None)], pool, 0xDD200)
    assert d == PEL_ZERO
    assert pe["calls"] == 1 and pe["cols_kernel"] == 4


def test_plain_entry_rejects_a_combination(hal):
    import ctypes as C

    import oracle
    from binius_amd._ffi import BnError
    from binius_amd._host import EvalcheckPlan

    pool = oracle.random_scalars(0xDE000, 13)
    alloc = hal.dev_alloc()
    col = alloc.alloc(1 << 6)
    hal.fill(col, 0)
    dev = [(6, [("lincomb", [(col, 0, 1)], 0, 13, 6, 7), ("shift", 6, 1, 0, 0, 6)], [(0, 1)], [0])]
    plan = EvalcheckPlan(hal, dev, pool, alloc.alloc(EvalcheckPlan.scratch_elems(dev)), [1], oracle.random_scalars(1, 6))
    plan.run()
    plan.has_lincomb = False  # kind 3 through bnh_evalcheck_bivariate_prove
    with pytest.raises(BnError):
        plan.run()
