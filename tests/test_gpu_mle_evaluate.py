"""GPU parity of the evaluations in front of an evalcheck round: bn_mle_evaluate_batch (binius_amd/csrc/kernels_mle_eval.hip +
abi_mle_eval.cpp; reference: the first step of EvalcheckProver::prove, evalcheck/prove.rs:191-275, 812-879) against oracle.mle_evaluate of
the widened column, and bnh_evalcheck_evaluate (evalcheck_evaluate_claims of binius_amd/host/evalcheck.hpp) against the same.  Everything
is bit-exact and nothing is compared with the op's own output.  Columns and tables sit between canary frames at bases that are odd
multiples of 16 bytes and are read back after the call: inputs are only read.  One context per module."""
import ctypes as C
import functools

import numpy as np
import pytest

import adversarial as A
import evalcheck_ref as R

pytestmark = pytest.mark.gpu

ARENA_ELEMS = 1 << 22
LEVELS = (0, 3, 4, 5, 6, 7)


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
def random_point(seed, n):
    import oracle

    return tuple(oracle.random_scalars(seed, n))


def expected(col, level, n_vars, coords):
    import oracle

    return oracle.mle_evaluate(R.widen(col, level, n_vars), n_vars, list(coords))


def me_delta(hal, before):
    now = hal.mle_evaluate_counters()
    return {k: now[k] - before[k] for k in now if k != "max_share"}, now["max_share"]


class Batch:
    """points: [(coords, lo_vars)]; jobs: [(packed array, tower_level, n_vars, point index)].  Everything is placed between canary frames;
    run() is one bn_mle_evaluate_batch; check_inputs() reads every column and table back."""

    def __init__(self, hal, points, jobs, alloc=None):
        self.hal = hal
        alloc = alloc or hal.dev_alloc()
        self.checks, self.d_points, self.d_jobs, lead = [], [], [], 1
        placed = {}
        for coords, lo in points:
            d_lo, chk_lo = A.place(hal, alloc, R.eq_expand(list(coords[:lo])), lead)
            d_hi, chk_hi = A.place(hal, alloc, R.eq_expand(list(coords[lo:])), lead + 2)
            lead += 4
            self.checks += [chk_lo, chk_hi]
            self.d_points.append((d_lo, lo, d_hi, len(coords) - lo))
        for col, level, n_vars, pt in jobs:
            if id(col) not in placed:  # (one column used by several jobs is one device array)
                placed[id(col)], chk = A.place(hal, alloc, col, lead)
                lead += 2
                self.checks.append(chk)
            self.d_jobs.append((placed[id(col)], level, n_vars, pt))
        self.wants = [expected(col, level, n_vars, points[pt][0]) for col, level, n_vars, pt in jobs]

    def run(self):
        return self.hal.mle_evaluate_batch(self.d_jobs, self.d_points)

    def check_inputs(self):
        for chk in self.checks:
            chk()


ONE_JOB = (
    [(0, lo, hi) for lo, hi in ((7, 0), (0, 7), (3, 4), (5, 9), (6, 6), (7, 7), (10, 0), (10, 8))]
    + [(3, 2, 2), (3, 4, 8), (4, 3, 0), (4, 5, 6), (5, 2, 0), (5, 6, 8), (6, 1, 0), (6, 0, 9), (7, 0, 0), (7, 1, 0), (7, 5, 7)]
)


@pytest.mark.parametrize("level,lo,hi", ONE_JOB)
def test_one_job(hal, level, lo, hi):
    n_vars = lo + hi
    col = random_column(0xF1000 + 64 * n_vars + level, level, n_vars)
    b = Batch(hal, [(random_point(0xF1100 + 32 * lo + hi, n_vars), lo)], [(col, level, n_vars, 0)])
    before = hal.mle_evaluate_counters()
    got = b.run()
    d, share = me_delta(hal, before)
    assert got == b.wants
    assert d["calls"] == 1 and d["jobs"] == 1 and 1 <= d["launches"] <= 3
    if (level, lo, hi) == (0, 10, 8):
        assert share > 1  # 256 rows of 1024 bits: several workgroups share the column and are XOR-combined
    if hi == 0:
        assert share == 1
    b.check_inputs()


@pytest.mark.parametrize("level", LEVELS)
def test_equals_inner_product_with_the_full_expansion(hal, level):
    n_vars = 12
    col = random_column(0xF2000 + level, level, n_vars)
    coords = random_point(0xF2100 + level, n_vars)
    b = Batch(hal, [(coords, 5)], [(col, level, n_vars, 0)])
    got = b.run()
    alloc = hal.dev_alloc()
    d_col = alloc.alloc(col.shape[0])
    hal.copy_h2d(col, d_col)
    full = alloc.alloc(1 << n_vars)
    hal.fill(full, 0)
    hal.fill(full.slice(0, 1), 1)
    hal.tensor_expand(0, list(coords), full)
    assert got == [hal.inner_product(d_col, level, full)]
    assert got == b.wants


def mixed_batch():
    """24 jobs over all six levels at three points: A has 7 variables split (3, 4), B and C have 16 variables split (10, 6) and (5, 11).
    Jobs 0 and 1 are identical; the column of job 2 is also used at point C (job 3)."""
    points = [(random_point(0xF3001, 7), 3), (random_point(0xF3002, 16), 10), (random_point(0xF3003, 16), 5)]
    shared = random_column(0xF3100, 0, 16)
    twice = random_column(0xF3101, 5, 16)
    jobs = [(shared, 0, 16, 1), (shared, 0, 16, 1), (twice, 5, 16, 1), (twice, 5, 16, 2)]
    for t in range(20):
        level = LEVELS[t % 6]
        pt = (0, 1, 2, 1, 0, 2, 2)[t % 7]
        n_vars = 7 if pt == 0 else 16
        jobs.append((random_column(0xF3200 + t, level, n_vars), level, n_vars, pt))
    return points, jobs


def test_mixed_batch(hal):
    one = Batch(hal, [(random_point(0xF3004, 9), 4)], [(random_column(0xF3300, 0, 9), 0, 9, 0)])
    before = hal.mle_evaluate_counters()
    assert one.run() == one.wants
    one_job, _ = me_delta(hal, before)
    points, jobs = mixed_batch()
    assert len(jobs) == 24 and {j[1] for j in jobs} == set(LEVELS) and {j[3] for j in jobs} == {0, 1, 2}
    b = Batch(hal, points, jobs)
    before, pe_before = hal.mle_evaluate_counters(), hal.partial_eval_counters()
    got = b.run()
    d, _ = me_delta(hal, before)
    for t, (g, w) in enumerate(zip(got, b.wants)):
        assert g == w, "job %d (level %d, n_vars %d, point %d)" % (t, jobs[t][1], jobs[t][2], jobs[t][3])
    assert got[0] == got[1]
    assert d == {"calls": 1, "launches": one_job["launches"], "jobs": 24}
    assert one_job["launches"] <= 3
    assert hal.partial_eval_counters() == pe_before
    b.check_inputs()


def one_hot(level, n_vars, x):
    """The column whose value at index x is 1 and that is zero elsewhere: a single set bit."""
    import oracle

    col = oracle.arr(1 << (n_vars + level - 7))
    bit = x << level
    col[bit // 128, (bit % 128) // 64] = np.uint64(1) << np.uint64(bit % 64)
    return col


@pytest.mark.parametrize("level,lo,hi", [(0, 6, 6), (0, 3, 9), (5, 4, 6)])
def test_adversarial_columns(hal, level, lo, hi):
    import oracle
    from binius_amd._ffi import HostField

    n_vars, last = lo + hi, (1 << (lo + hi)) - 1
    n = 1 << (n_vars + level - 7)
    zeros, ones = oracle.arr(n), np.full((n, 2), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    first_bit, last_bit = one_hot(level, n_vars, 0), one_hot(level, n_vars, last)
    rnd = random_column(0xF4000 + level, level, n_vars)
    coords = random_point(0xF4100 + 16 * lo + level, n_vars)
    vertex = tuple((0xB5A7 >> k) & 1 for k in range(n_vars))
    x_vertex = sum(c << k for k, c in enumerate(vertex))
    points = [(coords, lo), (vertex, lo), ((0,) * n_vars, lo)]
    jobs = [(zeros, level, n_vars, 0), (ones, level, n_vars, 0), (first_bit, level, n_vars, 0), (last_bit, level, n_vars, 0), (rnd, level, n_vars, 1),
            (rnd, level, n_vars, 2), (ones, level, n_vars, 1)]
    b = Batch(hal, points, jobs)
    got = b.run()
    assert got == b.wants
    assert got[0] == 0
    lo_tab, hi_tab = oracle.arr_to_ints(R.eq_expand(list(coords[:lo]))), oracle.arr_to_ints(R.eq_expand(list(coords[lo:])))
    assert got[2] == HostField.mul(lo_tab[0], hi_tab[0])
    assert got[3] == HostField.mul(lo_tab[last & ((1 << lo) - 1)], hi_tab[last >> lo])
    wide = oracle.arr_to_ints(R.widen(rnd, level, n_vars))
    assert got[4] == wide[x_vertex] and got[5] == wide[0]
    assert got[6] == (1 << (1 << level)) - 1
    b.check_inputs()


def test_inputs_are_only_read_and_no_state_is_left(hal):
    points, jobs = mixed_batch()
    b = Batch(hal, points, jobs[:8])
    first = b.run()
    b.check_inputs()
    assert first == b.wants
    assert b.run() == first
    # the shared result area is left as the other ops expect it
    import oracle

    col = random_column(0xF5000, 5, 12)
    vec = R.eq_expand(list(random_point(0xF5001, 12)))
    alloc = hal.dev_alloc()
    d_col, d_vec = alloc.alloc(col.shape[0]), alloc.alloc(vec.shape[0])
    hal.copy_h2d(col, d_col)
    hal.copy_h2d(vec, d_vec)
    b2 = Batch(hal, [(random_point(0xF5002, 10), 5)], [(random_column(0xF5003, 0, 10), 0, 10, 0)], alloc)
    want_ip = oracle.inner_product(np.ascontiguousarray(col), 5, vec)
    assert want_ip[0] == 0
    assert b2.run() == b2.wants
    assert hal.inner_product(d_col, 5, d_vec) == want_ip[1]


def raw_call(hal, jobs, points, n_jobs=None, n_points=None, null_out=False):
    """bn_mle_evaluate_batch with every field spelled out: jobs (ptr, level, n_vars, point, reserved), points (lo ptr, hi ptr, lo_vars, hi_vars)."""
    from binius_amd import _ffi as f

    table = (f.MeJob * max(1, len(jobs)))(*[f.MeJob(*jb) for jb in jobs])
    pts = (f.MePoint * max(1, len(points)))(*[f.MePoint(*pt) for pt in points])
    out = (f.F128 * max(1, len(jobs)))()
    rc = f.lib().bn_mle_evaluate_batch(hal._h, C.cast(table, C.c_void_p), len(jobs) if n_jobs is None else n_jobs, C.cast(pts, C.c_void_p),
                                       len(points) if n_points is None else n_points, None if null_out else out)
    return rc, [f.from_f128(out[j]) for j in range(len(jobs))]


def test_validation(hal):
    from binius_amd import _ffi as f

    good = Batch(hal, [(random_point(0xF6000, 12), 6), (random_point(0xF6001, 22), 10)], [(random_column(0xF6100, 0, 12), 0, 12, 0)])
    (d_lo, lo, d_hi, hi), (e_lo, _, e_hi, _) = good.d_points
    col = good.d_jobs[0][0]
    pt = (d_lo.ptr, d_hi.ptr, lo, hi)
    job = (col.ptr, 0, 12, 0, 0)
    rc, vals = raw_call(hal, [job], [pt])
    assert rc == 0 and vals == good.wants
    max_jobs = f.BN_ME_MAX_JOBS
    assert max_jobs >= 1024
    bad = {
        "lo_vars = 11": dict(jobs=[(col.ptr, 0, 22, 0, 0)], points=[(e_lo.ptr, e_hi.ptr, 11, 11)]),
        "lo_vars + hi_vars != n_vars": dict(jobs=[(col.ptr, 0, 13, 0, 0)], points=[pt]),
        "level 1": dict(jobs=[(col.ptr, 1, 12, 0, 0)], points=[pt]),
        "level 2": dict(jobs=[(col.ptr, 2, 12, 0, 0)], points=[pt]),
        "n_vars + level < 7": dict(jobs=[(col.ptr, 0, 6, 0, 0)], points=[(d_lo.ptr, d_hi.ptr, 3, 3)]),
        "a misaligned column": dict(jobs=[(col.ptr + 8, 0, 12, 0, 0)], points=[pt]),
        "point >= n_points": dict(jobs=[(col.ptr, 0, 12, 1, 0)], points=[pt]),
        "reserved != 0": dict(jobs=[(col.ptr, 0, 12, 0, 1)], points=[pt]),
        "n_jobs > BN_ME_MAX_JOBS": dict(jobs=[job] * (max_jobs + 1), points=[pt]),
        "null h_out": dict(jobs=[job], points=[pt], null_out=True),
    }
    for name, kw in bad.items():
        before = hal.mle_evaluate_counters()
        rc, _ = raw_call(hal, **kw)
        assert rc == f.BN_ERR_INPUT_VALIDATION, name
        assert hal.mle_evaluate_counters() == before, name
        assert good.run() == good.wants, "a valid call after: " + name
    # n_jobs = 0 is a no-op
    before = hal.mle_evaluate_counters()
    assert raw_call(hal, [], [], n_jobs=0, n_points=0)[0] == 0
    assert hal.mle_evaluate_counters() == before
    good.check_inputs()


def test_host_mirror(hal):
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION, BnError
    from binius_amd._host import EvalcheckEvaluatePlan

    # pool: point 1 = [0, 12); point 3 = [12, 22), split (5, 5); point 2 = [13, 22), split (4, 5): the suffix slice [17, 22) is shared;
    # point 4 = [22, 29)
    pool = list(random_point(0xF7000, 29))
    specs = [(random_column(0xF7100 + t, 0, 12), 0, 12, 0, 12) for t in range(24)]
    specs += [(random_column(0xF7200 + t, 5, 9), 5, 9, 13, 9) for t in range(3)]
    specs.append((random_column(0xF7300, 3, 10), 3, 10, 12, 10))
    specs.append((random_column(0xF7301, 0, 7), 0, 7, 22, 7))
    specs.append(specs[25])  # a duplicate claim
    distinct = len(specs) - 1
    alloc = hal.dev_alloc()
    placed, claims, checks, lead = {}, [], [], 1
    for col, level, n_vars, off, ln in specs:
        if id(col) not in placed:
            placed[id(col)], chk = A.place(hal, alloc, col, lead)
            lead += 2
            checks.append(chk)
        claims.append((placed[id(col)], level, n_vars, off, ln))
    need = EvalcheckEvaluatePlan.scratch_elems(claims)
    assert need == (64 + 32 + 16 + 8) + (64 + 32 + 16)
    scratch = alloc.alloc(need)
    wants = [expected(col, level, n_vars, pool[off : off + ln]) for col, level, n_vars, off, ln in specs]

    short = EvalcheckEvaluatePlan(hal, claims, pool, scratch.slice(0, need - 1))
    before = hal.mle_evaluate_counters()
    with pytest.raises(BnError) as e:
        short.run()
    assert e.value.code == BN_ERR_INPUT_VALIDATION
    assert hal.mle_evaluate_counters() == before

    plan = EvalcheckEvaluatePlan(hal, claims, pool, scratch)
    plan.run()
    d, _ = me_delta(hal, before)
    got = plan.evals()
    for t, (g, w) in enumerate(zip(got, wants)):
        assert g == w, "claim %d (level %d, n_vars %d)" % (t, specs[t][1], specs[t][2])
    assert d["calls"] == 1 and d["jobs"] == distinct
    for chk in checks:
        chk()
