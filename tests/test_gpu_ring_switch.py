"""GPU parity of the batched ring-switch equality indicator (bn_ring_switch_eq_ind_batch: binius_amd/csrc/kernels_ring_switch.hip +
abi_ring_switch.cpp; reference: RingSwitchEqInd, ring_switch/eq_ind.rs:81-147) against the CPU restatement (tests/ring_switch_ref.py,
pinned by tests/test_ring_switch_oracle.py).  Everything is bit-exact and nothing is compared with the device's own output, except where
a test says that the op ALSO equals the per-claim RingSwitchEqInd sequence on the device (fill, tensor_expand, fold_right).  Outputs lie
between canary frames at odd 16-byte bases and hold the canary before the call, so a result also pins that they are overwritten, not
accumulated, and that nothing is written beyond 2^n_vars elements.  Every case runs twice from resident inputs and must give the same
values.  One context per module."""
import numpy as np
import pytest

import adversarial as A
import ring_switch_ref as R

pytestmark = pytest.mark.gpu

KAPPAS = (0, 1, 2, 3, 4, 7)


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, 1 << 23)
    yield ctx
    ctx.close()


def delta(hal, before):
    now = hal.ring_switch_counters()
    return {k: now[k] - before[k] for k in now}


def run_batch(oracle, hal, queries, jobs, coeffs, also_sequence=False):
    """queries: [(table, suffix or None)], the table an (2^n, 2) array (the expansion of the suffix where there is one); jobs: [(query
    index, kappa, mixing coefficient)].  One call for all jobs; every output against the restatement, frames intact, queries unchanged.
    Returns the counter deltas of the first call."""
    alloc = hal.dev_alloc()
    d_q, q_checks = [], []
    for t, (table, _suffix) in enumerate(queries):
        s, chk = A.place(hal, alloc, table, 2 * t + 1)
        d_q.append(s)
        q_checks.append(chk)
    d_jobs, d_outs, out_checks, wants = [], [], [], []
    for j, (qi, kappa, mix) in enumerate(jobs):
        table = queries[qi][0]
        n_vars = table.shape[0].bit_length() - 1
        o, ochk = A.place(hal, alloc, table.shape[0], 2 * j + 9)
        d_jobs.append((d_q[qi], n_vars, kappa, mix))
        d_outs.append(o)
        out_checks.append(ochk)
        wants.append(R.eq_ind_from_query(table, kappa, mix, coeffs))
    got = None
    for _ in range(2):  # resident inputs, run twice: the same values
        before = hal.ring_switch_counters()
        hal.ring_switch_eq_ind_batch(d_jobs, coeffs, d_outs)
        got = got or delta(hal, before)
        for j, (ochk, want) in enumerate(zip(out_checks, wants)):
            try:
                ochk(want)
            except AssertionError as e:
                raise AssertionError("job %d (query %d, n_vars %d, kappa %d): %s" % (j, jobs[j][0], d_jobs[j][1], jobs[j][1], e))
        for chk in q_checks:
            chk()
    if also_sequence:
        d_c = alloc.alloc(len(coeffs))
        hal.copy_h2d(oracle.ints_to_arr(list(coeffs)), d_c)
        n_max = max(q[0].shape[0] for q in queries)
        evals, single = alloc.alloc(n_max), alloc.alloc(n_max)
        for j, (qi, kappa, mix) in enumerate(jobs):
            suffix = queries[qi][1]
            assert suffix is not None
            e, o = evals.slice(0, 1 << len(suffix)), single.slice(0, 1 << len(suffix))
            hal.fill(e, 0)
            hal.fill(e.slice(0, 1), mix)
            hal.tensor_expand(0, suffix, e)
            hal.fill(o, A.CANARY)
            hal.fold_right(e, 7 - kappa, d_c.slice(0, 1 << kappa), o)
            assert np.array_equal(hal.copy_d2h(o), wants[j]), "the per-claim sequence differs (job %d, kappa %d)" % (j, kappa)
    return got


def suffix_query(oracle, seed, n_vars):
    suffix = oracle.random_scalars(seed, n_vars)
    return R.eq_expand(suffix), suffix


@pytest.mark.parametrize("kappa", KAPPAS)
def test_one_job_vs_restatement(oracle, hal, kappa):
    """A workgroup's tile is 2^11 elements: n_vars = 11 fills one exactly, 12 is one tile past it, 14 well past (eight units)."""
    coeffs = oracle.random_scalars(0x4500 + kappa, 128)
    for n_vars in (0, 1, 6, 11, 12, 14):
        mix = oracle.random_scalars(0x4600 + 16 * n_vars + kappa, 1)[0]
        d = run_batch(oracle, hal, [suffix_query(oracle, 0x4700 + 16 * n_vars + kappa, n_vars)], [(0, kappa, mix)], coeffs)
        assert d == {"calls": 1, "launches": 1, "jobs": 1, "queries": 1}, n_vars


def test_fewer_coefficients_than_128(oracle, hal):
    """n_coeffs = 2^kappa exactly, below the 128 a workgroup stages."""
    for kappa in (0, 2, 4):
        coeffs = oracle.random_scalars(0x4400 + kappa, 1 << kappa)
        run_batch(oracle, hal, [suffix_query(oracle, 0x4410 + kappa, 7)], [(0, kappa, oracle.random_scalars(0x4420 + kappa, 1)[0])], coeffs)


def test_many_jobs_over_one_query(oracle, hal):
    """37 jobs over ONE query at n_vars = 12, more than the eight tables a workgroup holds, with mixed kappa: one launch; equal to the
    per-claim sequence on the device as well."""
    coeffs = oracle.random_scalars(0x4300, 128)
    mixes = oracle.random_scalars(0x4301, 37)
    jobs = [(0, KAPPAS[(5 * t) % 6], mixes[t]) for t in range(37)]
    assert {k for _q, k, _m in jobs} == set(KAPPAS)
    d = run_batch(oracle, hal, [suffix_query(oracle, 0x4302, 12)], jobs, coeffs, also_sequence=True)
    assert d == {"calls": 1, "launches": 1, "jobs": 37, "queries": 1}


def test_mixed_queries_one_launch(oracle, hal):
    """23 jobs over four queries of four sizes with interleaved kappa."""
    coeffs = oracle.random_scalars(0x4200, 128)
    queries = [suffix_query(oracle, 0x4210 + t, n) for t, n in enumerate((0, 5, 10, 14))]
    mixes = oracle.random_scalars(0x4201, 23)
    jobs = [(t % 4, KAPPAS[t % 6], mixes[t]) for t in range(23)]
    d = run_batch(oracle, hal, queries, jobs, coeffs, also_sequence=True)
    assert d == {"calls": 1, "launches": 1, "jobs": 23, "queries": 4}


def test_units_of_several_tiles(oracle, hal):
    """128 one-job runs of 16 tiles each (queries that overlap each other inside one buffer: they are only read): 2048 tiles, at which a
    workgroup of a 256-CU device takes two tiles through its tables."""
    coeffs = oracle.random_scalars(0x4100, 128)
    n = 1 << 15
    buf = oracle.random_b128(0x4101, n + 128)
    mixes = oracle.random_scalars(0x4102, 128)
    alloc = hal.dev_alloc()
    d_buf, chk = A.place(hal, alloc, buf, 3)
    outs = alloc.alloc(128 * n + 2 * A.FRAME)
    hal.fill(outs, A.CANARY)
    jobs = [(d_buf.slice(t, t + n), 15, KAPPAS[t % 6], mixes[t]) for t in range(128)]
    d_outs = [outs.slice(A.FRAME + t * n, A.FRAME + (t + 1) * n) for t in range(128)]
    before = hal.ring_switch_counters()
    hal.ring_switch_eq_ind_batch(jobs, coeffs, d_outs)
    assert delta(hal, before) == {"calls": 1, "launches": 1, "jobs": 128, "queries": 128}
    got = hal.copy_d2h(outs)
    frame = np.tile(oracle.ints_to_arr([A.CANARY]), (A.FRAME, 1))
    assert np.array_equal(got[: A.FRAME], frame) and np.array_equal(got[-A.FRAME :], frame)
    for t in range(128):
        want = R.eq_ind_from_query(buf[t : t + n], KAPPAS[t % 6], mixes[t], coeffs)
        assert np.array_equal(got[A.FRAME + t * n : A.FRAME + (t + 1) * n], want), "job %d" % t
    chk()


@pytest.mark.parametrize("what", ["mix_zero", "mix_one", "mix_ones", "coeffs_zero", "coeffs_ones", "coeffs_single", "query_ones"])
def test_extreme_operands(oracle, hal, what):
    coeffs = {"coeffs_zero": [0] * 128, "coeffs_ones": [A.ALL_ONES] * 128,
              "coeffs_single": [0] * 77 + [oracle.random_scalars(0x4001, 1)[0]] + [0] * 50}.get(what, oracle.random_scalars(0x4002, 128))
    if what == "coeffs_single":
        coeffs[5] = coeffs[77]  # (an entry every kappa >= 3 reads as well)
    mix = {"mix_zero": 0, "mix_one": 1, "mix_ones": A.ALL_ONES}.get(what, oracle.random_scalars(0x4003, 1)[0])
    table = np.tile(oracle.ints_to_arr([A.ALL_ONES]), (1 << 12, 1)) if what == "query_ones" else suffix_query(oracle, 0x4004, 12)[0]
    run_batch(oracle, hal, [(table, None)], [(0, kappa, mix) for kappa in KAPPAS], coeffs)


def test_no_jobs_is_a_no_op(hal):
    before = hal.ring_switch_counters()
    hal.ring_switch_eq_ind_batch([], [0] * 128, [])
    assert delta(hal, before) == {"calls": 0, "launches": 0, "jobs": 0, "queries": 0}


def test_validation_errors(oracle, hal):
    import binius_amd
    from binius_amd._ffi import DevSlice

    alloc = hal.dev_alloc()
    n_vars, kappa = 10, 4
    coeffs = oracle.random_scalars(0x3F00, 16)
    table, _ = suffix_query(oracle, 0x3F01, n_vars)
    mix = oracle.random_scalars(0x3F02, 1)[0]
    q = alloc.alloc(1 << n_vars)
    hal.copy_h2d(table, q)
    out, out2 = alloc.alloc(1 << n_vars), alloc.alloc(1 << n_vars)
    hal.fill(out, A.CANARY)
    hal.fill(out2, A.CANARY)
    # the valid call first: the cases below differ from it in one argument each
    hal.ring_switch_eq_ind_batch([(q, n_vars, kappa, mix)], coeffs, [out])
    want = hal.copy_d2h(out)
    assert np.array_equal(want, R.eq_ind_from_query(table, kappa, mix, coeffs))
    before = hal.ring_switch_counters()
    n = 1 << n_vars
    cases = [
        ([(q, n_vars, 5, mix)], coeffs * 2, [out]),                                              # kappa 5
        ([(q, n_vars, 6, mix)], coeffs * 4, [out]),                                              # kappa 6
        ([(q, n_vars, 8, mix)], coeffs * 16, [out]),                                             # kappa above 7
        ([(q, n_vars, 7, mix)], coeffs, [out]),                                                  # fewer coefficients than 2^kappa
        ([(q, n_vars, kappa, mix)], coeffs + coeffs[:8], [out]),                                 # not a power of two of coefficients
        ([(None, n_vars, kappa, mix)], coeffs, [out]),                                           # a null query
        ([(q, n_vars, kappa, mix)], coeffs, [None]),                                             # a null output
        ([(DevSlice(q.ptr + 8, n), n_vars, kappa, mix)], coeffs, [out]),                         # a misaligned query
        ([(q, n_vars, kappa, mix)], coeffs, [DevSlice(out.ptr + 4, n)]),                         # a misaligned output
        ([(q, n_vars, kappa, mix)], coeffs, [DevSlice(q.ptr + 16 * (n - 1), n)]),                # the output overlaps its query
        ([(q, n_vars, kappa, mix)] * 2, coeffs, [out, DevSlice(out.ptr + 16 * (n - 1), n)]),     # an output overlaps another output
        ([(q, n_vars, kappa, mix), (out2, n_vars, kappa, mix)], coeffs, [out, out2]),            # an output is another job's query
        ([(q, n_vars, kappa, mix)], coeffs, [DevSlice(out.ptr, n // 2)]),                        # an output of the wrong length
        ([(q, n_vars, kappa, mix)] * 2, coeffs, [out]),                                          # not one output per job
    ]
    for args in cases:
        with pytest.raises(binius_amd.BnError) as e:
            hal.ring_switch_eq_ind_batch(*args)
        assert e.value.kind == "InputValidation", args
    assert delta(hal, before) == {"calls": 0, "launches": 0, "jobs": 0, "queries": 0}
    assert np.array_equal(hal.copy_d2h(out), want)  # nothing was launched
    assert np.array_equal(hal.copy_d2h(out2), np.tile(oracle.ints_to_arr([A.CANARY]), (n, 1)))
