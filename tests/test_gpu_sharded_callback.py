"""The caller's reduce callback as the exchange of the sharded prover (bnh_bivariate_sumcheck_prove with `reduce`): every round
leaves this rank's {y_1, y_inf} on the device in d_partial and asks the callback for the world's.  One process, world 1, no
process group: the callback reads the two elements back (it runs between ABI calls on the calling thread, and the copy is
ordered on the context's stream after the round's kernels) and hands them over as they are, so the transcript must be the
unsharded oracle's and the plain compiled prover's, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def upload(hal, alloc, arr):
    d = alloc.alloc(arr.shape[0])
    hal.copy_h2d(arr, d)
    return d


def _instance(oracle, n_vars, m, comps):
    mls = [oracle.random_b128(0x5CA11000 + 32 * n_vars + j, 1 << n_vars) for j in range(m)]
    sums = [oracle.inner_product(mls[i], 7, mls[j])[1] for i, j in comps]
    stream = oracle.random_scalars(0xC4A1 + n_vars, n_vars + 1)
    return mls, sums, stream[0], stream[1:]


def _read_back(hal, partial, calls=None):
    """reduce callback of a world of one: the device partial IS the round's {y_1, y_inf}"""

    def cb(_user, d_partial, evals):
        got = hal.copy_d2h(partial)
        for i in range(2):
            evals[i].lo, evals[i].hi = int(got[i, 0]), int(got[i, 1])
        if calls is not None:
            calls.append(d_partial)  # (an assertion in here would be swallowed by ctypes: checked after run())
        return 0

    return cb


@pytest.mark.parametrize("n_vars,m,comps", [(2, 2, [(0, 1)]), (5, 3, [(0, 1), (2, 0)]), (10, 2, [(0, 1)])])
def test_callback_exchange_matches_oracle_and_plain_prover(oracle, n_vars, m, comps):
    import binius_amd
    from binius_amd._host import SumcheckPlan

    mls, sums, bc, ch = _instance(oracle, n_vars, m, comps)
    want = oracle.bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch, threads=4)
    with binius_amd.Context(0, (4 * m << n_vars) + 64) as hal:
        alloc = hal.dev_alloc()
        d_in = [upload(hal, alloc, x) for x in mls]
        scratch = alloc.alloc(m << (n_vars - 1))
        partial = alloc.alloc(2)
        calls = []
        plan = SumcheckPlan(hal, n_vars, d_in, scratch, comps, sums, bc, ch, reduce=_read_back(hal, partial, calls), d_partial=partial.ptr, world=1)
        plan.run()
        first = (plan.round_coeffs(), plan.final_evals())
        assert calls == [partial.ptr] * n_vars, "the callback is asked once a round, with the device address it was given"
        assert first[0] == want[0], "round polynomials differ from the oracle"
        assert first[1] == want[1], "final evaluations differ from the oracle"
        plain = SumcheckPlan(hal, n_vars, d_in, scratch, comps, sums, bc, ch)
        plain.run()
        assert (plain.round_coeffs(), plain.final_evals()) == first, "the plain compiled prover gives another transcript"
        plan.run()  # a second run from the same inputs: the prover must not have modified them
        assert (plan.round_coeffs(), plan.final_evals()) == first
        for j in range(m):
            assert np.array_equal(hal.copy_d2h(d_in[j]), mls[j])


def test_failing_callback_is_reported_and_leaves_the_context_usable(oracle):
    import binius_amd
    from binius_amd._host import BnError, SumcheckPlan

    n_vars, m, comps = 5, 2, [(0, 1)]
    mls, sums, bc, ch = _instance(oracle, n_vars, m, comps)
    want = oracle.bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch, threads=4)
    with binius_amd.Context(0, (4 * m << n_vars) + 64) as hal:
        alloc = hal.dev_alloc()
        d_in = [upload(hal, alloc, x) for x in mls]
        scratch = alloc.alloc(m << (n_vars - 1))
        partial = alloc.alloc(2)
        failing = SumcheckPlan(hal, n_vars, d_in, scratch, comps, sums, bc, ch, reduce=lambda _u, _p, _e: 1, d_partial=partial.ptr, world=1)
        with pytest.raises(BnError, match="round reduce callback failed"):
            failing.run()
        plain = SumcheckPlan(hal, n_vars, d_in, scratch, comps, sums, bc, ch)
        plain.run()
        assert plain.round_coeffs() == want[0] and plain.final_evals() == want[1]
