"""The CPU restatement of the ring-switching reduction (tests/ring_switch_ref.py; ring_switch::prove, core/src/ring_switch/prove.rs:42-144)
pinned by the verifier's equations and by the claim the phase hands to the PIOP, with evaluations that share nothing with prove():

  1. the MLE of each prefix's mixed tensor element's vertical elements at the prefix = sum of mixing_coeff_i * eval_i over the prefix's
     claims (verify.rs:100-139), eval_i the MLE of the column widened to B128 at the whole point
  2. fold_vertical(mixed, coeffs) = sum of row_batched_evals over the prefix's claims (verify.rs:63-72)
  3. row_batched_evals[i] = sum_x packed_i[x] * transparent_i[x], packed_i the committed column read as 2^(n_vars - kappa) B128 elements:
     the sum piop::prove is handed

Shape: seven claims over four columns at levels {0, 3, 5, 7}, 9 to 11 variables (ring_switch_ref.seven_claim_case): two suffixes at
kappa 7, 4 and 0 and one at kappa 2 (seven claims cannot give each of four kappas two), two prefixes that share kappa 7, and two
prefixes that mix two claims each."""
import numpy as np
import pytest

import ring_switch_ref as R


@pytest.fixture(scope="module")
def case(oracle):
    c = R.seven_claim_case()
    return c, R.prove(c)


def test_the_shape(case):
    c, _ = case
    assert len(c["claims"]) == 7 and len(c["columns"]) == 4
    assert sorted(level for _a, level, _n in c["columns"]) == [0, 3, 5, 7]
    assert {n for _a, _l, n in c["columns"]} == {9, 10, 11}
    kappas = [k for _off, k in c["prefixes"]]
    assert kappas.count(7) == 2  # two prefixes that share a kappa
    by_prefix = [sum(1 for cl in c["claims"] if cl[2] == p) for p in range(len(c["prefixes"]))]
    assert max(by_prefix) == 2 and min(by_prefix) == 1  # mixed and unmixed prefixes


def test_equation_1_mixed_elements_against_independent_evaluations(oracle, case):
    c, out = case
    want = [0] * len(c["prefixes"])
    for i, (ci, si, pi) in enumerate(c["claims"]):
        col, level, n_vars = c["columns"][ci]
        off, ln, kappa = c["suffixes"][si]
        p_off = c["prefixes"][pi][0]
        point = c["pool"][p_off : p_off + kappa] + c["pool"][off : off + ln]
        wide = oracle.arr(1 << n_vars)  # the column widened to B128: fold_left against the one-element query ONE
        assert oracle.fold_left(np.ascontiguousarray(col), level, oracle.ints_to_arr([1]), wide) == 0
        want[pi] ^= oracle.mul(out["mixing_coeffs"][i], oracle.mle_evaluate(wide, n_vars, point))
    for pi, (p_off, kappa) in enumerate(c["prefixes"]):
        got = oracle.mle_evaluate(oracle.ints_to_arr(out["mixed"][pi]), kappa, c["pool"][p_off : p_off + kappa])
        assert got == want[pi], "prefix %d" % pi


def test_equation_2_fold_vertical_of_the_mixed_elements(oracle, case):
    c, out = case
    for pi, (_off, kappa) in enumerate(c["prefixes"]):
        want = 0
        for i, cl in enumerate(c["claims"]):
            if cl[2] == pi:
                want ^= out["row_batched_evals"][i]
        assert R.fold_vertical(out["mixed"][pi], kappa, out["row_coeffs"]) == want, "prefix %d" % pi


def test_equation_3_the_sum_the_piop_is_handed(oracle, case):
    c, out = case
    for i, (ci, si, _pi) in enumerate(c["claims"]):
        col = c["columns"][ci][0]
        t = out["transparents"][i]
        assert t.shape[0] == col.shape[0] == 1 << c["suffixes"][si][1]
        rc, got = oracle.inner_product(np.ascontiguousarray(col), 7, t)
        assert rc == 0 and got == out["row_batched_evals"][i], "claim %d" % i


def test_transparent_is_the_linear_map_of_the_query(oracle, case):
    """out[x] = sum_i coeffs[i] * limb_i(mixing_coeff * query[x]): the closed form the device op is specified by."""
    c, out = case
    for i, (_ci, si, _pi) in enumerate(c["claims"]):
        off, ln, kappa = c["suffixes"][si]
        query = oracle.arr_to_ints(R.eq_expand(c["pool"][off : off + ln]))
        got = oracle.arr_to_ints(out["transparents"][i])
        for x in (0, 1, len(query) // 2, len(query) - 1):
            e = oracle.mul(out["mixing_coeffs"][i], query[x])
            want = 0
            for j in range(1 << kappa):
                want ^= oracle.mul(out["row_coeffs"][j], R.limb(e, j, kappa))
            assert got[x] == want, "claim %d element %d" % (i, x)


def test_transparent_from_the_table_equals_the_sequence(oracle, case):
    """eq_ind_from_query (what the GPU tests of the op compare with, for tables that are no tensor expansion as well) against eq_ind."""
    c, out = case
    for i, (_ci, si, _pi) in enumerate(c["claims"]):
        off, ln, kappa = c["suffixes"][si]
        got = R.eq_ind_from_query(R.eq_expand(c["pool"][off : off + ln]), kappa, out["mixing_coeffs"][i], out["row_coeffs"])
        assert np.array_equal(got, out["transparents"][i]), "claim %d" % i


def test_kappa_mismatch_inside_a_prefix_is_rejected(oracle):
    c = R.seven_claim_case()
    ci, si, pi = c["claims"][2]
    c["claims"][2] = (ci, si, 0)  # a byte column's claim under a bit column's prefix
    with pytest.raises(ValueError, match="TowerLevelMismatch"):
        R.prove(c)
