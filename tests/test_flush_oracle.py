"""Pins tests/flush_ref.py (CPU only), the restatement of the product-check phase that the GPU parity tests compare with
(constraint_system/prove.rs:276-428, 671-902, 1017-1117), independently of any device code: the balanced-channel property of the
witnesses, the composite identity row by row, the prefix rule against a brute-force search, and the whole prover output against
verifiers that share nothing with the prover (gkr_gpa_ref.gpa_verify, flush_ref.mlecheck_verify) and against independent
evaluations of the inner columns."""
import numpy as np
import pytest

import flush_ref as R
import gkr_gpa_ref as G


def rand_bits(o, seed, n):
    return (o.splitmix_words(seed, n) & np.uint64(1)).astype(np.uint8)


def test_balanced_channel_has_equal_products_until_a_row_changes(oracle):
    """One flush pushes rows, another pulls a permutation of the same rows through a different selector and with a different
    truncation: equal grand products for random alpha, r; unequal after one row is changed."""
    o = oracle
    n, live = 10, 300
    a, b = R.random_column(0xC0001, live, 5), R.random_column(0xC0002, live, 3)
    perm = np.argsort(o.splitmix_words(0xC0003, live), kind="stable")

    def table(rows_a, rows_b, slots):
        """The live rows scattered to `slots` of a 2^n table, the selector on exactly there, junk elsewhere."""
        sel = np.zeros(1 << n, dtype=np.uint8)
        sel[slots] = 1
        ca, cb = R.random_column(0xC0010, 1 << n, 5).copy(), R.random_column(0xC0011, 1 << n, 3).copy()
        ca[slots], cb[slots] = rows_a, rows_b
        return sel, ca, cb

    push_slots = np.arange(live)  # a dense prefix: truncated at 384
    pull_slots = np.sort(np.argsort(o.splitmix_words(0xC0004, 1 << n), kind="stable")[:live])  # scattered over the table
    alpha, r = o.random_scalars(0xC0005, 2)
    const_term, coeffs = R.mixing_terms([("oracle",), ("oracle",)], alpha, r)

    def grand_product(rows_a, rows_b, slots):
        sel, ca, cb = table(rows_a, rows_b, slots)
        prefix, wit = R.flush_witness(n, [sel], [(ca, 5, coeffs[0]), (cb, 3, coeffs[1])], const_term)
        assert not ((wit[:, 0] == 0) & (wit[:, 1] == 0)).any(), "a witness element is zero"
        return prefix, R.product(wit)

    p_push, push = grand_product(a, b, push_slots)
    p_pull, pull = grand_product(a[perm], b[perm], pull_slots)
    assert p_push == 384 and p_pull > p_push, "the two flushes are truncated differently"
    assert push == pull
    a2 = a.copy()
    a2[17] ^= np.uint64(1)
    assert grand_product(a2, b, push_slots)[1] != pull


@pytest.mark.parametrize("n_selectors", [1, 3])
def test_composite_identity_row_by_row(oracle, n_selectors):
    """w[i] = 1 + S[i] * (const_term + 1 + sum coeff_j col_j[i]) with S the product of the selector bits: the composite oracle of
    constraint_system/verify.rs:519-571 agrees with the masked witness on the hypercube (composite_steps through oracle.circuit_eval),
    tail beyond the prefix included."""
    o = oracle
    n = 6
    sels = [rand_bits(o, 0xC1000 + s, 1 << n) for s in range(n_selectors)]
    sels[0][40:] = 0
    levels = [0, 3, 5, 7]
    cols = [R.random_column(0xC1100 + l, 1 << n, l) for l in levels]
    coeffs, const_term = o.random_scalars(0xC1200, len(levels)), o.random_scalars(0xC1201, 1)[0]
    prefix, wit = R.flush_witness(n, sels, [(c, l, k) for c, l, k in zip(cols, levels, coeffs)], const_term)
    assert prefix == 64  # (one 16-byte element: no truncation below 128 rows)
    steps, _ = R.composite_steps(list(range(n_selectors)), list(range(n_selectors, n_selectors + len(levels))), coeffs, const_term)
    emb = [o.arr_to_ints(np.ascontiguousarray(R.embed(c, l))) for c, l in zip(cols, levels)]
    got = o.arr_to_ints(wit)
    for i in range(1 << n):
        assert got[i] == o.circuit_eval(steps, [int(s[i]) for s in sels] + [e[i] for e in emb]), "row %d" % i


@pytest.mark.parametrize("n_vars", [3, 7, 8, 12])
def test_prefix_rule_against_brute_force(oracle, n_vars):
    o = oracle
    rows = 1 << n_vars
    lasts = sorted({0, rows - 1, rows // 2, min(rows - 1, 127), min(rows - 1, 128), (3 * rows // 5) | 1})
    for last in lasts:
        sel = rand_bits(o, 0xC2000 + last, rows)
        sel[last + 1 :] = 0
        sel[last] = 1
        top = max(i for i in range(rows) if sel[i])  # brute force: the last set bit
        assert top == last
        assert R.selector_prefix(sel, n_vars) == min(rows, 128 * (top // 128 + 1))
    assert R.selector_prefix(np.zeros(rows, dtype=np.uint8), n_vars) == 0
    a, b = np.zeros(rows, dtype=np.uint8), np.ones(rows, dtype=np.uint8)
    a[0] = 1
    assert R.flush_witness(n_vars, [b, a], [(R.random_column(1, rows, 3), 3, 5)], 9)[0] == min(rows, 128), "the prefix is the minimum over the selectors"
    assert R.flush_witness(n_vars, [], [(R.random_column(1, rows, 3), 3, 5)], 9)[0] == rows


def small_system(o):
    n = 5
    s0, s1, s2 = rand_bits(o, 0xC3001, 1 << n), rand_bits(o, 0xC3002, 1 << n), rand_bits(o, 0xC3003, 8)
    c32, c8, c128, c1 = (R.random_column(0xC3010 + l, 1 << n, l) for l in (5, 3, 7, 0))
    d16 = R.random_column(0xC3020, 8, 4)
    nz = R.random_column(0xC3030, 1 << n, 4).copy()
    nz[nz == 0] = 1
    flushes = [
        {"channel": 0, "n_vars": n, "selectors": [(10, s0)], "entries": [("oracle", 20, c32, 5), ("const", 77), ("oracle", 21, c8, 3)]},
        {"channel": 1, "n_vars": 3, "selectors": [(12, s2)], "entries": [("oracle", 30, d16, 4)]},
        {"channel": 1, "n_vars": n, "selectors": [(11, s1), (10, s0)], "entries": [("oracle", 21, c8, 3), ("oracle", 22, c128, 7), ("oracle", 5, c1, 0)]},
        {"channel": 2, "n_vars": n, "selectors": [], "entries": [("oracle", 20, c32, 5)]},
    ]
    cols = {10: R.embed(s0.astype(np.uint64), 0), 11: R.embed(s1.astype(np.uint64), 0), 12: R.embed(s2.astype(np.uint64), 0), 20: R.embed(c32, 5),
            21: R.embed(c8, 3), 22: c128, 5: R.embed(c1.astype(np.uint64), 0), 30: R.embed(d16, 4)}
    return flushes, [(40, nz, 4, n)], cols


def test_prover_output_passes_the_verifiers_and_its_claims_are_evaluations(oracle):
    o = oracle
    flushes, nonzero, cols = small_system(o)
    S = o.random_scalars
    m = 5
    groups = R.flush_groups(flushes)
    assert [(g[0], g[1]) for g in groups] == [(5, [0, 2]), (3, [1])] and groups[0][2] == [5, 10, 11, 20, 21, 22], "grouped by point, first appearance; sorted union"
    smp = dict(mixing_challenge=S(0xC4000, 1)[0], permutation_challenges=S(0xC4001, 3), gpa_batch_coeffs=S(0xC4002, m),
               gpa_sumcheck_challenges=[S(0xC4100 + j, max(1, j))[:j] for j in range(m)], gpa_challenges=S(0xC4003, m), red_batch_coeffs=S(0xC4004, 2),
               red_challenges=[S(0xC4200 + g, n) for g, (n, _, _) in enumerate(groups)])
    out = R.flush_prodcheck_prove(flushes, nonzero, **smp)
    n_vars = [fl["n_vars"] for fl in flushes] + [nonzero[0][3]]
    points, evals = G.gpa_verify(n_vars, out["gpa"]["products"], out["gpa"], smp["gpa_batch_coeffs"], smp["gpa_sumcheck_challenges"], smp["gpa_challenges"])
    assert points == out["gpa"]["final_points"] and evals == out["gpa"]["final_evals"]
    assert out["linear_flushes"] == [3]
    terms = [R.mixing_terms(fl["entries"], smp["mixing_challenge"], smp["permutation_challenges"][fl["channel"]]) for fl in flushes]
    # the grand-product argument's claim on a flush is its witness's evaluation; on the linear one it is the linear combination's
    lin = o.mle_evaluate(np.ascontiguousarray(cols[20]), 5, points[3])
    assert evals[3] == terms[3][0] ^ o.mul(terms[3][1][0], lin)
    for g, (n, members, ids) in enumerate(groups):
        chk = out["checks"][g]
        assert chk["ids"] == ids and len(chk["round_proofs"]) == n
        assert len(chk["round_proofs"][0]) == max(2, max(len(flushes[f]["selectors"]) + 1 for f in members)) + 1, "truncated: degree + 1 coefficients"
        R.mlecheck_verify(flushes, terms, chk, members, points[members[0]], [evals[f] for f in members], smp["red_batch_coeffs"][g], smp["red_challenges"][g])
    claims = R.new_claims(out, smp["red_challenges"])
    assert [c[0] for c in claims] == groups[0][2] + groups[1][2]
    for oid, point, ev in claims:
        assert ev == o.mle_evaluate(np.ascontiguousarray(cols[oid]), len(point), point), "claim on oracle %d" % oid
    # a verifier must notice a wrong evaluation
    bad = dict(out["checks"][0], final_evals=[out["checks"][0]["final_evals"][0] ^ 1] + out["checks"][0]["final_evals"][1:])
    with pytest.raises(AssertionError):
        R.mlecheck_verify(flushes, terms, bad, groups[0][1], points[0], [evals[0], evals[2]], smp["red_batch_coeffs"][0], smp["red_challenges"][0])


def test_zero_nonzero_product_is_the_zeros_error(oracle):
    flushes, nonzero, _ = small_system(oracle)
    z = nonzero[0][1].copy()
    z[3] = 0
    with pytest.raises(R.ZerosError):
        R.flush_prodcheck_prove(flushes, [(40, z, 4, 5)], 3, [1, 2, 3], [1] * 5, [[1] * j for j in range(5)], [1] * 5, [1, 1], [[1] * 5, [1] * 3])
