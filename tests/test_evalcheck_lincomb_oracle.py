"""Pins tests/evalcheck_lincomb_ref.py (CPU only): the projection of a linear combination from its constituents' projections equals the
projection of the combination materialised element by element, for mixed tower levels and coefficients; the prover's restatement passes
the verifier of tests/evalcheck_ref.py; a lincomb's final evaluation is the materialised combination's multilinear extension at
r' || suffix."""
import json
import os

import numpy as np
import pytest

import evalcheck_lincomb_ref as L
import evalcheck_ref as R

GENERATOR = 0x2E895399AF449ACE499596F6E5FCCAFA  # the multiplicative generator of B128 (binary_field.rs:740-747)
# ONE, the generator of B128, all ones, the top basis element, an element of B8, zero, the generator of the tower's second level
COEFFS = (1, GENERATOR, (1 << 128) - 1, 1 << 127, 0x53, 0, 0x2)


def test_the_generator_is_the_recorded_one():
    with open(os.path.join(os.path.dirname(__file__), "golden", "field_kats.json")) as f:
        assert int(json.load(f)["multiplicative_generators"]["128"], 16) == GENERATOR


def column(oracle, seed, level, n_vars):
    return oracle.random_b128(seed, 1 << (n_vars + level - 7))


@pytest.mark.parametrize("n_vars,q", [(10, 4), (9, 0), (8, 8), (12, 7)])
def test_project_lincomb_equals_the_projection_of_the_materialised_column(oracle, n_vars, q):
    terms = [(column(oracle, 0xF1000 + 16 * n_vars + t, level, n_vars), level, COEFFS[(t + n_vars) % len(COEFFS)])
             for t, level in enumerate((0, 0, 3, 4, 5, 6, 7, 3, 0))]
    suffix = oracle.random_scalars(0xF1100 + n_vars, q)
    offset = oracle.random_scalars(0xF1200 + n_vars, 1)[0]
    want = R.project(L.materialise(terms, offset, n_vars), 7, n_vars, suffix)
    assert np.array_equal(L.project_lincomb(terms, offset, n_vars, suffix), want)


def test_degenerate_combinations(oracle):
    suffix = oracle.random_scalars(0xF2000, 3)
    a = column(oracle, 0xF2001, 0, 9)
    assert np.array_equal(L.project_lincomb([], 0x1234, 9, suffix), oracle.ints_to_arr([0x1234] * 64))
    assert np.array_equal(L.project_lincomb([(a, 0, 1)], 0, 9, suffix), R.project(a, 0, 9, suffix))
    assert np.array_equal(L.project_lincomb([(a, 0, 1), (a, 0, 1)], 7, 9, suffix), oracle.ints_to_arr([7] * 64))  # listed twice: it cancels
    assert np.array_equal(L.project_lincomb([(a, 0, 0)], 7, 9, suffix), oracle.ints_to_arr([7] * 64))


def keccak_like(oracle):
    """Two 6-variable provers over 14-variable bit columns: c[x] = the sum of five state columns under a rotation, beside a plain
    projection; and a 3-variable prover with a two-level combination with an offset."""
    pool = oracle.random_scalars(0xF3000, 25)  # [0:6) r, [6:14) its suffix; [14:17) r of the small prover, [17:25) its suffix
    state = [column(oracle, 0xF3100 + t, 0, 14) for t in range(10)]
    mls, comps = [], []
    for x in range(2):
        comps.append((len(mls), len(mls) + 1))
        mls += [("lincomb", [(state[5 * x + y], 0, 1) for y in range(5)], 0, 14, 6, 8), ("shift", 6, 1 + x, R.CIRCULAR_LEFT, 0, 6)]
    comps.append((len(mls), 1))
    mls.append(("proj", state[0], 0, 14, 6, 8))
    b8, b32 = column(oracle, 0xF3200, 3, 11), column(oracle, 0xF3201, 5, 11)
    small = [("lincomb", [(b8, 3, 0x53), (b32, 5, 1 << 127), (b8, 3, 1)], 0xABCDEF << 64, 11, 17, 8), ("shift", 3, 3, R.LOGICAL_RIGHT, 14, 3)]
    return [(3, small, [(0, 1)], None), (6, mls, comps, None)], pool


def test_prover_restatement_passes_the_verifier(oracle):
    provers, pool = keccak_like(oracle)
    tables = L.resolve(provers, pool)
    provers = [(b, mls, comps, R.claim_sums(tabs, comps)) for (b, mls, comps, _), tabs in zip(provers, tables)]
    bcs, chs = oracle.random_scalars(0xF3300, 2), oracle.random_scalars(0xF3301, 6)
    proofs, evals = L.prove(provers, pool, bcs, chs, tables=tables)
    memo = {}
    assert L.verify(provers, pool, bcs, chs, proofs, evals, memo)
    # a lincomb's final evaluation v: the claim (r' || suffix, v) on the combination itself
    for (b, mls, _c, _s), ev in zip(provers, evals):
        r_rev = list(reversed(chs[:b]))
        for ml, v in zip(mls, ev):
            if ml[0] == "lincomb":
                _, terms, offset, n_vars, off, ln = ml
                assert v == oracle.mle_evaluate(L.materialise(terms, offset, n_vars), n_vars, r_rev + list(pool[off : off + ln]))
    # the verifier is a checker: a wrong final evaluation and a wrong offset are refused
    bad = [list(e) for e in evals]
    bad[1][0] ^= 1
    assert not L.verify(provers, pool, bcs, chs, proofs, bad, memo)
    b, mls, comps, sums = provers[0]
    other = [(b, [("lincomb", mls[0][1], mls[0][2] ^ 1) + mls[0][3:]] + mls[1:], comps, sums), provers[1]]
    assert not L.verify(other, pool, bcs, chs, proofs, evals)
