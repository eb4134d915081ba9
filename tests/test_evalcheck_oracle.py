"""Pins tests/evalcheck_ref.py (CPU only): the shift indicator against its brute-force definition and against the point formula, the
identities that make a shifted / packed claim a bivariate sumcheck over b variables, and the prover's transcript against the verifier's
equations, with tampered inputs rejected."""
import random

import numpy as np
import pytest

import evalcheck_ref as ref
import oracle as o

VARIANTS = [ref.CIRCULAR_LEFT, ref.LOGICAL_LEFT, ref.LOGICAL_RIGHT]


def _offsets(b):
    n = 1 << b
    if b <= 3:
        return list(range(1, n))
    return sorted({1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 1, 5 % n or 1})


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 6])
def test_shift_indicator_is_its_brute_force_definition(b, variant):
    r = o.random_scalars(0xEC000 + 16 * b + variant, b)
    for offset in _offsets(b):
        assert ref.shift_ind_table(b, offset, variant, r) == ref.shift_ind_brute(b, offset, variant, r), (b, offset, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("b", [1, 3, 6])
def test_shift_indicator_extends_to_the_point_formula(b, variant):
    r = o.random_scalars(0xEC100 + 16 * b + variant, b)
    x = o.random_scalars(0xEC200 + 16 * b + variant, b)
    for offset in _offsets(b)[:4]:
        table = o.ints_to_arr(ref.shift_ind_table(b, offset, variant, r))
        assert o.mle_evaluate(table, b, x) == ref.shift_ind_eval(b, offset, variant, x, r), (b, offset, variant)


def test_shift_indicator_rejects_invalid_arguments():
    r = o.random_scalars(1, 3)
    for bad in (0, 8, 9):
        with pytest.raises(AssertionError):
            ref.shift_ind_table(3, bad, ref.CIRCULAR_LEFT, r)
    with pytest.raises(AssertionError):
        ref.shift_ind_table(3, 1, ref.CIRCULAR_LEFT, r[:2])


def _random_values(seed, n, level):
    rng = random.Random(seed)
    return [rng.getrandbits(1 << level) for _ in range(n)]


@pytest.mark.parametrize("level,n_vars,b,offset,variant", [
    (0, 9, 5, 1, ref.LOGICAL_LEFT), (0, 10, 6, 17, ref.CIRCULAR_LEFT), (0, 8, 3, 2, ref.LOGICAL_RIGHT),
    (5, 6, 3, 1, ref.LOGICAL_RIGHT), (5, 5, 2, 3, ref.CIRCULAR_LEFT), (5, 7, 4, 5, ref.LOGICAL_LEFT),
])
def test_a_shifted_claim_is_the_sum_of_projection_times_indicator(level, n_vars, b, offset, variant):
    values = _random_values(0xEC300 + n_vars, 1 << n_vars, level)
    point = o.random_scalars(0xEC400 + n_vars + level, n_vars)
    shifted = ref.shifted_column(values, b, offset, variant)
    want = o.mle_evaluate(o.ints_to_arr(shifted), n_vars, point)
    proj = ref.project(ref.pack_values(values, level), level, n_vars, point[b:])
    ind = o.ints_to_arr(ref.shift_ind_table(b, offset, variant, point[:b]))
    assert o.inner_product(proj, 7, ind)[1] == want
    # and the projection is the widened column with its high variables bound
    assert o.arr_to_ints(ref.widen(ref.pack_values(values, level), level, n_vars)) == values


@pytest.mark.parametrize("iota,k,n_vars", [(0, 6, 10), (0, 3, 8), (3, 2, 6), (5, 2, 5)])
def test_a_packed_claim_is_the_sum_of_projection_times_tower_basis(iota, k, n_vars):
    values = _random_values(0xEC500 + n_vars, 1 << n_vars, iota)
    point = o.random_scalars(0xEC600 + n_vars + iota, n_vars - k)
    packed = ref.packed_column(values, k, iota)
    want = o.mle_evaluate(o.ints_to_arr(packed), n_vars - k, point)
    proj = ref.project(ref.pack_values(values, iota), iota, n_vars, point)
    assert o.inner_product(proj, 7, o.ints_to_arr(ref.tower_basis_table(k, iota)))[1] == want


def _round():
    """Three provers of 3, 5 and 6 variables: B64 logical right; B1 logical left; B1 circular left, a packed claim and a shared indicator."""
    pool = o.random_scalars(0xEC700, 40)
    c64 = [ref.pack_values(_random_values(0xEC710 + t, 1 << 6, 6), 6) for t in range(2)]
    c1a = [ref.pack_values(_random_values(0xEC720 + t, 1 << 9, 0), 0) for t in range(2)]
    c1b = [ref.pack_values(_random_values(0xEC730 + t, 1 << 10, 0), 0) for t in range(3)]
    # pool: [0:6) r of the 6-variable claims, [6:10) their suffix; [10:15) r of the 5-variable ones, [15:19) suffix; [19:22) r, [22:25) suffix;
    # [25:29) the packed claims' point
    p3 = (3, [("proj", c64[0], 6, 6, 22, 3), ("shift", 3, 1, ref.LOGICAL_RIGHT, 19, 3), ("proj", c64[1], 6, 6, 22, 3)], [(0, 1), (2, 1)], None)
    p5 = (5, [("proj", c1a[0], 0, 9, 15, 4), ("shift", 5, 1, ref.LOGICAL_LEFT, 10, 5), ("proj", c1a[1], 0, 9, 15, 4)], [(0, 1), (2, 1)], None)
    p6 = (6, [("proj", c1b[0], 0, 10, 6, 4), ("shift", 6, 17, ref.CIRCULAR_LEFT, 0, 6), ("proj", c1b[1], 0, 10, 6, 4), ("shift", 6, 63, ref.CIRCULAR_LEFT, 0, 6),
              ("proj", c1b[0], 0, 10, 25, 4), ("basis", 6, 0), ("proj", c1b[2], 0, 10, 6, 4)], [(0, 1), (2, 3), (4, 5), (6, 1)], None)
    provers = [p3, p5, p6]
    tables = ref.resolve(provers, pool)
    provers = [(b, mls, comps, ref.claim_sums(tabs, comps)) for (b, mls, comps, _), tabs in zip(provers, tables)]
    return provers, pool, o.random_scalars(0xEC740, 3), o.random_scalars(0xEC750, 6)


def test_prover_output_satisfies_the_verifier():
    provers, pool, bcs, chs = _round()
    proofs, evals = ref.prove(provers, pool, bcs, chs)
    assert len(proofs) == 6 and [len(e) for e in evals] == [3, 3, 7]
    assert ref.verify(provers, pool, bcs, chs, proofs, evals)
    # the new claims: a projection's final value is the inner column at r' || suffix
    b, mls, _c, _s = provers[2]
    _, col, level, n_vars, off, ln = mls[4]
    assert evals[2][4] == o.mle_evaluate(ref.widen(col, level, n_vars), n_vars, list(reversed(chs[:b])) + pool[off : off + ln])
    # the sums are the claimed evaluations of the virtual columns: the first 6-variable claim is a circular shift by 17
    values = o.arr_to_ints(ref.widen(mls[0][1], 0, 10))
    assert provers[2][3][0] == o.mle_evaluate(o.ints_to_arr(ref.shifted_column(values, 6, 17, ref.CIRCULAR_LEFT)), 10, pool[0:6] + pool[6:10])


def test_tampered_sum_is_rejected():
    provers, pool, bcs, chs = _round()
    b, mls, comps, sums = provers[1]
    bad = provers[:1] + [(b, mls, comps, [sums[0] ^ 1] + sums[1:])] + provers[2:]
    proofs, evals = ref.prove(bad, pool, bcs, chs)
    assert not ref.verify(bad, pool, bcs, chs, proofs, evals)


def test_tampered_table_is_rejected():
    provers, pool, bcs, chs = _round()
    for prover, ml in ((2, 1), (2, 0), (0, 2), (2, 5)):
        tables = ref.resolve(provers, pool)
        tables[prover][ml][3, 0] ^= np.uint64(1)
        proofs, evals = ref.prove(provers, pool, bcs, chs, tables=tables)
        assert not ref.verify(provers, pool, bcs, chs, proofs, evals), (prover, ml)


def test_tampered_transcript_is_rejected():
    provers, pool, bcs, chs = _round()
    proofs, evals = ref.prove(provers, pool, bcs, chs)
    bad = [list(p) for p in proofs]
    bad[2][1] ^= 1
    assert not ref.verify(provers, pool, bcs, chs, bad, evals)
    bad_evals = [list(e) for e in evals]
    bad_evals[0][0] ^= 1
    assert not ref.verify(provers, pool, bcs, chs, proofs, bad_evals)
