"""The checker's own pins for tests/test_gpu_adversarial.py.  That module compares the HIP kernels with the PCLMULQDQ oracle
(oracle/fastcpu_ref.c: fast_inner_product, fast_bivariate_sumcheck_prove) at sizes the scalar tower-recursion restatement is too
slow for, on patterned operands and edge scalars; tests/test_oracle_fastcpu.py pins the fast oracle to the scalar one on random
inputs only.  Here: every operand kind and every edge scalar at n <= 16 -- transcript, final evaluations and the verifier's
equations --, and the operand generator itself (bit counts per element, subfield membership through the oracle's field)."""
import numpy as np
import pytest

import adversarial as A


@pytest.fixture(scope="module")
def oracle():
    import oracle as o

    o.build()
    return o


def fast_or_skip(res):
    if res is None:
        pytest.skip("host without PCLMULQDQ")
    return res


def verifier_accepts(oracle, comps, sums, batch_coeff, challenges, coeffs, finals):
    """P_r(0) + P_r(1) = the running sum, P_r(z_r) becomes the next one, the batched product of the final evaluations is the last."""
    running = oracle.evaluate_univariate(sums, batch_coeff)
    for r, (c0, c1, c2) in enumerate(coeffs):
        assert c0 ^ (c0 ^ c1 ^ c2) == running, "round %d" % r
        running = oracle.evaluate_univariate([c0, c1, c2], challenges[r])
    expect, p = 0, 1
    for i, j in comps:
        expect ^= oracle.mul(oracle.mul(finals[i], finals[j]), p)
        p = oracle.mul(p, batch_coeff)
    assert expect == running


# ------------------------------------------------------------------ the generator
@pytest.mark.parametrize("n", [1, 1000, 1 << 12])
def test_operand_bit_counts(oracle, n):
    pc = A.popcounts
    assert (pc(A.operands("dense", 1, n)) == 127).all()
    assert (pc(A.operands("sparse", 2, n)) == 1).all()
    assert (pc(A.operands("zero", 3, n)) == 0).all()
    r = A.operands("random", 4, n)
    n8, n7 = A.operands("nib8", 4, n), A.operands("nib7", 4, n)
    assert np.array_equal(n8 | n7, r) and not (n8 & n7).any()
    assert not (n8 & np.uint64(0x7777777777777777)).any() and not (n7 & np.uint64(0x8888888888888888)).any()
    for j in range(4):
        x = A.operands("limb%d" % j, 5 + j, n)
        keep = np.zeros(2, dtype=np.uint64)
        keep[j >> 1] = np.uint64(0xFFFFFFFF << (32 * (j & 1)))
        assert not (x & ~keep).any()
        assert n < 1000 or (x[:, j >> 1] != 0).sum() > n - 8  # random inside the limb
    a, b = A.pair("same", 9, n)
    assert np.array_equal(a, b) and a is not b and not np.shares_memory(a, b)
    z, other = A.pair("zero", 10, n)
    assert not z.any() and (n < 1000 or other.any())
    # deterministic from the seed, different across seeds
    for kind in A.KINDS:
        assert np.array_equal(A.operands(kind, 77, n), A.operands(kind, 77, n))
    if n >= 1000:
        # the cleared / set bit moves over all 128 positions and both words
        for kind in ("dense", "sparse"):
            x = A.operands(kind, 11, n)
            x = ~x if kind == "dense" else x
            assert np.bitwise_or.reduce(x[:, 0]) == np.uint64(A.M64) and np.bitwise_or.reduce(x[:, 1]) == np.uint64(A.M64)
            assert not np.array_equal(A.operands(kind, 11, n), A.operands(kind, 12, n))


@pytest.mark.parametrize("level", [0, 3, 5])
def test_subfield_operands_are_subfield_elements(oracle, level):
    """x is in the subfield of 2^(2^l) elements iff x^(2^(2^l)) = x; the values are not all in the next smaller subfield."""
    x = A.operands("sub%d" % level, 21, 256)
    vals = oracle.arr_to_ints(x)
    for v in vals:
        y = v
        for _ in range(1 << level):
            y = oracle.square(y)
        assert y == v
    assert all(v < (1 << (1 << level)) for v in vals)
    if level:
        def in_smaller(v):
            y = v
            for _ in range(1 << (level - 1)):
                y = oracle.square(y)
            return y == v

        assert not all(in_smaller(v) for v in vals)
    else:
        assert set(vals) == {0, 1}
    # the edge scalars named "a B8 element" and "a B32 element" are what they are called, and in no smaller subfield
    for v, lv in ((A.EDGE_SCALARS[3], 3), (A.EDGE_SCALARS[4], 5)):
        y = v
        for _ in range(1 << (lv - 1)):
            y = oracle.square(y)
        assert y != v
        for _ in range(1 << (lv - 1)):
            y = oracle.square(y)
        assert y == v


# ------------------------------------------------------------------ the fast oracle on every operand kind
@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("n", [1000, (1 << 14) + 3])
def test_fast_inner_product_on_operand_kinds(oracle, kind, n):
    a, b = A.pair(kind, 0xAD00 + n, n)
    a0, b0 = a.copy(), b.copy()
    got = fast_or_skip(oracle.fast_inner_product(a, b, threads=3))
    rc, want = oracle.inner_product(a, 7, b)
    assert rc == 0 and got == want
    assert np.array_equal(a, a0) and np.array_equal(b, b0)
    if kind == "zero":
        assert got == 0


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("level", [0, 3, 4, 5, 6])
def test_subfield_inner_product_through_the_fast_oracle(oracle, kind, level):
    """sum_i a_i * b_i with a_i the packed level-l values: the scalar oracle's subfield x F product equals the fast oracle's F x F
    product of the embedded values -- the reference the GPU module uses for inner_product at levels below 7."""
    n_b = 1 << 12
    a, b = A.pair(kind, 0xAD60 + level, n_b)
    a = np.ascontiguousarray(a[: n_b >> (7 - level)])
    rc, want = oracle.inner_product(a, level, b)
    assert rc == 0
    wide = A.unpack_subfield(a, level)
    assert wide.shape == (n_b, 2)
    assert fast_or_skip(oracle.fast_inner_product(wide, b, threads=2)) == want


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("n_vars", [5, 12, 16])
def test_fast_sumcheck_on_operand_kinds(oracle, kind, n_vars):
    mls = list(A.pair(kind, 0xAD10 + n_vars, 1 << n_vars))
    comps = [(0, 1)]
    sums = [oracle.inner_product(mls[0], 7, mls[1])[1]]
    stream = oracle.random_scalars(0xAD20 + n_vars, n_vars + 1)
    bc, ch = stream[0], stream[1:]
    want = oracle.bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch, threads=4)
    got = fast_or_skip(oracle.fast_bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch, threads=4))
    assert got[0] == want[0] and got[1] == want[1]
    verifier_accepts(oracle, comps, sums, bc, ch, got[0], got[1])


def test_fast_sumcheck_on_a_claim_group_of_mixed_kinds(oracle):
    """Four claims over eight multilinears of eight different kinds, one multilinear shared: the shape of the GPU module's group case."""
    n_vars, comps = 12, [(0, 4), (1, 5), (2, 6), (0, 7)]
    kinds = ("dense", "sparse", "nib8", "nib7", "limb1", "sub3", "zero", "limb2")
    mls = [A.operands(k, 0xAD30 + j, 1 << n_vars) for j, k in enumerate(kinds)]
    sums = [oracle.inner_product(mls[i], 7, mls[j])[1] for i, j in comps]
    stream = oracle.random_scalars(0xAD31, n_vars + 1)
    bc, ch = stream[0], stream[1:]
    want = oracle.bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch)
    got = fast_or_skip(oracle.fast_bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch, threads=4))
    assert got[0] == want[0] and got[1] == want[1]
    verifier_accepts(oracle, comps, sums, bc, ch, got[0], got[1])


# ------------------------------------------------------------------ the fast oracle on every edge scalar
def _edge_challenge_vectors(n_vars):
    out = [("all %#x" % z, [z] * n_vars) for z in A.EDGE_SCALARS]
    out.append(("cycle", [A.EDGE_SCALARS[r % len(A.EDGE_SCALARS)] for r in range(n_vars)]))
    return out


@pytest.mark.parametrize("kind", ["random", "dense"])
@pytest.mark.parametrize("n_vars", [7, 14])
def test_fast_sumcheck_with_edge_challenges(oracle, kind, n_vars):
    mls = list(A.pair(kind, 0xAD40 + n_vars, 1 << n_vars))
    comps = [(0, 1)]
    sums = [oracle.inner_product(mls[0], 7, mls[1])[1]]
    bc = oracle.random_scalars(0xAD41, 1)[0]
    for name, ch in _edge_challenge_vectors(n_vars):
        want = oracle.bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch, threads=4)
        got = fast_or_skip(oracle.fast_bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch, threads=4))
        assert got[0] == want[0] and got[1] == want[1], name
        verifier_accepts(oracle, comps, sums, bc, ch, got[0], got[1])
    # folding with 0 keeps the lower half, with 1 the upper half (High-to-Low: the top variable first)
    z0 = oracle.fast_bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, [0] * n_vars, threads=2)[1]
    z1 = oracle.fast_bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, [1] * n_vars, threads=2)[1]
    assert z0 == [oracle.arr_to_ints(x[:1])[0] for x in mls]
    assert z1 == [oracle.arr_to_ints(x[-1:])[0] for x in mls]


@pytest.mark.parametrize("bc", [0, 1, A.ALL_ONES])
@pytest.mark.parametrize("n_vars", [6, 13])
def test_fast_sumcheck_with_edge_batching_coefficients(oracle, bc, n_vars):
    """Two claims batched with 0 (the second claim vanishes), 1 (plain sum) and all ones."""
    comps = [(0, 1), (2, 1)]
    mls = [oracle.random_b128(0xAD50 + n_vars + j, 1 << n_vars) for j in range(3)]
    sums = [oracle.inner_product(mls[i], 7, mls[j])[1] for i, j in comps]
    ch = oracle.random_scalars(0xAD51, n_vars)
    want = oracle.bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch)
    got = fast_or_skip(oracle.fast_bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, comps, sums, bc, ch, threads=4))
    assert got[0] == want[0] and got[1] == want[1]
    verifier_accepts(oracle, comps, sums, bc, ch, got[0], got[1])
