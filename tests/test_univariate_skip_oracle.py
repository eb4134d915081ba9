"""Pins the CPU restatement of the univariate round of the univariate-skip zerocheck (tests/univariate_skip_ref.py) by the
VERIFIER's equation (crates/core/src/protocols/sumcheck/verify_zerocheck.rs:92-112): on a witness that satisfies the constraints,
the prover's message -- P_c(omega_j) for 2^k <= j < D, zeros in front -- interpolated over omega_0 .. omega_{D-1} and evaluated at
a challenge z of GF(2^128) equals sum_x eq(x) C_c(Mhat_1(z, x), ...), the claim the eq-ind rounds take over.  The right-hand
side is computed here in GF(2^128) with the oracle's o.mul / o.invert / o.circuit_eval, not in B8.  CPU only."""
import numpy as np
import pytest

import univariate_skip_ref as R

# (a, b random; c = a b; e = a + b): every composition below vanishes on every row
LIN = [("var", 0), ("var", 1), ("add", 0, 1), ("var", 3), ("add", 2, 3)]
QUAD = [("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("add", 2, 3)]
CUBIC = QUAD + [("var", 0), ("mul", 4, 5)]
QUARTIC = CUBIC + [("var", 1), ("mul", 6, 7)]
SATISFIED = [(LIN, 1), (QUAD, 2), (CUBIC, 3), (QUARTIC, 4)]


def witness(seed, n_vars, level):
    mul, _ = R.b8_tables()
    rng = np.random.default_rng(seed)
    hi = 2 if level == 0 else 256
    a, b = rng.integers(0, hi, 1 << n_vars, dtype=np.uint8), rng.integers(0, hi, 1 << n_vars, dtype=np.uint8)
    return [a, b, mul[a, b], a ^ b]


def lagrange_at(o, n, z):
    """ell_p(z), p < n, over omega_0 .. omega_{n-1}, z in GF(2^128) outside the domain: plain products in GF(2^128)."""
    out = []
    for p in range(n):
        num, den = 1, 1
        for q in range(n):
            if q != p:
                num = o.mul(num, z ^ q)
                den = o.mul(den, p ^ q)
        out.append(o.mul(num, o.invert(den)))
    return out


def direct_claim(o, vals, n_vars, k, steps, eq_ints, z):
    """sum_x eq(x) C(Mhat_1(z, x), ...), Mhat_i(z, x) = sum_u L_u(z) M_i(u + 2^k x), all in GF(2^128)."""
    K = 1 << k
    L = lagrange_at(o, K, z)
    used = sorted({s[1] for s in steps if s[0] == "var"})
    total = 0
    for x in range(1 << (n_vars - k)):
        q = [0] * (max(used) + 1)
        for i in used:
            acc = 0
            for u in range(K):
                acc ^= o.mul(L[u], int(vals[i][u + K * x]))
            q[i] = acc
        total ^= o.mul(eq_ints[x], o.circuit_eval(steps, q))
    return total


def test_b8_action_on_gf128_is_coordinatewise(oracle):
    """The restatement multiplies a GF(2^128) element by a B8 scalar byte by byte; the oracle's full product agrees."""
    rng = np.random.default_rng(7)
    for _ in range(300):
        s = int(rng.integers(0, 256))
        e = int.from_bytes(rng.bytes(16), "little")
        assert R.bytes_to_int(R.b8_times_b128(np.uint8(s), R.int_to_bytes(e))) == oracle.mul(s, e)


def test_lagrange_basis_is_the_identity_on_its_domain(oracle):
    W = R.lagrange_matrix(8, range(8))
    assert np.array_equal(W, np.eye(8, dtype=np.uint8))
    # and sums to one anywhere (the constant polynomial)
    W = R.lagrange_matrix(16, range(16, 256))
    assert np.all(np.bitwise_xor.reduce(W, axis=1) == 1)


@pytest.mark.parametrize("level,n_vars,k", [(0, 9, 7), (0, 10, 3), (3, 6, 1), (3, 9, 6)])
def test_fold_matches_the_oracles_fold_right(oracle, level, n_vars, k):
    """The restatement's fold (evaluate_partial_low at 2^k coefficients) is the oracle's pinned fold_right of the packed column."""
    rng = np.random.default_rng(11 * n_vars + k)
    v = rng.integers(0, 2 if level == 0 else 256, 1 << n_vars, dtype=np.uint8)
    coeffs = oracle.random_scalars(0x5E00 + n_vars, 1 << k)
    out = oracle.arr(1 << (n_vars - k))
    assert oracle.fold_right(R.pack(v, level), level, oracle.ints_to_arr(coeffs), out) == 0
    assert R.fold(v, k, coeffs) == oracle.arr_to_ints(out)


def test_claim_restatements_agree(oracle):
    """claim_at (through the fold) equals the per-element sum of direct_claim."""
    vals = witness(5, 9, 3)
    ch = oracle.random_scalars(0x5E80, 6)
    z = oracle.random_scalars(0x5E81, 1)[0]
    eq_ints = R.eq_expansion(ch)
    assert R.claim_at(vals, 9, 3, CUBIC, eq_ints, z) == direct_claim(oracle, vals, 9, 3, CUBIC, eq_ints, z)


def test_pack_roundtrip():
    rng = np.random.default_rng(3)
    for level, hi, n in ((0, 2, 3), (0, 2, 10), (3, 256, 2), (3, 256, 9)):
        v = rng.integers(0, hi, 1 << n, dtype=np.uint8)
        assert np.array_equal(R.unpack(R.pack(v, level), level, n), v)


CASES = [(n, k, d) for k in (1, 3, 6, 7) for d in (1, 2, 3, 4) if d << k <= 256 for n in (k, k + 1, k + 5)]


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("n_vars,k,d", CASES)
def test_restatement_satisfies_the_verifier(oracle, n_vars, k, d, level):
    o = oracle
    seed = 1000 * n_vars + 10 * k + d + 7 * level
    vals = witness(seed, n_vars, level)
    comps = [s for s, dc in SATISFIED if dc <= d]
    degrees = [dc for _, dc in SATISFIED if dc <= d]
    D = d << k
    ch = o.random_scalars(0x5C00 + seed, n_vars - k)
    alpha, z = o.random_scalars(0x5C80 + seed, 2)
    cols = [(v, level) for v in vals]
    per = R.univariate_evals(cols, n_vars, k, comps, degrees, ch, D)
    batched = R.univariate_evals(cols, n_vars, k, comps, degrees, ch, D, alpha)
    assert all(len(p) == D - (1 << k) for p in per) and len(batched) == D - (1 << k)
    eq_ints = R.eq_expansion(ch)
    ell = lagrange_at(o, D, z)
    want_batched, scale = 0, 1
    for steps, p in zip(comps, per):
        got = 0
        for j, v in enumerate(p, start=1 << k):
            got ^= o.mul(v, ell[j])
        want = direct_claim(o, vals, n_vars, k, steps, eq_ints, z)
        assert got == want
        want_batched ^= o.mul(scale, want)
        scale = o.mul(scale, alpha)
    got_batched = 0
    for j, v in enumerate(batched, start=1 << k):
        got_batched ^= o.mul(v, ell[j])
    assert got_batched == want_batched


def test_unsatisfied_witness_breaks_the_equation(oracle):
    """Without the honest zero prefix the message does not interpolate the claim: the check above is not vacuous."""
    o = oracle
    n_vars, k = 5, 3
    vals = witness(99, n_vars, 0)
    vals[2] = vals[2] ^ np.eye(1, 1 << n_vars, 5, dtype=np.uint8)[0]  # one row of c = a b broken
    ch = o.random_scalars(0x5D00, n_vars - k)
    z = o.random_scalars(0x5D01, 1)[0]
    (p,) = R.univariate_evals([(v, 0) for v in vals], n_vars, k, [QUAD], [2], ch, 2 << k)
    ell = lagrange_at(o, 2 << k, z)
    got = 0
    for j, v in enumerate(p, start=1 << k):
        got ^= o.mul(v, ell[j])
    assert got != direct_claim(o, vals, n_vars, k, QUAD, R.eq_expansion(ch), z)
