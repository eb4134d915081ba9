"""GPU parity of the univariate round of the univariate-skip zerocheck (bn_zerocheck_univariate_evals: binius_amd/csrc/
kernels_univariate.hip + abi_univariate.cpp; reference: prove/univariate.rs:235-507, :571-640) against the CPU restatement
tests/univariate_skip_ref.py (pinned by tests/test_univariate_skip_oracle.py): per-composition and batched output, B1 and B8 columns,
k in {1, 3, 6, 7, 8}, degrees 1 .. 4 with d 2^k <= 256, n in {k, k + 1, k + 6}, and the keccak table's constraint set at n = 13.
The definition holds without the constraints, so the witnesses are random.  Every case runs twice from resident inputs and must give
the same values; every validation case is an error."""
import numpy as np
import pytest

import univariate_skip_ref as R
from test_gpu_hal import upload
from test_gpu_hal_wide import keccak_constraints

pytestmark = pytest.mark.gpu


def comp_set(d_max):
    """Compositions over B8 of degrees up to d_max (constants in B8, a power, a product of d_max columns) over 5 columns."""
    top = [("var", 0)]
    for i in range(1, d_max):
        top += [("var", i), ("mul", len(top) - 1, len(top))]
    top += [("var", 4), ("add", len(top) - 1, len(top)), ("const", 0x53), ("add", len(top) + 1, len(top) + 2)]
    lin = [("var", 0), ("var", 1), ("add", 0, 1), ("const", 7), ("add", 2, 3)]
    comps, degrees = [top, lin], [d_max, 1]
    if d_max >= 2:
        comps.append([("var", 2), ("const", 0x9D), ("mul", 0, 1), ("var", 3), ("mul", 2, 3)])
        degrees.append(2)
    if d_max >= 3:
        comps.append([("var", 1), ("pow", 0, 3), ("var", 4), ("add", 1, 2)])
        degrees.append(3)
    return comps, degrees


def run_case(oracle, hal, n_vars, k, level, comps, degrees, vals, seed):
    D = max(degrees) << k
    ch = oracle.random_scalars(0x7A00 + seed, n_vars - k)
    alpha = oracle.random_scalars(0x7A80 + seed, 1)[0]
    cols = [(v, level) for v in vals]
    want = R.univariate_evals(cols, n_vars, k, comps, degrees, ch, D)
    want_b, scale = [0] * (D - (1 << k)), 1
    for p in want:
        want_b = [a ^ oracle.mul(scale, b) for a, b in zip(want_b, p)]
        scale = oracle.mul(scale, alpha)
    alloc = hal.dev_alloc()
    d_cols = [(upload(hal, alloc, R.pack(v, level)), level) for v in vals]
    d_eq = upload(hal, alloc, oracle.ints_to_arr(R.eq_expansion(ch)))
    for _ in range(2):  # resident inputs, run twice: the same values
        got = hal.zerocheck_univariate_evals(n_vars, k, d_cols, comps, degrees, d_eq, D)
        got_b = hal.zerocheck_univariate_evals(n_vars, k, d_cols, comps, degrees, d_eq, D, alpha)
        assert got == want, "per-composition output differs (n=%d k=%d level=%d)" % (n_vars, k, level)
        assert got_b == want_b, "batched output differs (n=%d k=%d level=%d)" % (n_vars, k, level)


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, 1 << 24)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("k", [1, 3, 6, 7, 8])
def test_univariate_evals_vs_restatement(oracle, hal, k, level):
    rng = np.random.default_rng(100 * k + level)
    for d_max in (1, 2, 3, 4):
        if d_max << k > 256:
            continue
        comps, degrees = comp_set(d_max)
        for n_vars in (k, k + 1, k + 6):
            vals = [rng.integers(0, 2 if level == 0 else 256, 1 << n_vars, dtype=np.uint8) for _ in range(5)]
            run_case(oracle, hal, n_vars, k, level, comps, degrees, vals, 16 * n_vars + d_max)


def test_keccak_shape_vs_restatement(oracle, hal):
    """The keccak table's 100 constraints of degree 2 over 204 one-bit columns, k = 7, n = 13."""
    n_mls, cons = keccak_constraints(3)
    comps = [s for s, _ in cons]
    rng = np.random.default_rng(0x4B)
    vals = [rng.integers(0, 2, 1 << 13, dtype=np.uint8) for _ in range(n_mls)]
    run_case(oracle, hal, 13, 7, 0, comps, [2] * len(comps), vals, 0x4B)


def test_keccak_shape_short_last_tile(oracle, hal):
    """n = 15: 256 values of x over 20 tiles of 13 -- the last tile holds 9 (the clamp of the tile loop)."""
    n_mls, cons = keccak_constraints(3)
    comps = [s for s, _ in cons]
    rng = np.random.default_rng(0x4C)
    vals = [rng.integers(0, 2, 1 << 15, dtype=np.uint8) for _ in range(n_mls)]
    run_case(oracle, hal, 15, 7, 0, comps, [2] * len(comps), vals, 0x4C)


@pytest.mark.parametrize("level,n_vars,k", [(0, 13, 7), (0, 12, 3), (3, 10, 6), (3, 8, 1)])
def test_fold_vs_restatement(oracle, hal, level, n_vars, k):
    """The univariate round's fold: bn_fold_right of the packed column with the 2^k Lagrange coefficients L_u(z) computed on the
    host in GF(2^128) (univariate.rs:139-195, prove/zerocheck.rs:384-434)."""
    rng = np.random.default_rng(13 * n_vars + k + level)
    v = rng.integers(0, 2 if level == 0 else 256, 1 << n_vars, dtype=np.uint8)
    z = oracle.random_scalars(0x7B00 + n_vars, 1)[0]
    coeffs = R.lagrange_at(1 << k, z)
    alloc = hal.dev_alloc()
    col = upload(hal, alloc, R.pack(v, level))
    q = upload(hal, alloc, oracle.ints_to_arr(coeffs))
    out = alloc.alloc(1 << (n_vars - k))
    hal.fold_right(col, level, q, out)
    assert oracle.arr_to_ints(hal.copy_d2h(out)) == R.fold(v, k, coeffs)


def u32_add_witness(log_rows, seed):
    """Columns 0 xin, 1 yin, 2 cin, 3 cout, 4 zout of real 32-bit additions (value index = 32 row + bit)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, 1 << log_rows, dtype=np.uint64).astype(np.uint32)
    y = rng.integers(0, 1 << 32, 1 << log_rows, dtype=np.uint64).astype(np.uint32)
    z = (x.astype(np.uint64) + y).astype(np.uint32)
    cin = x ^ y ^ z
    cout = (x & y) | (cin & (x ^ y))
    return [np.unpackbits(w.view(np.uint8), bitorder="little") for w in (x, y, cin, cout, z)]


def test_u32_add_at_2_22_values_per_column_satisfies_the_verifier(oracle, hal):
    """2^17 real additions = 2^22 one-bit values per column, k = 7: too large for the brute-force restatement, so the device's
    message (per composition and batched) is checked by the verifier's equation at a random z against the claim computed in
    GF(2^128) from the witness."""
    n_vars, k = 22, 7
    vals = u32_add_witness(17, 0x32)
    # carry: (xin + cin)(yin + cin) + cin + cout, zout: xin + yin + cin + zout (m3/src/gadgets/add.rs:95-110)
    carry = [("var", 0), ("var", 2), ("add", 0, 1), ("var", 1), ("var", 2), ("add", 3, 4), ("mul", 2, 5), ("var", 2), ("add", 6, 7), ("var", 3), ("add", 8, 9)]
    zout = [("var", 0), ("var", 1), ("add", 0, 1), ("var", 2), ("add", 2, 3), ("var", 4), ("add", 4, 5)]
    comps, degrees = [carry, zout], [2, 1]
    D = 2 << k
    ch = oracle.random_scalars(0x7C00, n_vars - k)
    alpha, z = oracle.random_scalars(0x7C80, 2)
    eq_ints = R.eq_expansion(ch)
    alloc = hal.dev_alloc()
    d_cols = [(upload(hal, alloc, R.pack(v, 0)), 0) for v in vals]
    d_eq = upload(hal, alloc, oracle.ints_to_arr(eq_ints))
    per = hal.zerocheck_univariate_evals(n_vars, k, d_cols, comps, degrees, d_eq, D)
    batched = hal.zerocheck_univariate_evals(n_vars, k, d_cols, comps, degrees, d_eq, D, alpha)
    assert all(v == 0 for v in per[1])  # degree 1: the zero polynomial
    want = R.claim_at(vals, n_vars, k, comps[0], eq_ints, z)
    assert R.message_at(k, D, per[0], z) == want
    assert R.message_at(k, D, batched, z) == want  # (the linear constraint adds nothing: alpha^1 * 0)
    assert batched == per[0]


def test_validation_errors(oracle, hal):
    import binius_amd

    alloc = hal.dev_alloc()
    n_vars, k = 8, 3
    col0 = upload(hal, alloc, R.pack(np.ones(1 << n_vars, dtype=np.uint8), 0))
    eq = upload(hal, alloc, oracle.ints_to_arr(R.eq_expansion(oracle.random_scalars(5, n_vars - k))))
    quad = [("var", 0), ("var", 0), ("mul", 0, 1)]
    # the valid call first: the cases below differ from it in one argument each
    assert len(hal.zerocheck_univariate_evals(n_vars, k, [(col0, 0)], [quad], [2], eq, 16)[0]) == 8
    wide = upload(hal, alloc, oracle.random_b128(6, (1 << n_vars) >> 2))  # a level-5 column of the same size
    cases = [
        (n_vars, k, [(wide, 5)], [quad], [2], eq, 16),                                     # level outside {0, 3}
        (n_vars, k, [(col0, 0)], [quad + [("const", 0x100), ("add", 2, 3)]], [2], eq, 16),  # constant outside B8
        (n_vars, 7, [(col0, 0)], [quad], [3], None, 256),                                  # d * 2^k > 256
        (n_vars, n_vars + 1, [(col0, 0)], [quad], [2], eq, 256),                           # k > n
        (n_vars, 0, [(col0, 0)], [quad], [2], eq, 2),                                      # k = 0
    ]
    for args in cases:
        with pytest.raises(binius_amd.BnError) as e:
            hal.zerocheck_univariate_evals(*args)
        assert e.value.kind == "InputValidation", args
