"""Pins of the NTT oracle off the (B16, B16) / (B32, B32) diagonal that tests/test_oracle_pins.py covers, so that the GPU parity of
tests/test_gpu_ntt_pairs.py -- every (element, twiddle) pair the ABI accepts -- rests on definitions and not on the restatement alone:

* the twiddle basis at levels 3 and 6 is the normalized subspace polynomials (the helper of test_oracle_pins.py, unchanged);
* the forward NTT with a subfield twiddle and a wider element is the evaluation of the novel-basis polynomial, the W^_i taken in the
  twiddle field and the product coefficient x W^_i in the element field (a tower subfield element is the low bits of its embedding:
  crates/field/src/binary_field.rs:361-393);
* log_x / log_z batches, cosets and skip_rounds are what their definitions say in terms of the plain transform
  (crates/ntt/src/tests/reference.rs:170-204, additive_ntt.rs:23-56), at a mixed pair;
* the library's host-side twiddle basis (bn_ntt_s_evals) is the oracle's at every level and every domain size.
"""
import numpy as np
import pytest

import test_oracle_pins as pins

DT = {3: np.uint8, 4: np.uint16, 5: np.uint32, 6: np.uint64}


def _stride(s):
    return len(s) // int(round(len(s) ** 0.5))


@pytest.mark.parametrize("level,d", [(3, 8), (3, 5), (6, 7), (6, 9)])
def test_s_evals_are_normalized_subspace_polynomials_levels_3_and_6(oracle, level, d):
    s = oracle.ntt_s_evals(level, d)
    stride = _stride(s)
    beta = [1 << k for k in range(d)]
    for i in range(d):
        for b in range(d - 1 - i):
            assert int(s[i * stride + b]) == pins._w_hat(oracle, beta, i, beta[i + 1 + b], level), (i, b)
        assert pins._w_hat(oracle, beta, i, beta[i], level) == 1
        assert not s[i * stride + max(d - 1 - i, 0) : (i + 1) * stride].any()  # nothing behind the row's d - 1 - i entries


def _elem_mul(oracle, a, b, elem_level):
    return oracle.mul(a, b) if elem_level == 7 else oracle.gf_mul(a, b, elem_level)


def _coeffs(oracle, seed, n, elem_level):
    """n random elements of the level as Python ints, and the same as the array the oracle transforms."""
    if elem_level == 7:
        data = oracle.random_b128(seed, n)
        return oracle.arr_to_ints(data), data
    data = oracle.splitmix_words(seed, n).astype(DT[elem_level])
    return [int(x) for x in data], data


def _ints(oracle, data, elem_level):
    return oracle.arr_to_ints(data) if elem_level == 7 else [int(x) for x in data]


def _direct_eval(oracle, basis, coeffs, elem_level, tw_level):
    """evals[k] = sum_j coeffs[j] * X_j(omega_k), X_j = prod_{bit i of j} W^_i: the points and every W^_i(omega_k) in the twiddle field
    (pins._w_hat at tw_level), the products with the coefficient in the element field."""
    d = len(basis)
    pts = pins._span(basis)  # pts[k] = sum_b bit_b(k) basis[b]
    out = []
    for k in range(1 << d):
        wh = [pins._w_hat(oracle, basis, i, pts[k], tw_level) for i in range(d)]
        assert all(w < (1 << (1 << tw_level)) for w in wh)
        acc = 0
        for j, c in enumerate(coeffs):
            x = c
            for i in range(d):
                if (j >> i) & 1:
                    x = _elem_mul(oracle, x, wh[i], elem_level)
            acc ^= x
        out.append(acc)
    return out


PAIRS = [(3, 3), (4, 3), (5, 3), (5, 4), (6, 4), (6, 6), (7, 3), (7, 5), (7, 6)]


@pytest.mark.parametrize("extra", [0, 2])
@pytest.mark.parametrize("log_y", [4, 5])
@pytest.mark.parametrize("elem_level,tw_level", PAIRS)
def test_forward_ntt_is_novel_basis_evaluation_for_mixed_pairs(oracle, elem_level, tw_level, log_y, extra):
    log_domain = log_y + extra
    s = oracle.ntt_s_evals(tw_level, log_domain)
    stride = _stride(s)
    coeffs, data = _coeffs(oracle, 0x4E5450 + 16 * elem_level + tw_level + log_y, 1 << log_y, elem_level)
    assert oracle.ntt_forward(data, elem_level, tw_level, s, log_domain, 0, log_y, 0) == 0
    # domain S^(l-k): basis W^_{l-k}(beta_{l-k}), W^_{l-k}(beta_{l-k+1}), ... = (1, s_evals[l-k][0], ...)
    basis = [1] + [int(s[extra * stride + b]) for b in range(log_y - 1)]
    if extra == 0:
        assert basis == [1 << k for k in range(log_y)]
    assert _ints(oracle, data, elem_level) == _direct_eval(oracle, basis, coeffs, elem_level, tw_level)
    assert oracle.ntt_inverse(data, elem_level, tw_level, s, log_domain, 0, log_y, 0) == 0
    assert _ints(oracle, data, elem_level) == coeffs


# ---- batch, coset, skip_rounds in terms of the plain transform, at B64 elements with B16 twiddles
EL, TW = 6, 4


def _fwd(oracle, x, s, log_domain, log_x, log_y, log_z, coset=0, coset_bits=0, skip=0):
    y = np.ascontiguousarray(x).copy()
    assert oracle.ntt_forward(y, EL, TW, s, log_domain, log_x, log_y, log_z, coset, coset_bits, skip) == 0
    return y


def _inv(oracle, x, s, log_domain, log_x, log_y, log_z, coset=0, coset_bits=0, skip=0):
    y = np.ascontiguousarray(x).copy()
    assert oracle.ntt_inverse(y, EL, TW, s, log_domain, log_x, log_y, log_z, coset, coset_bits, skip) == 0
    return y


def test_batches_are_the_transform_column_by_column(oracle):
    """index = x | y << log_x | z << (log_x + log_y): every (x, z) column is transformed on its own."""
    log_domain, log_x, log_y, log_z, coset, coset_bits = 9, 2, 5, 1, 2, 2
    s = oracle.ntt_s_evals(TW, log_domain)
    data = oracle.splitmix_words(0xBA7C, 1 << (log_x + log_y + log_z))
    cube = data.reshape(1 << log_z, 1 << log_y, 1 << log_x)
    want_f, want_i = np.zeros_like(cube), np.zeros_like(cube)
    for z in range(1 << log_z):
        for x in range(1 << log_x):
            want_f[z, :, x] = _fwd(oracle, cube[z, :, x], s, log_domain, 0, log_y, 0, coset, coset_bits)
            want_i[z, :, x] = _inv(oracle, cube[z, :, x], s, log_domain, 0, log_y, 0, coset, coset_bits)
    assert np.array_equal(_fwd(oracle, data, s, log_domain, log_x, log_y, log_z, coset, coset_bits), want_f.reshape(-1))
    assert np.array_equal(_inv(oracle, data, s, log_domain, log_x, log_y, log_z, coset, coset_bits), want_i.reshape(-1))
    assert not np.array_equal(want_f.reshape(-1), data)


@pytest.mark.parametrize("coset,coset_bits", [(1, 1), (2, 2), (5, 3)])
def test_coset_transform_is_a_slice_of_the_transform_of_the_larger_size(oracle, coset, coset_bits):
    """A polynomial of 2^log_y coefficients evaluated on coset c of the domain of 2^(log_y + coset_bits) points: the coefficients padded
    with zeros, transformed at the larger size, evaluations c * 2^log_y .. (c + 1) * 2^log_y."""
    log_y = 5
    log_domain = log_y + coset_bits + 1
    s = oracle.ntt_s_evals(TW, log_domain)
    data = oracle.splitmix_words(0xC05E + coset, 1 << log_y)
    padded = np.zeros(1 << (log_y + coset_bits), dtype=np.uint64)
    padded[: 1 << log_y] = data
    big = _fwd(oracle, padded, s, log_domain, 0, log_y + coset_bits, 0)
    got = _fwd(oracle, data, s, log_domain, 0, log_y, 0, coset, coset_bits)
    assert np.array_equal(got, big[coset << log_y : (coset + 1) << log_y])
    assert np.array_equal(_inv(oracle, got, s, log_domain, 0, log_y, 0, coset, coset_bits), data)


@pytest.mark.parametrize("skip", [1, 2, 4])
def test_skip_rounds_leaves_independent_transforms_over_cosets(oracle, skip):
    """skip_rounds = s: 2^s transforms of size log_y - s, part c over coset c (of a coset (c0, b0): over coset c0 << s | c)."""
    log_y, log_domain = 6, 8
    s = oracle.ntt_s_evals(TW, log_domain)
    data = oracle.splitmix_words(0x5C1B + skip, 1 << log_y)
    part = 1 << (log_y - skip)
    for c0, b0 in ((0, 0), (3, 2)):
        got = _fwd(oracle, data, s, log_domain, 0, log_y, 0, c0, b0, skip)
        for c in range(1 << skip):
            want = _fwd(oracle, data[c * part : (c + 1) * part], s, log_domain, 0, log_y - skip, 0, (c0 << skip) | c, b0 + skip)
            assert np.array_equal(got[c * part : (c + 1) * part], want), (c0, c)
        assert np.array_equal(_inv(oracle, got, s, log_domain, 0, log_y, 0, c0, b0, skip), data)


# ---- the library's host-side basis
@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


@pytest.mark.parametrize("tw_level", [3, 4, 5, 6])
def test_library_s_evals_match_the_oracle_at_every_domain_size(ffi, oracle, tw_level):
    for d in range(1, min(1 << tw_level, 64) + 1):
        assert np.array_equal(ffi.ntt_s_evals(tw_level, d), oracle.ntt_s_evals(tw_level, d)), (tw_level, d)
    for d in (0, min(1 << tw_level, 64) + 1):
        with pytest.raises(ffi.BnError) as e:
            ffi.ntt_s_evals(tw_level, d)
        assert e.value.kind == "InputValidation"
