"""tests/derive_ref.py pinned by facts that do not come from it (CPU only): vectors written out by hand from validate.rs:177-238 and
fold.rs:52-75 for n_vars = 3, and identities every implementation of the definitions must satisfy."""
import numpy as np
import pytest

import derive_ref as D

V8 = np.array([1, 2, 3, 4, 5, 6, 7, 8], dtype=np.uint8)
V4 = np.array([1, 2, 3, 4], dtype=np.uint8)

# (block_size, shift_offset, variant) -> the column, index by index from the loops of validate.rs
SHIFT_LITERALS = [
    # CircularLeft: out[start + o] = in[start + (o + (B - s)) % B]
    (3, 3, D.CIRCULAR_LEFT, [6, 7, 8, 1, 2, 3, 4, 5]),
    (2, 1, D.CIRCULAR_LEFT, [4, 1, 2, 3, 8, 5, 6, 7]),
    (1, 1, D.CIRCULAR_LEFT, [2, 1, 4, 3, 6, 5, 8, 7]),
    # LogicalLeft: zero for o < s, in[start + o - s] from there
    (3, 3, D.LOGICAL_LEFT, [0, 0, 0, 1, 2, 3, 4, 5]),
    (2, 1, D.LOGICAL_LEFT, [0, 1, 2, 3, 0, 5, 6, 7]),
    (3, 7, D.LOGICAL_LEFT, [0, 0, 0, 0, 0, 0, 0, 1]),
    # LogicalRight: in[start + o + s] for o < B - s, zero from there
    (3, 3, D.LOGICAL_RIGHT, [4, 5, 6, 7, 8, 0, 0, 0]),
    (2, 1, D.LOGICAL_RIGHT, [2, 3, 4, 0, 6, 7, 8, 0]),
    (3, 7, D.LOGICAL_RIGHT, [8, 0, 0, 0, 0, 0, 0, 0]),
]

# (n_pad_vars, start_index, nonzero_index) on the inner [1, 2, 3, 4] -> the column of 2^3 values, index by index from fold.rs:57-76
PAD_LITERALS = [
    (1, 0, 0, [1, 0, 2, 0, 3, 0, 4, 0]),
    (1, 0, 1, [0, 1, 0, 2, 0, 3, 0, 4]),
    (1, 1, 0, [1, 2, 0, 0, 3, 4, 0, 0]),
    (1, 1, 1, [0, 0, 1, 2, 0, 0, 3, 4]),
    (1, 2, 0, [1, 2, 3, 4, 0, 0, 0, 0]),
    (1, 2, 1, [0, 0, 0, 0, 1, 2, 3, 4]),
]


@pytest.mark.parametrize("block_size,shift_offset,variant,want", SHIFT_LITERALS)
def test_shift_literals(block_size, shift_offset, variant, want):
    assert D.shifted(V8, block_size, shift_offset, variant).tolist() == want


@pytest.mark.parametrize("n_pad_vars,start_index,nonzero_index,want", PAD_LITERALS)
def test_zero_pad_literals(n_pad_vars, start_index, nonzero_index, want):
    assert D.zero_padded(V4, n_pad_vars, start_index, nonzero_index).tolist() == want


def test_zero_pad_by_two_variables_literal():
    # two values, start_index 1, four times as long: the pair sits in quarter `nonzero_index` of the one row
    v = np.array([7, 9], dtype=np.uint8)
    assert D.zero_padded(v, 2, 1, 2).tolist() == [0, 0, 0, 0, 7, 9, 0, 0]
    # start_index 0: each value alone in its row of four
    assert D.zero_padded(v, 2, 0, 3).tolist() == [0, 0, 0, 7, 0, 0, 0, 9]


@pytest.mark.parametrize("level", D.LEVELS)
def test_shift_identities(level):
    rng = np.random.default_rng(100 + level)
    n_vars = 7
    v = D.random_values(rng, level, n_vars)
    for b in (1, 3, 7):
        block = 1 << b
        for a in sorted({1, block // 2, block - 1} - {0}):
            # CircularLeft by a, then by 2^b - a: the identity
            once = D.shifted(v, b, a, D.CIRCULAR_LEFT)
            assert np.array_equal(D.shifted(once, b, block - a, D.CIRCULAR_LEFT), v)
            # LogicalLeft then LogicalRight by a: exactly the top a values of every block are zeroed
            back = D.shifted(D.shifted(v, b, a, D.LOGICAL_LEFT), b, a, D.LOGICAL_RIGHT)
            want = v.copy()
            want[(np.arange(1 << n_vars) & (block - 1)) >= block - a] = 0
            assert np.array_equal(back, want)
            # the circular shift is a permutation inside blocks; the logical ones agree with it where they are not zero
            left = D.shifted(v, b, a, D.LOGICAL_LEFT)
            keep = (np.arange(1 << n_vars) & (block - 1)) >= a
            assert np.array_equal(left[keep], once[keep]) and not left[~keep].any()


@pytest.mark.parametrize("level", D.LEVELS)
def test_trivial_repeat_and_pad_are_the_identity(level):
    rng = np.random.default_rng(200 + level)
    v = D.random_values(rng, level, 6)
    assert np.array_equal(D.repeating(v, 6), v)  # log_count = 0
    for start_index in (0, 3, 6):
        assert np.array_equal(D.zero_padded(v, 0, start_index, 0), v)  # n_pad_vars = 0
    r = D.repeating(v, 8)
    assert all(np.array_equal(r[k << 6:(k + 1) << 6], v) for k in range(4))


def test_a_byte_shift_is_a_bit_shift_by_eight():
    rng = np.random.default_rng(7)
    v = D.random_values(rng, 3, 6)
    bits = np.unpackbits(v, bitorder="little")
    for variant in (D.CIRCULAR_LEFT, D.LOGICAL_LEFT, D.LOGICAL_RIGHT):
        for b, s in ((2, 1), (6, 1), (6, 5), (4, 15)):
            as_bytes = D.shifted(v, b, s, variant)
            as_bits = D.shifted(bits, b + 3, 8 * s, variant)
            assert np.array_equal(np.unpackbits(as_bytes, bitorder="little"), as_bits)


def test_pack_round_trip_and_xor():
    rng = np.random.default_rng(9)
    for level in D.LEVELS:
        n_vars = 9 - min(level, 2)
        a, b = D.random_values(rng, level, n_vars), D.random_values(rng, level, n_vars)
        assert np.array_equal(D.unpack(D.pack(a, level), level, n_vars), a)
        # a column that appears twice cancels; the constant column is the offset
        off = (0x5A5A5A5A5A5A5A5AA5A5A5A5A5A5A5A5 >> 3) & ((1 << (1 << level)) - 1)
        assert np.array_equal(D.xor_combination([a, b, a], off, level, n_vars), b ^ D.constant(off, level, 1 << n_vars))
        assert np.array_equal(D.pack(D.xor_combination([a, b], 0, level, n_vars), level), D.pack(a, level) ^ D.pack(b, level))
