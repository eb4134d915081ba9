"""The virtual columns of a constraint system, restated on unpacked value arrays (numpy): what bn_derive_columns_batch and the witness
plan must write.  Written from the definitions, value by value:

  Shifted                crates/core/src/constraint_system/validate.rs:177-238 (conditions: oracle/multilinear.rs:805-816)
  Repeating              validate.rs:167-176
  ZeroPadded             crates/math/src/fold.rs:52-75 (MultilinearExtension::zero_pad)
  LinearCombination      validate.rs:151-166 with every coefficient ONE: a sum in characteristic two is an XOR

A column is its 2^n_vars values: a uint8 array of bits (level 0) or bytes (level 3), or an (N, 2^(level - 3)) uint8 array of
little-endian values above (the conventions of tests/univariate_skip_base_ref.py, whose pack / unpack put them into 16-byte elements).
Nothing here looks at packed words: an index is a value index.
"""
import numpy as np

from univariate_skip_base_ref import pack, unpack  # noqa: F401  (re-exported: the tests pack with the same functions)

CIRCULAR_LEFT, LOGICAL_LEFT, LOGICAL_RIGHT = 0, 1, 2
LEVELS = (0, 3, 4, 5, 6, 7)


def random_values(rng, level, n_vars):
    """2^n_vars pseudo-random values of the level from a numpy Generator."""
    n = 1 << n_vars
    if level == 0:
        return rng.integers(0, 2, n, dtype=np.uint8)
    if level == 3:
        return rng.integers(0, 256, n, dtype=np.uint8)
    return rng.integers(0, 256, (n, 1 << (level - 3)), dtype=np.uint8)


def constant(value, level, n):
    """n copies of the int `value` (below 2^(2^level)) as a column of the level."""
    assert value >> (1 << level) == 0
    if level <= 3:
        return np.full(n, value, dtype=np.uint8)
    row = np.frombuffer(int(value).to_bytes(1 << (level - 3), "little"), dtype=np.uint8)
    return np.tile(row, (n, 1))


def shifted(values, block_size, shift_offset, variant):
    v = np.asarray(values)
    n, block = len(v), 1 << block_size
    assert block <= n and 1 <= shift_offset < block
    i = np.arange(n)
    o = i & (block - 1)
    start = i - o
    if variant == CIRCULAR_LEFT:
        return v[start + (o + (block - shift_offset)) % block].copy()
    if variant == LOGICAL_LEFT:
        src, ok = o - shift_offset, o >= shift_offset
    else:
        assert variant == LOGICAL_RIGHT
        src, ok = o + shift_offset, o < block - shift_offset
    out = v[start + np.where(ok, src, 0)].copy()
    out[~ok] = 0
    return out


def repeating(values, n_vars):
    v = np.asarray(values)
    assert len(v) <= 1 << n_vars
    return v[np.arange(1 << n_vars) % len(v)].copy()


def zero_padded(values, n_pad_vars, start_index, nonzero_index):
    v = np.asarray(values)
    inner_n_vars = len(v).bit_length() - 1
    assert start_index <= inner_n_vars and nonzero_index < 1 << n_pad_vars
    j = np.arange(len(v) << n_pad_vars)
    per_row = 1 << (start_index + n_pad_vars)
    col, row = j % per_row, j // per_row
    first = nonzero_index << start_index
    ok = (col >= first) & (col < first + (1 << start_index))
    out = v[np.where(ok, (row << start_index) + col - first, 0)].copy()
    out[~ok] = 0
    return out


def xor_combination(terms, offset, level, n_vars):
    out = constant(offset, level, 1 << n_vars)
    for t in terms:
        out = out ^ np.asarray(t)
    return out
