"""The columns of a constraint system that a few integers, one field element or a 0/1 projection determine, restated on unpacked
value arrays (numpy): what bn_generate_columns_batch and the build plan must write.  Written from the definitions, value by value:

  projected_bits   Projected at a hypercube vertex: MultilinearExtension::evaluate_partial (crates/math/src/multilinear_extension.rs:
                   193-237) at a query of ZEROs and ONEs keeps, of the 2^query_size values that differ in the projected variables, the one
                   whose variables equal the query (constraint_system/validate.rs:239-254)
  constant         crates/core/src/transparent/constant.rs
  step_down        step_down.rs:38-70 (populate: ones below index)
  step_up          step_up.rs:39-66 (zeros below index)
  select_row       select_row.rs:37 (one at index)
  incrementing     crates/m3/src/builder/structured.rs:73-81: sum of X_b beta_b, beta_b the b-th basis element over F_2 -- bit b of the value
                   is bit b of the index
  powers           powers.rs:35-57: successive products by the base, starting from ONE

A column is its 2^n_vars values in the conventions of tests/derive_ref.py: a uint8 array of bits (level 0) or bytes (level 3), or an
(N, 2^(level - 3)) uint8 array of little-endian values above.  Nothing here looks at packed words: an index is a value index.
"""
import numpy as np

from univariate_skip_base_ref import pack, unpack  # noqa: F401  (re-exported: the tests pack with the same functions)

LEVELS = (0, 3, 4, 5, 6, 7)


def from_ints(ints, level):
    """Python ints below 2^(2^level) -> a column of the level."""
    if level <= 3:
        return np.array([int(x) for x in ints], dtype=np.uint8)
    w = 1 << (level - 3)
    return np.frombuffer(b"".join(int(x).to_bytes(w, "little") for x in ints), dtype=np.uint8).reshape(len(ints), w).copy()


def to_ints(values):
    v = np.asarray(values, dtype=np.uint8)
    return [int.from_bytes(bytes(row), "little") for row in v.reshape(len(v), -1)]


def random_values(rng, level, n_vars):
    """2^n_vars pseudo-random values of the level from a numpy Generator."""
    n = 1 << n_vars
    if level == 0:
        return rng.integers(0, 2, n, dtype=np.uint8)
    if level == 3:
        return rng.integers(0, 256, n, dtype=np.uint8)
    return rng.integers(0, 256, (n, 1 << (level - 3)), dtype=np.uint8)


def projected_bits(values, start_index, query_size, query_bits):
    v = np.asarray(values)
    inner_n_vars = len(v).bit_length() - 1
    assert query_size >= 1 and start_index + query_size <= inner_n_vars and 0 <= query_bits < 1 << query_size
    i = np.arange(len(v) >> query_size)
    lo, hi = i % (1 << start_index), i >> start_index
    return v[lo + (query_bits << start_index) + (hi << (start_index + query_size))].copy()


def constant(value, level, n_vars):
    assert value >> (1 << level) == 0
    n = 1 << n_vars
    if level <= 3:
        return np.full(n, value, dtype=np.uint8)
    row = np.frombuffer(int(value).to_bytes(1 << (level - 3), "little"), dtype=np.uint8)
    return np.tile(row, (n, 1))


def step_down(n_vars, index):
    assert 0 <= index <= 1 << n_vars
    return (np.arange(1 << n_vars) < index).astype(np.uint8)


def step_up(n_vars, index):
    assert 0 <= index <= 1 << n_vars
    return (np.arange(1 << n_vars) >= index).astype(np.uint8)


def select_row(n_vars, index):
    assert 0 <= index < 1 << n_vars
    return (np.arange(1 << n_vars) == index).astype(np.uint8)


def incrementing(level, n_vars):
    assert n_vars <= 1 << level
    i = np.arange(1 << n_vars, dtype=np.uint64)
    if level == 0:
        return i.astype(np.uint8)
    w = 1 << max(0, level - 3)
    out = np.stack([((i >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8) if b < 8 else np.zeros(len(i), dtype=np.uint8) for b in range(w)], axis=1)
    return out.reshape(-1) if level == 3 else out


def field_mul(a, b, level):
    """The product of two values (ints) of the level's field, by the oracle."""
    import oracle as o

    return o.mul(a, b) if level == 7 else o.gf_mul(a, b, level)


def powers(base, level, n_vars):
    assert 3 <= level <= 7 and base >> (1 << level) == 0
    out, p = [], 1
    for _ in range(1 << n_vars):
        out.append(p)
        p = field_mul(p, base, level)
    return from_ints(out, level)
