"""tests/compose_tower_ref.py (the reference of every tower-expression test) pinned by independent definitions: pack_fp is the integer
whose bits are the inputs, a B1 circuit is numpy's & and ^, products agree with the subfield product oracle.gf_mul at every level, and a
product of mixed levels stays in the larger field."""
import numpy as np
import pytest

import compose_tower_ref as T
import oracle as o
import univariate_skip_base_ref as U

N = 256


@pytest.mark.parametrize("level,n_bits", [(5, 32), (6, 64), (3, 8)])
def test_pack_is_the_integer_whose_bits_are_the_inputs(level, n_bits):
    rng = np.random.default_rng([0xC7, level])
    bits = [T.random_values(rng, 0, N) for _ in range(n_bits)]
    steps = T.pack_steps(n_bits)
    assert len(steps) == 4 * n_bits - 1
    got = U.to_ints(T.evaluate(steps, [(b, 0) for b in bits], level))
    want = [sum(int(bits[i][r]) << i for i in range(n_bits)) for r in range(N)]
    assert got == want


def test_b1_circuit_is_and_xor():
    rng = np.random.default_rng(0xB1)
    a, b, s = (T.random_values(rng, 0, N) for _ in range(3))
    steps = [("var", 0), ("var", 1), ("var", 2), ("add", 0, 1), ("mul", 2, 3), ("add", 0, 4)]  # a + s (a + b): mul.rs:466-489
    assert np.array_equal(T.evaluate(steps, [(a, 0), (b, 0), (s, 0)], 0), a ^ (s & (a ^ b)))
    assert np.array_equal(T.evaluate([("var", 0), ("pow", 0, 0)], [(a, 0)], 0), np.ones(N, dtype=np.uint8))
    assert np.array_equal(T.evaluate([("var", 0), ("pow", 0, 5)], [(a, 0)], 0), a)


@pytest.mark.parametrize("level", [3, 4, 5, 6])
def test_products_agree_with_the_subfield_product(level):
    rng = np.random.default_rng([0x6F, level])
    a, b = T.random_values(rng, level, N), T.random_values(rng, level, N)
    got = U.to_ints(T.evaluate([("var", 0), ("var", 1), ("mul", 0, 1)], [(a, level), (b, level)], level))
    assert got == [o.gf_mul(x, y, level) for x, y in zip(U.to_ints(a), U.to_ints(b))]


def test_product_at_b128_is_the_field_product():
    rng = np.random.default_rng(0x7F)
    a, b = T.random_values(rng, 7, 32), T.random_values(rng, 7, 32)
    got = U.to_ints(T.evaluate([("var", 0), ("var", 1), ("mul", 0, 1)], [(a, 7), (b, 7)], 7))
    assert got == [o.mul(x, y) for x, y in zip(U.to_ints(a), U.to_ints(b))]


@pytest.mark.parametrize("lo,hi", [(lo, hi) for hi in T.LEVELS for lo in T.LEVELS if lo < hi])
def test_mixed_level_products_stay_in_the_larger_field(lo, hi):
    rng = np.random.default_rng([0x3D, lo, hi])
    a, b = T.random_values(rng, lo, 64), T.random_values(rng, hi, 64)
    steps = [("var", 0), ("var", 1), ("mul", 0, 1)]
    got = U.to_ints(T.evaluate(steps, [(a, lo), (b, hi)], hi))  # (evaluate asserts that nothing leaves T_hi)
    assert got == [o.mul(x, y) for x, y in zip(U.to_ints(a), U.to_ints(b))]
    assert got == U.to_ints(T.evaluate([("var", 1), ("var", 0), ("mul", 0, 1)], [(a, lo), (b, hi)], hi))
    if hi < 7:
        assert got == [o.gf_mul(x, y, hi) for x, y in zip(U.to_ints(a), U.to_ints(b))]


def test_levels_and_packing():
    assert [T.const_level(c) for c in (0, 1, 2, 3, 4, 15, 16, 255, 256, 1 << 64, (1 << 128) - 1)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 7, 7]
    steps = [("var", 0), ("const", 2), ("mul", 0, 1), ("var", 1), ("add", 2, 3), ("pow", 0, 9)]
    assert T.step_levels(steps, [0, 5]) == [0, 1, 1, 5, 5, 0]
    rng = np.random.default_rng(5)
    for level in T.LEVELS:
        for n_vars in (0, 3, 9):
            v = T.random_values(rng, level, 1 << n_vars)
            p = T.pack(v, level)
            assert p.shape == (max(1, (1 << (n_vars + level)) >> 7), 2)
            assert np.array_equal(T.unpack(p, level, n_vars), v)
