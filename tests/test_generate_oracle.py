"""tests/generate_ref.py pinned by facts that do not come from it (CPU only): the hand-written vectors of the reference's own tests
(step_down.rs:127-130 and their analogues), the multilinear extension evaluated by brute force through the oracle's field, and
identities every implementation of the definitions must satisfy."""
import json
import os

import numpy as np
import pytest

import generate_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stepdown_evals(2, index), index 0 .. 4 (step_down.rs:127-132); step-up is its complement (step_up.rs), select-row the unit vector
STEP_DOWN_2 = {0: [0, 0, 0, 0], 1: [1, 0, 0, 0], 2: [1, 1, 0, 0], 3: [1, 1, 1, 0], 4: [1, 1, 1, 1]}
STEP_UP_2 = {0: [1, 1, 1, 1], 1: [0, 1, 1, 1], 2: [0, 0, 1, 1], 3: [0, 0, 0, 1], 4: [0, 0, 0, 0]}
SELECT_ROW_2 = {0: [1, 0, 0, 0], 1: [0, 1, 0, 0], 2: [0, 0, 1, 0], 3: [0, 0, 0, 1]}


@pytest.mark.parametrize("index", sorted(STEP_DOWN_2))
def test_step_literals(index):
    assert G.step_down(2, index).tolist() == STEP_DOWN_2[index]
    assert G.step_up(2, index).tolist() == STEP_UP_2[index]
    assert G.step_down(3, 1).tolist() == [1, 0, 0, 0, 0, 0, 0, 0]  # step_down.rs:137-140


@pytest.mark.parametrize("index", sorted(SELECT_ROW_2))
def test_select_row_literals(index):
    assert G.select_row(2, index).tolist() == SELECT_ROW_2[index]
    with pytest.raises(AssertionError):
        G.select_row(2, 4)  # the strict bound


def _evaluate_partial_brute(oracle, values, query, start_index):
    """MultilinearExtension::evaluate_partial over B8 by its definition: out[lo, hi] = sum over x of eq(query, x) in[lo, x, hi], every
    product the oracle's."""
    m, run = len(query), 1 << start_index
    weights = []
    for x in range(1 << m):
        w = 1
        for k, q in enumerate(query):
            w = oracle.gf_mul(w, q if (x >> k) & 1 else q ^ 1, 3)
        weights.append(w)
    out = []
    for i in range(len(values) >> m):
        lo, hi = i % run, i // run
        acc = 0
        for x in range(1 << m):
            acc ^= oracle.gf_mul(weights[x], int(values[lo + x * run + (hi << (start_index + m))]), 3)
        out.append(acc)
    return out


@pytest.mark.parametrize("start_index,query_size,query_bits", [(0, 1, 0), (0, 1, 1), (1, 2, 2), (2, 2, 1), (0, 3, 5), (3, 3, 7), (4, 2, 3), (1, 1, 1)])
def test_projection_is_the_multilinear_extension_at_the_vertex(oracle, start_index, query_size, query_bits):
    values = G.random_values(np.random.default_rng([7, start_index, query_size]), 3, 6)
    query = [(query_bits >> k) & 1 for k in range(query_size)]
    assert G.projected_bits(values, start_index, query_size, query_bits).tolist() == _evaluate_partial_brute(oracle, values, query, start_index)


@pytest.mark.parametrize("level", G.LEVELS)
def test_projection_edges(level):
    values = G.random_values(np.random.default_rng([8, level]), level, 9)
    for m in (1, 3):
        for bits in (0, (1 << m) - 1, 1):
            assert np.array_equal(G.projected_bits(values, 0, m, bits), values[bits :: 1 << m])  # start_index = 0: a strided slice
            block = len(values) >> m
            assert np.array_equal(G.projected_bits(values, 9 - m, m, bits), values[bits * block : (bits + 1) * block])  # the top variables: a block


@pytest.mark.parametrize("level", [3, 4, 5, 6, 7])
def test_powers_identities(oracle, level):
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "field_kats.json")))
    g = int(kats["multiplicative_generators"][str(1 << level)], 16)
    out = G.to_ints(G.powers(g, level, 6))
    assert out[0] == 1 and out[1] == g
    for i in range(0, 64, 5):
        for j in range(0, 64 - i, 7):
            assert out[i + j] == G.field_mul(out[i], out[j], level), (i, j)
    assert G.to_ints(G.powers(0, level, 3)) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert G.to_ints(G.powers(1, level, 3)) == [1] * 8


def test_powers_of_the_b8_generator_have_order_255(oracle):
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "field_kats.json")))
    g = int(kats["multiplicative_generators"]["8"], 16)
    out = G.to_ints(G.powers(g, 3, 8))
    assert out[255] == 1 and len(set(out[:255])) == 255


@pytest.mark.parametrize("level,n_vars", [(0, 1), (3, 8), (4, 10), (5, 12), (6, 12), (7, 12)])
def test_incrementing_unpacks_to_the_index(level, n_vars):
    col = G.incrementing(level, n_vars)
    assert G.to_ints(col) == list(range(1 << n_vars))
    packed = G.pack(col, level)
    assert np.array_equal(G.unpack(packed, level, n_vars), col)
    with pytest.raises(AssertionError):
        G.incrementing(level, (1 << level) + 1)


@pytest.mark.parametrize("level", G.LEVELS)
def test_constant_is_the_value_everywhere(level):
    value = (1 << (1 << level)) - 1
    assert G.to_ints(G.constant(value, level, 4)) == [value] * 16
    assert G.to_ints(G.constant(0, level, 4)) == [0] * 16
