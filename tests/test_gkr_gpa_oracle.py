"""Pins tests/gkr_gpa_ref.py (the CPU restatement of the GKR grand-product argument) by things that are not the code under
test: (a) gkr_gpa::batch_verify (verify.rs:24-188) restated as a checker accepts every proof; (b) each final claim equals
oracle.mle_evaluate of the ONE-padded input at its point; (c) each product equals the brute-force product; (d) the output is in
the callers' order with mixed n_vars and ties; and the layers are the definition, element by element."""
import numpy as np
import pytest

import gkr_gpa_ref as R

# (n_vars, input_len) per claim: full, truncated, empty, constant, ties in n_vars, smallest and largest first
BATCH = [(5, 32), (3, 5), (7, 100), (0, 1), (5, 0), (1, 2), (7, 128)]


def make_inputs(oracle, shapes, seed):
    return [oracle.random_b128(seed + 17 * t, ln) if ln else None for t, (_, ln) in enumerate(shapes)]


def transcript(oracle, n_vars, seed):
    m = max(n_vars)
    bc = oracle.random_scalars(seed, m)
    gc = oracle.random_scalars(seed + 1, m)
    flat = oracle.random_scalars(seed + 2, m * (m - 1) // 2 + 1)
    sc, off = [], 0
    for j in range(m):
        sc.append(flat[off : off + j])
        off += j
    return bc, sc, gc


def brute_product(oracle, vals):
    r = 1
    for v in oracle.arr_to_ints(vals) if vals is not None else []:
        r = oracle.mul(r, v)
    return r


def check_proof(oracle, shapes, inputs, proof, bc, sc, gc):
    n_vars = [n for n, _ in shapes]
    points, evals = R.gpa_verify(n_vars, proof["products"], proof, bc, sc, gc)
    assert points == proof["final_points"] and evals == proof["final_evals"]
    for t, (n, _) in enumerate(shapes):
        assert len(points[t]) == n
        assert evals[t] == oracle.mle_evaluate(R.pad_ones(inputs[t], n), n, points[t]), "claim %d: the final claim is not the input's evaluation" % t


def test_layers_are_the_definition(oracle):
    for n, ln in [(4, 16), (4, 11), (3, 0), (0, 1), (0, 0), (1, 1)]:
        vals = oracle.random_b128(0x6B00 + n + ln, ln) if ln else None
        layers = R.product_layers(vals, n)
        assert len(layers) == n + 1
        top = oracle.arr_to_ints(R.pad_ones(vals, n))
        assert oracle.arr_to_ints(layers[n]) == top and all(v == 1 for v in top[ln:])
        for j in range(n):
            up = oracle.arr_to_ints(layers[j + 1])
            assert oracle.arr_to_ints(layers[j]) == [oracle.mul(up[i], up[i + (1 << j)]) for i in range(1 << j)]
        assert oracle.arr_to_ints(layers[0])[0] == brute_product(oracle, vals)
        arena = R.heap_arena(layers)
        for j in range(n):
            assert np.array_equal(arena[1 << j : 2 << j], layers[j])


def test_batch_passes_the_verifier(oracle):
    inputs = make_inputs(oracle, BATCH, 0x6C00)
    n_vars = [n for n, _ in BATCH]
    bc, sc, gc = transcript(oracle, n_vars, 0x6C80)
    proof = R.gpa_prove(inputs, n_vars, bc, sc, gc)
    assert proof["products"] == [brute_product(oracle, x) for x in inputs]
    assert [len(p) for p in proof["round_proofs"]] == list(range(max(n_vars)))
    assert all(len(r) == 3 for p in proof["round_proofs"] for r in p)
    check_proof(oracle, BATCH, inputs, proof, bc, sc, gc)


def test_output_is_in_the_callers_order(oracle):
    """Permuting the claims permutes the per-claim outputs the same way when the sorted order is unchanged (a tie swapped
    changes the claim's place in the batch, so only swaps across different n_vars are compared), and every order verifies."""
    shapes = [(2, 3), (4, 16), (2, 4), (3, 8), (4, 9)]
    inputs = make_inputs(oracle, shapes, 0x6D00)
    n_vars = [n for n, _ in shapes]
    bc, sc, gc = transcript(oracle, n_vars, 0x6D80)
    base = R.gpa_prove(inputs, n_vars, bc, sc, gc)
    check_proof(oracle, shapes, inputs, base, bc, sc, gc)
    assert R.stable_order(n_vars) == [1, 4, 3, 0, 2]
    perm = [3, 1, 0, 4, 2]  # keeps 1 before 4 and 0 before 2: the same sorted sequence of claims
    p_shapes, p_inputs = [shapes[i] for i in perm], [inputs[i] for i in perm]
    moved = R.gpa_prove(p_inputs, [n for n, _ in p_shapes], bc, sc, gc)
    check_proof(oracle, p_shapes, p_inputs, moved, bc, sc, gc)
    assert moved["round_proofs"] == base["round_proofs"] and moved["layer_evals"] == base["layer_evals"]
    for key in ("products", "final_points", "final_evals"):
        assert moved[key] == [base[key][i] for i in perm]


@pytest.mark.parametrize("k,n", [(1, 1), (3, 2), (1, 6), (3, 6)])
def test_equal_sized_batches_pass_the_verifier(oracle, k, n):
    shapes = [(n, 1 << n)] * k
    inputs = make_inputs(oracle, shapes, 0x6E00 + 8 * n + k)
    bc, sc, gc = transcript(oracle, [n] * k, 0x6E80 + n)
    proof = R.gpa_prove(inputs, [n] * k, bc, sc, gc)
    check_proof(oracle, shapes, inputs, proof, bc, sc, gc)


def test_verifier_rejects_a_wrong_proof(oracle):
    shapes = [(3, 8), (2, 3)]
    inputs = make_inputs(oracle, shapes, 0x6F00)
    n_vars = [3, 2]
    bc, sc, gc = transcript(oracle, n_vars, 0x6F80)
    proof = R.gpa_prove(inputs, n_vars, bc, sc, gc)
    bad = dict(proof, products=[proof["products"][0] ^ 1, proof["products"][1]])
    with pytest.raises(AssertionError):
        R.gpa_verify(n_vars, bad["products"], bad, bc, sc, gc)
    bad_evals = [list(x) for x in proof["layer_evals"]]
    bad_evals[2][0] ^= 1
    with pytest.raises(AssertionError):
        R.gpa_verify(n_vars, proof["products"], dict(proof, layer_evals=bad_evals), bc, sc, gc)
