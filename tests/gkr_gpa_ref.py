"""CPU restatement of the GKR grand-product argument (core/src/protocols/gkr_gpa): the product circuit's layers
(gkr_gpa.rs:38-90), gkr_gpa::batch_prove (prove.rs:33-296) composed from the oracle's pinned eq-indicator sumcheck
(oracle.zerocheck_ref.eqind_sumcheck_prove) plus the protocol bookkeeping, and gkr_gpa::batch_verify (verify.rs:24-188) as a
checker that shares nothing with the prover.  Pinned by tests/test_gkr_gpa_oracle.py; the GPU parity tests compare with it.

Conventions (all the reference's): layer_j[i] = layer_{j+1}[i] * layer_{j+1}[i + 2^j]; a truncated input counts as followed by
ONEs; states sorted stably by n_vars descending; step j runs ONE eq-indicator sumcheck prover over j variables, High-to-Low, as a
front-loaded batch of one (round proof = the prover's coefficients times the batch coefficient, last coefficient dropped); the
sumcheck challenges are reversed into the next evaluation point, the layer challenge appended."""
import numpy as np

import oracle as o
from oracle.zerocheck_ref import eqind_sumcheck_prove

ONE = 1


def pad_ones(vals, n_vars):
    """The 2^n_vars elements a truncated input stands for."""
    out = o.arr(1 << n_vars)
    out[:, 0] = 1
    n = 0 if vals is None else vals.shape[0]
    assert n <= 1 << n_vars
    if n:
        out[:n] = vals
    return out


def product_layers(vals, n_vars):
    """[layer_0, ..., layer_{n_vars}] as (2^j, 2) uint64 arrays; layer_{n_vars} = the ONE-padded input."""
    layers = [pad_ones(vals, n_vars)]
    for j in range(n_vars - 1, -1, -1):
        top = layers[0]
        half = 1 << j
        layers.insert(0, o.mul_vec(np.ascontiguousarray(top[:half]), np.ascontiguousarray(top[half : 2 * half])))
    return layers


def heap_arena(layers):
    """The layers below the input in heap order: element 2^j + i = element i of layer j (element 0 is not defined: zero here)."""
    n_vars = len(layers) - 1
    out = o.arr(1 << n_vars)
    for j in range(n_vars):
        out[1 << j : 2 << j] = layers[j]
    return out


def line(e0, e1, z):
    return e0 ^ o.mul(z, e1 ^ e0)


def stable_order(n_vars):
    """Indices of the claims sorted stably by n_vars descending (prove.rs:61-62)."""
    return sorted(range(len(n_vars)), key=lambda t: -n_vars[t])


def gpa_prove(inputs, n_vars, batch_coeffs, sumcheck_challenges, gpa_challenges, layers=None):
    """inputs[t]: (len, 2) array or None; batch_coeffs[j], gpa_challenges[j]: one per step j < max n_vars;
    sumcheck_challenges[j]: the j challenges of step j.  Returns a dict:
      products[t]; round_proofs[j] = j lists of 3 coefficients; layer_evals[j] = the 2 * active evaluations then the prefix;
      final_points[t] (n_vars[t] coordinates), final_evals[t] -- in the callers' order."""
    k = len(n_vars)
    if layers is None:
        layers = [product_layers(inputs[t], n_vars[t]) for t in range(k)]
    products = [o.arr_to_ints(layers[t][0])[0] for t in range(k)]
    order = stable_order(n_vars)
    layer_eval = list(products)
    final_points, final_evals = [None] * k, [None] * k
    eval_point, round_proofs, layer_evals = [], [], []
    max_n = max(n_vars) if k else 0
    for j in range(max_n + 1):
        for t in order:
            if n_vars[t] == j:
                final_points[t], final_evals[t] = list(eval_point), layer_eval[t]
        active = [t for t in order if n_vars[t] > j]
        if not active:
            break
        c, g = batch_coeffs[j], gpa_challenges[j]
        mls = []
        for t in active:
            L = layers[t][j + 1]
            mls += [np.ascontiguousarray(L[: 1 << j]), np.ascontiguousarray(L[1 << j :])]
        if j == 0:
            finals, proofs, ch = [o.arr_to_ints(x)[0] for x in mls] + [ONE], [], []
        else:
            comps = [([("var", 2 * i), ("var", 2 * i + 1), ("mul", 0, 1)],) * 2 for i in range(len(active))]
            ch = list(sumcheck_challenges[j])
            assert len(ch) == j
            coeffs, finals = eqind_sumcheck_prove(mls, j, comps, [layer_eval[t] for t in active], eval_point, c, ch)
            proofs = [[o.mul(v, c) for v in rc[:-1]] for rc in coeffs]
        round_proofs.append(proofs)
        layer_evals.append(finals)
        eval_point = ch[::-1] + [g]
        for i, t in enumerate(active):
            layer_eval[t] = line(finals[2 * i], finals[2 * i + 1], g)
    return {"products": products, "round_proofs": round_proofs, "layer_evals": layer_evals, "final_points": final_points, "final_evals": final_evals}


def eq_eval(x, y):
    """eq(x, y) = prod (x_i y_i + (1 - x_i)(1 - y_i))."""
    r = 1
    for a, b in zip(x, y):
        r = o.mul(r, 1 ^ a ^ b)
    return r


def gpa_verify(n_vars, products, proof, batch_coeffs, sumcheck_challenges, gpa_challenges):
    """gkr_gpa::batch_verify (verify.rs:24-188) with the front-loaded sumcheck verifier for one claim per step: raises
    AssertionError where the verifier would reject; returns (final_points, final_evals) in the callers' order."""
    k = len(n_vars)
    order = stable_order(n_vars)
    cur = list(products)
    points, evals = [None] * k, [None] * k
    point = []
    max_n = max(n_vars) if k else 0
    for j in range(max_n + 1):
        for t in order:
            if n_vars[t] == j:
                points[t], evals[t] = list(point), cur[t]
        active = [t for t in order if n_vars[t] > j]
        if not active:
            break
        c, g = batch_coeffs[j], gpa_challenges[j]
        # the batched claim: c * sum_i c^i eval_i
        claim, scale = 0, c
        for t in active:
            claim ^= o.mul(scale, cur[t])
            scale = o.mul(scale, c)
        ch = list(sumcheck_challenges[j]) if j else []
        assert len(proof["round_proofs"][j]) == j
        for r in range(j):
            c0, c1, c2 = proof["round_proofs"][j][r]
            c3 = claim ^ c1 ^ c2  # P(0) + P(1) = claim: c0 + (c0 + c1 + c2 + c3) = claim
            claim = o.evaluate_univariate([c0, c1, c2, c3], ch[r])
        fin = proof["layer_evals"][j]
        assert len(fin) == 2 * len(active) + 1
        rev = ch[::-1]
        want, scale = 0, c
        for i in range(len(active)):
            want ^= o.mul(scale, o.mul(fin[2 * i], fin[2 * i + 1]))
            scale = o.mul(scale, c)
        ind = eq_eval(point, rev)
        assert fin[-1] == ind, "step %d: the indicator's evaluation is not eq(point, challenges)" % j
        assert o.mul(want, ind) == claim, "step %d: the final sumcheck claim does not match the layer evaluations" % j
        point = rev + [g]
        for i, t in enumerate(active):
            cur[t] = line(fin[2 * i], fin[2 * i + 1], g)
    return points, evals
