"""Pins tests/gkr_exp_ref.py, the CPU restatement of the GKR exponentiation argument that the GPU parity tests compare with (CPU
only): the layers against brute-force scalar exponentiation, exp_prove against exp_verify (which shares no code with it) and against
independent mle_evaluate of the bit and base columns, and exp_verify against tampered proofs."""
import copy

import numpy as np
import pytest

import gkr_exp_ref as R

B8_ELEM = 0x53
FULL_ELEM = 0x0123456789ABCDEFFEDCBA9876543210


def rand_bits(oracle, seed, n):
    return (oracle.splitmix_words(seed, n) & np.uint64(1)).astype(np.uint8)


def scalar_pow(oracle, base, e):
    r = 1
    for _ in range(e):
        r = oracle.mul(r, base)
    return r


def brute_layers(oracle, bits, base, kind):
    """Row by row with scalar products only."""
    w, n = len(bits), len(bits[0])
    bases = [base] * n if isinstance(base, int) else oracle.arr_to_ints(base)
    out = [[0] * n for _ in range(w)]
    for i in range(n):
        if kind == "static":
            v, c = 1, bases[i]
            for k in range(w):
                v = oracle.mul(v, c if bits[k][i] else 1)
                out[k][i] = v
                c = oracle.mul(c, c)
        else:
            v = 1
            for k in range(w):
                v = oracle.mul(oracle.mul(v, v), bases[i] if bits[w - 1 - k][i] else 1)
                out[k][i] = v
    return out


@pytest.mark.parametrize("width", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", ["static", "dynamic"])
def test_layers_equal_brute_force_and_scalar_powers(oracle, kind, width):
    n = 16
    for t, base in enumerate([0, 1, B8_ELEM, FULL_ELEM]):
        bits = [rand_bits(oracle, 0xE100 + 16 * width + k, n) for k in range(width)]
        b = base if kind == "static" else oracle.ints_to_arr([base] * (n - 1) + [FULL_ELEM ^ t])
        layers = R.exp_layers(bits, b, kind)
        want = brute_layers(oracle, bits, b, kind)
        assert [oracle.arr_to_ints(x) for x in layers] == want
        bases = [base] * n if kind == "static" else oracle.arr_to_ints(b)
        for i in range(n):
            e = sum(int(bits[k][i]) << k for k in range(width))
            assert oracle.arr_to_ints(layers[-1])[i] == scalar_pow(oracle, bases[i], e)


@pytest.mark.parametrize("kind", ["static", "dynamic"])
def test_width_128_and_extreme_exponents(oracle, kind):
    n, w = 4, 128
    for base in (0, 1, B8_ELEM, FULL_ELEM):
        b = base if kind == "static" else oracle.ints_to_arr([base] * n)
        for bits in ([np.zeros(n, np.uint8)] * w, [np.ones(n, np.uint8)] * w, [rand_bits(oracle, 0xE200 + k, n) for k in range(w)]):
            layers = R.exp_layers(bits, b, kind)
            assert [oracle.arr_to_ints(x) for x in layers] == brute_layers(oracle, bits, b, kind)
            if not bits[0].any() and not bits[-1].any():
                assert oracle.arr_to_ints(layers[-1]) == [1] * n  # x^0 = 1, 0^0 = 1 included
    # all ones: x^(2^128 - 1) = 1 for x != 0, 0 for x = 0
    ones = [np.ones(n, np.uint8)] * w
    b = FULL_ELEM if kind == "static" else oracle.ints_to_arr([FULL_ELEM] * n)
    assert oracle.arr_to_ints(R.exp_layers(ones, b, kind)[-1]) == [1] * n
    z = 0 if kind == "static" else oracle.ints_to_arr([0] * n)
    assert oracle.arr_to_ints(R.exp_layers(ones, z, kind)[-1]) == [0] * n


# ------------------------------------------------------------------------------------------------ the prover
def make_claims(oracle, shapes, seed, points=None):
    """shapes: [(n_vars, width, kind)].  The claim of a witness is its result layer's evaluation at a point: a random one per n_vars
    (claims of equal n_vars share it), or points[t]."""
    claims, by_n = [], {}
    for t, (n, w, kind) in enumerate(shapes):
        bits = [rand_bits(oracle, seed + 131 * t + k, 1 << n) for k in range(w)]
        base = oracle.random_scalars(seed + 7 * t + 1, 1)[0] if kind == "static" else oracle.random_b128(seed + 7 * t + 2, 1 << n)
        if points is not None:
            pt = points[t]
        else:
            pt = by_n.setdefault(n, oracle.random_scalars(seed + 1000 + n, max(1, n))[:n])
        layers = R.exp_layers(bits, base, kind)
        claims.append({"n_vars": n, "kind": kind, "base": base, "bits": bits, "point": pt, "eval": oracle.mle_evaluate(layers[-1], n, pt)})
    return claims


def samples(oracle, claims, seed):
    max_w = max(len(c["bits"]) for c in claims)
    max_n = max(c["n_vars"] for c in claims)
    flat_c = oracle.random_scalars(seed, max_w * len(claims))
    flat_z = oracle.random_scalars(seed + 1, max(1, max_w * max_n))
    return ([flat_c[L * len(claims) : (L + 1) * len(claims)] for L in range(max_w)], [flat_z[L * max_n : (L + 1) * max_n] for L in range(max_w)])


def meta_of(claims):
    return [{"n_vars": c["n_vars"], "width": len(c["bits"]), "kind": c["kind"], "base": c["base"] if c["kind"] == "static" else None,
             "point": c["point"], "eval": c["eval"]} for c in claims]


def check_claims_against_columns(oracle, claims, layer_claims):
    """Every LayerClaim is the evaluation of a bit column (then, for a dynamic base, of the base column) at its point."""
    live = list(range(len(claims)))
    for L, lc in enumerate(layer_claims):
        at = 0
        for t in live:
            c, w, n = claims[t], len(claims[t]["bits"]), claims[t]["n_vars"]
            k = w - 1 - L if c["kind"] == "static" else L
            pt, ev = lc[at]
            assert len(pt) == n
            assert ev == oracle.mle_evaluate(R.bits_to_b128(c["bits"][k]), n, pt), "layer %d claim %d: not the bit column's evaluation" % (L, t)
            at += 1
            if c["kind"] == "dynamic":
                pt, ev = lc[at]
                assert ev == oracle.mle_evaluate(c["base"], n, pt), "layer %d claim %d: not the base column's evaluation" % (L, t)
                at += 1
        assert at == len(lc)
        live = [t for t in live if len(claims[t]["bits"]) - 1 - L != 0]


MIXED = [(5, 3, "dynamic"), (5, 1, "static"), (3, 4, "static"), (0, 2, "dynamic")]


@pytest.mark.parametrize("shapes", [[(4, 3, "static")], [(4, 3, "dynamic")], [(3, 1, "static")], [(3, 1, "dynamic")], MIXED,
                                    [(4, 2, "static"), (4, 3, "dynamic"), (4, 1, "dynamic"), (2, 5, "static"), (2, 2, "dynamic"), (0, 3, "static")]])
def test_prover_output_passes_the_verifier(oracle, shapes):
    claims = make_claims(oracle, shapes, 0xE300 + len(shapes))
    coeffs, chals = samples(oracle, claims, 0xE400)
    proof = R.exp_prove(claims, coeffs, chals)
    got = R.exp_verify(meta_of(claims), proof, coeffs, chals)
    assert got == proof["layer_claims"]
    check_claims_against_columns(oracle, claims, got)


def test_two_groups_in_layer_0_one_afterwards(oracle):
    n = 4
    pts = [oracle.random_scalars(0xE500, n), oracle.random_scalars(0xE501, n)]
    claims = make_claims(oracle, [(n, 3, "static"), (n, 3, "dynamic")], 0xE510, points=pts)
    coeffs, chals = samples(oracle, claims, 0xE520)
    proof = R.exp_prove(claims, coeffs, chals)
    assert [len(e) for e in proof["multilinear_evals"]] == [2, 1, 1]
    got = R.exp_verify(meta_of(claims), proof, coeffs, chals)
    assert got == proof["layer_claims"]
    check_claims_against_columns(oracle, claims, got)


def test_static_only_batch_has_a_layer_without_sumcheck(oracle):
    claims = make_claims(oracle, [(3, 2, "static"), (3, 2, "static")], 0xE600)
    coeffs, chals = samples(oracle, claims, 0xE610)
    proof = R.exp_prove(claims, coeffs, chals)
    assert proof["round_proofs"][1] == [] and proof["multilinear_evals"][1] == []
    assert R.exp_verify(meta_of(claims), proof, coeffs, chals) == proof["layer_claims"]
    check_claims_against_columns(oracle, claims, proof["layer_claims"])
    # base 1: the last bit's claim is 0 (invert_or_zero)
    one = make_claims(oracle, [(2, 1, "static")], 0xE620)
    one[0]["base"], one[0]["eval"] = 1, 1
    c1, z1 = samples(oracle, one, 0xE630)
    assert R.exp_prove(one, c1, z1)["layer_claims"] == [[(one[0]["point"], 0)]]


def test_tampered_proofs_are_rejected(oracle):
    claims = make_claims(oracle, MIXED, 0xE700)
    coeffs, chals = samples(oracle, claims, 0xE710)
    proof = R.exp_prove(claims, coeffs, chals)
    R.exp_verify(meta_of(claims), proof, coeffs, chals)
    bad = copy.deepcopy(proof)
    bad["round_proofs"][0][1][2] ^= 1
    with pytest.raises(AssertionError):
        R.exp_verify(meta_of(claims), bad, coeffs, chals)
    bad = copy.deepcopy(proof)
    bad["multilinear_evals"][1][0][1] ^= 1
    with pytest.raises(AssertionError):
        R.exp_verify(meta_of(claims), bad, coeffs, chals)
    with pytest.raises(AssertionError):
        R.exp_prove(list(reversed(claims)), coeffs, chals)  # ClaimsOutOfOrder
