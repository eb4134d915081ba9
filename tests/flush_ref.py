"""TEST INFRASTRUCTURE: CPU restatement of the flush witnesses of the constraint-system prover's product check, over the oracle's pinned
field (oracle.mul_vec).  Restated from the reference, no text of it copied:

  selector_prefix   count_zero_suffixes                core/src/constraint_system/prove.rs:883-902 (at a 128-bit underlier)
  flush_witness     make_masked_flush_witnesses        core/src/constraint_system/prove.rs:671-881
  mixing_terms      the mixing powers by entry position, constants folded into one term   prove.rs:744-771
  flush_prodcheck_prove   the product-check phase  prove.rs:276-428: the witnesses above, gkr_gpa::batch_prove (gkr_gpa_ref.gpa_prove) over
                    chain(flushes, non-zero oracles), reduce_flush_evalcheck_claims (prove.rs:1017-1117) with the composite oracle
                    1 + S * L of constraint_system/verify.rs:519-571, ConstraintSetBuilder::build_one's sorted de-duplicated union
                    (oracle/constraint.rs:114-129) and one eq-indicator sumcheck per group (oracle.zerocheck_ref.eqind_sumcheck_prove) as a
                    front-loaded batch of one (evalcheck/subclaims.rs:589-633)
  mlecheck_verify   the verifier's equations of such an MLE-check, sharing nothing with the prover but composite_steps

Conventions: a selector is an array of 0/1 bytes, one per row; a column is (values, level): for level <= 6 a uint64 array of
2^n_vars values below 2^(2^level), for level 7 an (2^n_vars, 2) uint64 array.  A subfield value embeds into B128 as the identity on
the low bits.  Pinned by tests/test_flush_oracle.py; the GPU parity tests compare with it."""
import numpy as np

import oracle as o

ONE = 1
LEVELS = (0, 3, 4, 5, 6, 7)


def pack_bits(bits):
    """A bit column packed into 16-byte elements: bit i = bit i & 127 of element i >> 7, little-endian; at least one element."""
    b = np.asarray(bits, dtype=np.uint8)
    padded = np.zeros(max(128, b.shape[0]), dtype=np.uint8)
    padded[: b.shape[0]] = b
    return np.packbits(padded, bitorder="little").view(np.uint64).reshape(-1, 2).copy()


def pack_column(values, level):
    """A column of level-`level` values packed into 16-byte elements as the device takes it (at least one element, zero padded)."""
    if level == 0:
        return pack_bits(values)
    if level == 7:
        return np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 2).copy()
    dt = {3: np.uint8, 4: np.uint16, 5: np.uint32, 6: np.uint64}[level]
    raw = np.asarray(values, dtype=np.uint64).astype(dt).view(np.uint8)
    padded = np.zeros(max(16, raw.shape[0]), dtype=np.uint8)
    padded[: raw.shape[0]] = raw
    return padded.view(np.uint64).reshape(-1, 2).copy()


def embed(values, level):
    """The column's values as B128 elements, an (n, 2) array."""
    if level == 7:
        return np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 2)
    out = o.arr(len(values))
    out[:, 0] = np.asarray(values, dtype=np.uint64)
    return out


def random_column(seed, n, level):
    """n SplitMix64 values of the level."""
    if level == 7:
        return o.random_b128(seed, n)
    w = o.splitmix_words(seed, n)
    return w if level == 6 else w & np.uint64((1 << (1 << level)) - 1)


def selector_prefix(bits, n_vars):
    """128 * (1 + index of the last non-zero 16-byte element of the packed selector), 0 if there is none, clipped to 2^n_vars."""
    packed = pack_bits(bits)
    nz = np.flatnonzero((packed[:, 0] != 0) | (packed[:, 1] != 0))
    if nz.size == 0:
        return 0
    return min(128 * (1 + int(nz[-1])), 1 << n_vars)


def broadcast(c, n):
    out = o.arr(n)
    out[:, 0] = c & o.MASK64
    out[:, 1] = (c >> 64) & o.MASK64
    return out


def flush_witness(n_vars, selectors, columns, const_term):
    """selectors: 0/1 arrays; columns: [(values, level, coefficient)].  Returns (prefix_len, witness): the witness as a
    (2^n_vars, 2) array whose rows at and beyond prefix_len are ONE (what the truncated witness stands for)."""
    rows = 1 << n_vars
    prefix = min([selector_prefix(s, n_vars) for s in selectors] + [rows])
    acc = broadcast(const_term, rows)
    for values, level, coeff in columns:
        acc ^= o.mul_vec(broadcast(coeff, rows), np.ascontiguousarray(embed(values, level)))
    on = np.ones(rows, dtype=bool)
    for s in selectors:
        on &= np.asarray(s, dtype=np.uint8).astype(bool)
    on[prefix:] = False
    out = broadcast(ONE, rows)
    out[on] = acc[on]
    return prefix, out


def mixing_terms(entries, mixing_challenge, permutation_challenge):
    """entries: ("oracle", ...) or ("const", base) in the flush's order.  Entry k carries the power alpha^k whatever its kind.
    Returns (const_term, [alpha^k of the oracle entries in order]): const_term = r_channel + sum over the constants of
    base * alpha^k."""
    const_term, coeffs, power = permutation_challenge, [], 1
    for e in entries:
        if e[0] == "const":
            const_term ^= o.mul(e[1], power)
        else:
            coeffs.append(power)
        power = o.mul(power, mixing_challenge)
    return const_term, coeffs


def product(arr):
    """The product of all elements of an (n, 2) array, n a power of two."""
    cur = np.ascontiguousarray(arr)
    while cur.shape[0] > 1:
        h = cur.shape[0] // 2
        cur = o.mul_vec(np.ascontiguousarray(cur[:h]), np.ascontiguousarray(cur[h:]))
    return o.arr_to_ints(cur)[0]


# ---------------------------------------------------------------------------------------------- the product-check phase
def composite_steps(selector_vars, column_vars, coeffs, const_term):
    """The composite flush oracle 1 + prod selectors * (const_term + 1 + sum coeff_j x_j) (constraint_system/verify.rs:519-571) and its
    leading form prod selectors * sum coeff_j x_j as step lists for oracle.make_steps; *_vars: variable indices."""
    def build(leading):
        steps = []

        def push(s):
            steps.append(s)
            return len(steps) - 1

        sel = push(("var", selector_vars[0]))
        for v in selector_vars[1:]:
            sel = push(("mul", sel, push(("var", v))))
        lin = None if leading else push(("const", const_term ^ ONE))
        for v, c in zip(column_vars, coeffs):
            term = push(("mul", push(("var", v)), push(("const", c))))
            lin = term if lin is None else push(("add", lin, term))
        prod = push(("mul", sel, lin))
        if not leading:
            push(("add", push(("const", ONE)), prod))
        return steps

    return build(False), build(True)


def flush_groups(flushes):
    """reduce_flush_evalcheck_claims' grouping as far as it can be known ahead (prove.rs:1045-1073): the composite flushes by n_vars
    -- claims of equal n_vars leave the grand-product argument with the same point -- in order of first appearance, with the sorted,
    de-duplicated union of their oracle ids (oracle/constraint.rs:114-129).  [(n_vars, [flush indices], ids)]"""
    out = []
    for f, fl in enumerate(flushes):
        if not fl["selectors"]:
            continue
        g = next((g for g in out if g[0] == fl["n_vars"]), None)
        if g is None:
            g = (fl["n_vars"], [], [])
            out.append(g)
        g[1].append(f)
        g[2].extend([s[0] for s in fl["selectors"]] + [e[1] for e in fl["entries"] if e[0] == "oracle"])
    return [(n, fs, sorted(set(ids))) for n, fs, ids in out]


class ZerosError(Exception):
    """Error::Zeros (prove.rs:311-316)."""


def flush_prodcheck_prove(flushes, nonzero, mixing_challenge, permutation_challenges, gpa_batch_coeffs, gpa_sumcheck_challenges, gpa_challenges,
                          red_batch_coeffs, red_challenges):
    """The product-check phase (prove.rs:276-428) on host data.  flushes: dicts {"channel", "n_vars", "selectors": [(id, 0/1 array)],
    "entries": [("oracle", id, values, level) | ("const", base)]}; nonzero: [(id, values, level, n_vars)].  Returns
    {"prefix_lens", "gpa": gkr_gpa_ref.gpa_prove's dict over chain(flushes, non-zero), "checks": [{"n_vars", "ids", "round_proofs",
    "final_evals" (the indicator's last)}], "linear_flushes"}."""
    import gkr_gpa_ref as G
    from oracle.zerocheck_ref import eqind_sumcheck_prove

    nz_wit = [np.ascontiguousarray(embed(v, level)) for _, v, level, _ in nonzero]
    if any(product(w) == 0 for w in nz_wit):
        raise ZerosError()
    inputs, n_vars, terms, prefix_lens = [], [], [], []
    for fl in flushes:
        const_term, coeffs = mixing_terms(fl["entries"], mixing_challenge, permutation_challenges[fl["channel"]])
        cols = [(e[2], e[3], c) for e, c in zip([e for e in fl["entries"] if e[0] == "oracle"], coeffs)]
        prefix, wit = flush_witness(fl["n_vars"], [s[1] for s in fl["selectors"]], cols, const_term)
        inputs.append(np.ascontiguousarray(wit[:prefix]) if prefix else None)
        n_vars.append(fl["n_vars"])
        terms.append((const_term, coeffs))
        prefix_lens.append(prefix)
    for (_, _, _, n), w in zip(nonzero, nz_wit):
        inputs.append(w)
        n_vars.append(n)
    gpa = G.gpa_prove(inputs, n_vars, gpa_batch_coeffs, gpa_sumcheck_challenges, gpa_challenges)
    checks = []
    for g, (n, members, ids) in enumerate(flush_groups(flushes)):
        point = gpa["final_points"][members[0]]
        assert all(gpa["final_points"][f] == point for f in members)
        mls = {}
        for f in members:
            for sid, bits in flushes[f]["selectors"]:
                mls.setdefault(sid, np.ascontiguousarray(embed(np.asarray(bits, dtype=np.uint64), 0)))
            for e in flushes[f]["entries"]:
                if e[0] == "oracle":
                    mls.setdefault(e[1], np.ascontiguousarray(embed(e[2], e[3])))
        comps, sums, degrees = [], [], []
        for f in members:
            fl = flushes[f]
            comps.append(composite_steps([ids.index(s[0]) for s in fl["selectors"]], [ids.index(e[1]) for e in fl["entries"] if e[0] == "oracle"],
                                         terms[f][1], terms[f][0]))
            sums.append(gpa["final_evals"][f])
            degrees.append(len(fl["selectors"]) + 1)
        c = red_batch_coeffs[g]
        if n == 0:
            rounds, finals = [], [o.arr_to_ints(mls[i])[0] for i in ids] + [ONE]
        else:
            coeffs, finals = eqind_sumcheck_prove([mls[i] for i in ids], n, comps, sums, point, c, list(red_challenges[g]), degrees=degrees)
            rounds = [[o.mul(v, c) for v in rc[:-1]] for rc in coeffs]
        checks.append({"n_vars": n, "ids": ids, "round_proofs": rounds, "final_evals": finals})
    return {"prefix_lens": prefix_lens, "gpa": gpa, "checks": checks, "linear_flushes": [f for f, fl in enumerate(flushes) if not fl["selectors"]]}


def new_claims(out, red_challenges):
    """The claims the reductions leave: (oracle id, the group's challenges reversed, evaluation); the indicator's evaluation is dropped."""
    claims = []
    for g, chk in enumerate(out["checks"]):
        point = list(red_challenges[g])[::-1] if chk["n_vars"] else []
        claims += [(i, point, e) for i, e in zip(chk["ids"], chk["final_evals"][:-1])]
    return claims


def mlecheck_verify(flushes, terms, chk, members, point, sums, batch_coeff, challenges):
    """The verifier's equations of one front-loaded MLE-check of one prover (sumcheck/verify.rs with eq_ind.rs's verify side): every
    round polynomial -- its last coefficient recovered from P(0) + P(1) = claim -- is evaluated at the challenge; the last claim must be
    the batched composition of the final evaluations times the indicator's evaluation eq(point, reversed challenges)."""
    import gkr_gpa_ref as G

    n, ids, c = chk["n_vars"], chk["ids"], batch_coeff
    claim, scale = 0, c
    for s in sums:
        claim ^= o.mul(scale, s)
        scale = o.mul(scale, c)
    assert len(chk["round_proofs"]) == n
    for r in range(n):
        head = list(chk["round_proofs"][r])
        last = claim ^ head[0]
        for v in head:
            last ^= v  # P(0) + P(1) = c_0 + sum_i c_i
        claim = o.evaluate_univariate(head + [last], challenges[r])
    fin = chk["final_evals"]
    assert len(fin) == len(ids) + 1
    rev = list(challenges)[::-1]
    assert fin[-1] == G.eq_eval(point, rev), "the indicator's evaluation is not eq(point, challenges)"
    want, scale = 0, c
    for f in members:
        fl = flushes[f]
        steps, _ = composite_steps([ids.index(s[0]) for s in fl["selectors"]], [ids.index(e[1]) for e in fl["entries"] if e[0] == "oracle"], terms[f][1], terms[f][0])
        want ^= o.mul(scale, o.circuit_eval(steps, fin[:-1]))
        scale = o.mul(scale, c)
    assert o.mul(want, fin[-1]) == claim, "the final sumcheck claim does not match the final evaluations"
