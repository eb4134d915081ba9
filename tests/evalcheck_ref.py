"""CPU restatement of one round of evalcheck's bivariate sumchecks (core/src/protocols/evalcheck/subclaims.rs): the witness construction
(process_shifted_sumcheck / process_packed_sumcheck :52-145, collect_projected_mles :356-439) and one call of
prove_bivariate_sumchecks_with_switchover (:549-586), composed from the oracle's pinned pieces:

  projection          evaluate_partial_high = oracle.fold_left against the tensor expansion of the suffix
  shift indicator     ShiftIndPartialEval::multilinear_extension, the recurrence of transparent/shift_ind.rs:332-366 restated
  tower basis         TowerField::basis(iota, i) = 1 << (i << iota) (transparent/tower_basis.rs:54-70, field/src/binary_field.rs:60-72)
  the batch           oracle.piop_ref.batch_sumcheck_prove (front_loaded.rs:33-203)

and the verifier's side of it (verify) as a checker that shares nothing with the prover.  Pinned by tests/test_evalcheck_oracle.py; the
GPU parity tests compare with it.

A prover is (b, multilins, comps, sums), provers ascending by b.  A multilinear is one of
  ("proj", column, tower_level, n_vars, suffix_off, suffix_len)   column: the packed (N, 2) uint64 array; suffix = pool[off : off + len]
  ("shift", block_size, shift_offset, variant, r_off, r_len)      variant: 0 circular left, 1 logical left, 2 logical right
  ("basis", k, iota)
Everything is High-to-Low: round 0 binds variable b - 1, the final evaluations are at the reversed challenges."""
import numpy as np

import oracle as o
from oracle import piop_ref

CIRCULAR_LEFT, LOGICAL_LEFT, LOGICAL_RIGHT = 0, 1, 2


# ------------------------------------------------------------------------------------------------ the multilinears
def eq_expand(r):
    """eq(r)[y] = prod_k (y_k ? r_k : 1 + r_k)."""
    out = o.arr(1 << len(r))
    out[0] = o.ints_to_arr([1])[0]
    if len(r):
        assert o.tensor_expand(out, 0, list(r)) == 0
    return out


def project(column, tower_level, n_vars, suffix):
    """evaluate_partial_high: the column's high len(suffix) variables bound to the suffix; 2^(n_vars - len(suffix)) B128 elements."""
    out = o.arr(1 << (n_vars - len(suffix)))
    assert o.fold_left(np.ascontiguousarray(column), tower_level, eq_expand(suffix), out) == 0
    return out


def widen(column, tower_level, n_vars):
    return project(column, tower_level, n_vars, [])


def _hypercube_p_pp(b, offset, r):
    """partial_evaluate_hypercube_with_buffers (shift_ind.rs:332-366) on scalars: (s_ind_p, s_ind_pp) as lists of ints."""
    assert len(r) == b and 0 < offset < (1 << b)  # assert_valid_shift_ind_args (:212-231)
    p, pp = [1] * (1 << b), [0] * (1 << b)
    for k in range(b):
        rk = r[k]
        for i in range(1 << k):
            hi = (1 << k) | i
            if (offset >> k) & 1:
                pp_hi = o.mul(pp[i], rk)
                pp_lo = pp[i] ^ pp_hi
                p_hi = o.mul(p[i], rk)
                pp_hi ^= p[i] ^ p_hi
                pp[i], pp[hi], p[i], p[hi] = pp_lo, pp_hi, p_hi, 0
            else:
                p_hi = o.mul(p[i], rk)
                p_lo = p[i] ^ p_hi
                pp_hi = o.mul(pp[i], 1 ^ rk)
                p_lo ^= pp[i] ^ pp_hi
                p[i], p[hi], pp[i], pp[hi] = p_lo, p_hi, 0, pp_hi
    return p, pp


def shift_ind_table(b, offset, variant, r):
    """ShiftIndPartialEval::multilinear_extension (shift_ind.rs:117-161) as a list of 2^b ints."""
    if variant == CIRCULAR_LEFT:
        p, pp = _hypercube_p_pp(b, offset, r)
        return [x ^ y for x, y in zip(p, pp)]
    if variant == LOGICAL_LEFT:
        return _hypercube_p_pp(b, offset, r)[0]
    assert variant == LOGICAL_RIGHT
    return _hypercube_p_pp(b, (1 << b) - offset, r)[1]


def shift_target(b, offset, variant, x):
    """The y with f(x, y) = 1 (shift_ind.rs:14-34), or None."""
    n = 1 << b
    if variant == CIRCULAR_LEFT:
        return (x + offset) % n
    if variant == LOGICAL_LEFT:
        return x + offset if x + offset < n else None
    return x - offset if x >= offset else None


def shift_ind_brute(b, offset, variant, r):
    """table[x] = sum_y f(x, y) eq(y, r) from the definition."""
    eq = o.arr_to_ints(eq_expand(r))
    out = []
    for x in range(1 << b):
        y = shift_target(b, offset, variant, x)
        out.append(eq[y] if y is not None else 0)
    return out


def shift_ind_eval(b, offset, variant, x, r):
    """evaluate_at_point (shift_ind.rs:164-185) over evaluate_shift_ind_help (:237-269)."""
    left = (1 << b) - offset if variant == LOGICAL_RIGHT else offset
    p, pp = 1, 0
    for k in range(b):
        prod = o.mul(x[k], r[k])
        eq = 1 ^ x[k] ^ r[k]  # x y + (1 - x)(1 - y) in characteristic 2
        if (left >> k) & 1:
            p, pp = o.mul(r[k] ^ prod, p), o.mul(x[k] ^ prod, p) ^ o.mul(eq, pp)
        else:
            p, pp = o.mul(eq, p) ^ o.mul(r[k] ^ prod, pp), o.mul(x[k] ^ prod, pp)
    return p ^ pp if variant == CIRCULAR_LEFT else (p if variant == LOGICAL_LEFT else pp)


def tower_basis_table(k, iota):
    assert iota + k <= 7
    return [1 << (i << iota) for i in range(1 << k)]


def shifted_column(values, b, offset, variant):
    """The shifted virtual column from the definition, block by block: shifted[blk, y] = sum_x f(x, y) inner[blk, x]."""
    n = 1 << b
    out = [0] * len(values)
    for blk in range(0, len(values), n):
        for x in range(n):
            y = shift_target(b, offset, variant, x)
            if y is not None:
                out[blk + y] ^= values[blk + x]
    return out


def packed_column(values, k, iota):
    """The packed virtual column: 2^k consecutive T_iota values are the coordinates of one T_(iota+k) value."""
    return [sum(values[j + i] << (i << iota) for i in range(1 << k)) for j in range(0, len(values), 1 << k)]


def pack_values(values, tower_level):
    """Subfield values (ints below 2^(2^level)) packed into 16-byte elements, least-significant limb first; at least one element."""
    w = 1 << tower_level
    per = 128 // w
    n = max(1, (len(values) + per - 1) // per)
    ints = [0] * n
    for i, v in enumerate(values):
        ints[i // per] |= int(v) << ((i % per) * w)
    return o.ints_to_arr(ints)


# ------------------------------------------------------------------------------------------------ the prover
def resolve(provers, pool):
    """The tables of every prover, as (2^b, 2) arrays, in the order of its multilinears."""
    cache, out = {}, []
    for b, mls, _comps, _sums in provers:
        tabs = []
        for ml in mls:
            if ml[0] == "proj":
                _, col, level, n_vars, off, ln = ml
                assert n_vars == b + ln
                key = (id(col), level, off, ln)
                if key not in cache:
                    cache[key] = project(col, level, n_vars, pool[off : off + ln])
                tabs.append(cache[key].copy())
            elif ml[0] == "shift":
                _, bs, offset, variant, r_off, r_len = ml
                assert bs == b and r_len == b
                tabs.append(o.ints_to_arr(shift_ind_table(b, offset, variant, pool[r_off : r_off + r_len])))
            else:
                _, k, iota = ml
                assert k == b
                tabs.append(o.ints_to_arr(tower_basis_table(k, iota)))
        out.append(tabs)
    return out


def claim_sums(tables, comps):
    return [o.inner_product(np.ascontiguousarray(tables[i]), 7, np.ascontiguousarray(tables[j]))[1] for i, j in comps]


def prove(provers, pool, batch_coeffs, challenges, tables=None):
    """(round_proofs, final_evals): per round the truncated polynomial padded to two coefficients, per prover its final evaluations."""
    tables = resolve(provers, pool) if tables is None else tables
    ps = [dict(n_vars=b, multilins=[t.copy() for t in tabs], comps=list(comps), sums=list(sums)) for (b, _m, comps, sums), tabs in zip(provers, tables)]
    items, evals = piop_ref.batch_sumcheck_prove(ps, list(batch_coeffs), list(challenges))
    proofs = [(list(v) + [0, 0])[:2] for kind, v in items if kind == "round_proof"]
    return proofs, evals


# ------------------------------------------------------------------------------------------------ the verifier
def verify(provers, pool, batch_coeffs, challenges, round_proofs, final_evals):
    """The verifier's equations on a transcript: every round R(0) + R(1) = the running claim (which is how the truncated coefficient is
    recovered), a finishing prover's batched product of final evaluations leaves the claim, the claim ends at zero; a projection's
    final evaluation is the inner column's multilinear extension at r' || suffix, a transparent's is its own evaluation at r'."""

    def batched(bc, values):
        acc, scale = 0, 1
        for v in values:
            acc ^= o.mul(v, scale)
            scale = o.mul(scale, bc)
        return acc

    claim = 0
    for (b, _m, _c, sums), bc in zip(provers, batch_coeffs):
        claim ^= o.mul(bc, batched(bc, sums))
    total = provers[-1][0] if provers else 0
    if len(round_proofs) != total or len(final_evals) != len(provers):
        return False
    at = 0

    def retire(round_):
        nonlocal at, claim
        while at < len(provers) and provers[at][0] == round_:
            b, mls, comps, _s = provers[at]
            ev = final_evals[at]
            if len(ev) != len(mls):
                return False
            claim ^= o.mul(batch_coeffs[at], batched(batch_coeffs[at], [o.mul(ev[i], ev[j]) for i, j in comps]))
            r_rev = list(reversed(challenges[:b]))
            for ml, v in zip(mls, ev):
                if ml[0] == "proj":
                    _, col, level, n_vars, off, ln = ml
                    want = o.mle_evaluate(widen(col, level, n_vars), n_vars, r_rev + list(pool[off : off + ln]))
                elif ml[0] == "shift":
                    want = shift_ind_eval(b, ml[2], ml[3], r_rev, pool[ml[4] : ml[4] + ml[5]])
                else:
                    want = o.mle_evaluate(o.ints_to_arr(tower_basis_table(ml[1], ml[2])), b, r_rev)
                if want != v:
                    return False
            at += 1
        return True

    for r in range(total):
        if not retire(r):
            return False
        c0, c1 = round_proofs[r]
        c2 = claim ^ c1  # R(0) + R(1) = c1 + c2 = the running claim
        claim = o.evaluate_univariate([c0, c1, c2], challenges[r])
    if not retire(total):
        return False
    return at == len(provers) and claim == 0
