"""CPU restatement of evalcheck's projection of a LINEAR-COMBINATION inner column from its constituents (try_build_partial_eval,
core/src/protocols/evalcheck/subclaims.rs:305-346), on top of tests/evalcheck_ref.py:

  project_lincomb     offset + sum_t coeff_t * evaluate_partial_high(column_t): evalcheck_ref.project per term, oracle.mul, XOR
  materialise         the combination as a column of B128 values, element by element (oracle.mul_vec on the unpacked values): what the
                      projection must agree with and what the verifier evaluates -- it shares nothing with project_lincomb
  resolve / prove     a ("lincomb", terms, offset, n_vars, suffix_off, suffix_len) multilinear becomes its 2^b table, the rest is
                      evalcheck_ref.prove
  verify              evalcheck_ref.verify with every lincomb replaced by the plain projection of its materialised column: its final
                      evaluation is the combination's multilinear extension at r' || suffix

terms: [(column, tower_level, coeff)], column the packed (N, 2) uint64 array of 2^n_vars values of its level, coeff and offset ints.
Pinned by tests/test_evalcheck_lincomb_oracle.py; the GPU parity tests compare with it."""
import numpy as np

import adversarial as A
import evalcheck_ref as R
import oracle as o


def project_lincomb(terms, offset, n_vars, suffix, query=None):
    """offset + sum_t coeff_t * project(column_t): 2^(n_vars - len(suffix)) elements.  The offset is added once, unscaled (*acc += offset in
    the reference: a tensor expansion sums to one).  query: a 2^q-element table to take in place of the suffix's tensor expansion (the
    device op does not ask for one: tables of zeros and ones)."""
    q = len(suffix) if query is None else query.shape[0].bit_length() - 1
    acc = [offset] * (1 << (n_vars - q))
    for col, level, coeff in terms:
        if query is None:
            part = R.project(col, level, n_vars, suffix)
        else:
            part = o.arr(1 << (n_vars - q))
            assert o.fold_left(np.ascontiguousarray(col), level, np.ascontiguousarray(query), part) == 0
        part = o.arr_to_ints(part)
        for i, v in enumerate(part):
            acc[i] ^= v if coeff == 1 else (o.mul(coeff, v) if coeff else 0)
    return o.ints_to_arr(acc)


def materialise(terms, offset, n_vars):
    """The combination's 2^n_vars values as B128 elements."""
    n = 1 << n_vars
    acc = np.zeros((n, 2), dtype=np.uint64)
    acc[:, 0] = np.uint64(offset & A.M64)
    acc[:, 1] = np.uint64(offset >> 64)
    for col, level, coeff in terms:
        vals = A.unpack_subfield(col, level)[:n]
        assert vals.shape[0] == n
        scale = np.zeros((n, 2), dtype=np.uint64)
        scale[:, 0] = np.uint64(coeff & A.M64)
        scale[:, 1] = np.uint64(coeff >> 64)
        acc ^= o.mul_vec(np.ascontiguousarray(vals), scale)
    return acc


def plain(provers, memo=None):
    """The provers with every lincomb replaced by ("proj", its materialised column, 7, n_vars, suffix_off, suffix_len)."""
    memo = {} if memo is None else memo
    out = []
    for b, mls, comps, sums in provers:
        new = []
        for ml in mls:
            if ml[0] == "lincomb":
                _, terms, offset, n_vars, off, ln = ml
                key = (tuple((id(c), lv, cf) for c, lv, cf in terms), offset, n_vars)
                if key not in memo:
                    memo[key] = materialise(terms, offset, n_vars)
                new.append(("proj", memo[key], 7, n_vars, off, ln))
            else:
                new.append(ml)
        out.append((b, new, comps, sums))
    return out


def resolve(provers, pool):
    """The tables of every prover as evalcheck_ref.resolve gives them, a lincomb's through project_lincomb."""
    cache, out = {}, []
    for b, mls, comps, sums in provers:
        tabs = []
        for ml in mls:
            if ml[0] == "lincomb":
                _, terms, offset, n_vars, off, ln = ml
                assert n_vars == b + ln
                key = (tuple((id(c), lv, cf) for c, lv, cf in terms), offset, off, ln)
                if key not in cache:
                    cache[key] = project_lincomb(terms, offset, n_vars, pool[off : off + ln])
                tabs.append(cache[key].copy())
            else:
                tabs.append(R.resolve([(b, [ml], [], [])], pool)[0][0])
        out.append(tabs)
    return out


def prove(provers, pool, batch_coeffs, challenges, tables=None):
    return R.prove(provers, pool, batch_coeffs, challenges, tables=resolve(provers, pool) if tables is None else tables)


def verify(provers, pool, batch_coeffs, challenges, round_proofs, final_evals, memo=None):
    return R.verify(plain(provers, memo), pool, batch_coeffs, challenges, round_proofs, final_evals)
