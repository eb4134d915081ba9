"""TEST INFRASTRUCTURE: CPU restatement of the batched univariate-skip zerocheck for the domain field B8 -- the prover
sumcheck::prove::batch_zerocheck::batch_prove (crates/core/src/protocols/sumcheck/prove/batch_zerocheck.rs:166-293, with
ZerocheckProverImpl, prove/zerocheck.rs:79-516, and ZerocheckUnivariateEvalsOutput::fold, prove/univariate.rs:139-193) and, written
independently of it, the verifier batch_verify (verify_zerocheck.rs:53-166, zerocheck.rs:157-289, front_loaded.rs:106-310,
eq_ind.rs:121-181).  Built from tests/univariate_skip_ref.py (the univariate round, the fold, the Lagrange coefficients),
oracle.zerocheck_ref (the eq-ind sumcheck prover over the old HAL) and the oracle's field; the transcript's samples are arguments.

A table is a dict {"n_vars": n, "cols": [(values, level)], "comps": [(steps, steps_of_the_leading_form, degree)]}: values a numpy uint8
array of the 2^n column values (B1 as 0 / 1, B8 as bytes), the steps over B8 (the same circuits serve the multilinear rounds over
B128: a B8 constant embeds as itself).  Tables come in ascending n_vars.

  prove(tables, k, zerocheck_challenges, batch_coeffs, univariate_challenge, sumcheck_challenges, reduction_batch_coeff,
        reduction_challenges) -> the proof, a dict, in the transcript's writing order:
      message                 the univariate round's message: D - 2^k values, D = (largest degree of the batch) 2^k
      round_coeffs            max_n - k round polynomials of the multilinear rounds, each padded to Dmax + 2 coefficients,
                              Dmax = max(2, largest degree of the batch) -- all coefficients, not the truncated form of the transcript
      final_evals             per table in finishing order (= the given order): the univariatized columns' evaluations, then the
                              indicator's
      reduction_round_coeffs  k round polynomials (3 coefficients) of the univariatizing reduction
      reduction_final_evals   every projected column's evaluation, then the Lagrange-coefficient multilinear's
      skipped_challenges, unskipped_challenges, concat_multilinear_evals   BatchZerocheckOutput (zerocheck.rs:140-150)
  verify(shapes, k, ..., proof)   shapes = [(n_vars, n_cols, comps)]; raises VerifyError, returns the BatchZerocheckOutput triple
  column_evals(tables, k, skipped, unskipped)   every ORIGINAL column's multilinear extension at skipped || unskipped, independently"""
import numpy as np

import oracle as o
from univariate_skip_ref import (b8_tables, b8_times_b128, bytes_to_int, eq_expansion, fold, int_to_bytes, lagrange_at, pack, unpack,  # noqa: F401
                                 univariate_evals)


class VerifyError(Exception):
    pass


def eq2(a, b):
    """eq(a, b) = a b + (1 - a)(1 - b) in characteristic 2."""
    return 1 ^ a ^ b


def pad_high(values, n_vars, k):
    """high_pad_small_multilinear (prove/zerocheck.rs:79-119): 2^(k - n_vars) copies, one after the other."""
    v = np.asarray(values, dtype=np.uint8)
    return v if n_vars >= k else np.tile(v, 1 << (k - n_vars))


def weighted_rows(values, weights, axis_rows):
    """sum over the rows (axis_rows = 0) or the columns (1) of a 2-d array of B8 values times one GF(2^128) weight per row / column."""
    w = np.stack([int_to_bytes(e) for e in weights])
    w = w[:, None, :] if axis_rows == 0 else w[None, :, :]
    return [bytes_to_int(s) for s in np.bitwise_xor.reduce(b8_times_b128(values, w), axis=axis_rows)]


def project(values, n_eff, k, unskipped):
    """project_to_skipped_variables (prove/zerocheck.rs:472-516): evaluate_partial_high at the last n_eff - k unskipped challenges."""
    q = n_eff - k
    eqq = eq_expansion(unskipped[len(unskipped) - q:])
    return weighted_rows(np.asarray(values, dtype=np.uint8).reshape(1 << q, 1 << k), eqq, 0)


def batch_shape(shapes, k):
    ns = [s[0] for s in shapes]
    if ns != sorted(ns):
        raise VerifyError("ClaimsOutOfOrder")
    if not ns or ns[-1] < k:
        raise VerifyError("IncorrectSkippedRoundsCount")
    degrees = [[c[2] for c in s[2]] for s in shapes]
    for ds in degrees:
        for d in ds:
            if d < 1 or (d << k) > 256:
                raise VerifyError("degree out of range")
    d_top = max([d for ds in degrees for d in ds] + [0])
    return ns[-1] - k, d_top << k, max(2, d_top), degrees


def prove(tables, k, zerocheck_challenges, batch_coeffs, univariate_challenge, sumcheck_challenges, reduction_batch_coeff, reduction_challenges):
    from oracle.zerocheck_ref import eqind_sumcheck_prove

    rounds, D, d_max, degrees = batch_shape([(t["n_vars"], len(t["cols"]), t["comps"]) for t in tables], k)
    K = 1 << k
    assert len(zerocheck_challenges) == rounds and len(sumcheck_challenges) == rounds and len(batch_coeffs) == len(tables) and len(reduction_challenges) == k
    z = univariate_challenge
    l_sub, l_full = lagrange_at(K, z), lagrange_at(D, z)
    message = [0] * max(0, D - K)
    round_coeffs = [[0] * (d_max + 2) for _ in range(rounds)]
    final_evals, padded = [], []
    for t, bc, ds in zip(tables, batch_coeffs, degrees):
        n_eff = max(t["n_vars"], k)
        nr = n_eff - k
        cols = [(pad_high(v, t["n_vars"], k), level) for v, level in t["cols"]]
        padded.append((cols, n_eff))
        ch = list(zerocheck_challenges[rounds - nr:])  # (constraint_system/prove.rs:470)
        per = univariate_evals(cols, n_eff, k, [c[0] for c in t["comps"]], ds, ch, D)
        scale = bc  # powers of the coefficient, times the coefficient (batch_zerocheck.rs:198-206, prove/zerocheck.rs:354-370)
        for p in per:
            message = [a ^ o.mul(scale, b) for a, b in zip(message, p)]
            scale = o.mul(scale, bc)
        sums = []
        for p in per:
            s = 0
            for j, v in enumerate(p):
                s ^= o.mul(v, l_full[K + j])
            sums.append(s)
        folded = [o.ints_to_arr(fold(v, k, l_sub)) for v, _ in cols]
        if nr == 0:
            finals = [o.arr_to_ints(f)[0] for f in folded] + [1]
        else:
            coeffs, finals = eqind_sumcheck_prove(folded, nr, [(c[0], c[1]) for c in t["comps"]], sums, ch, bc, list(sumcheck_challenges[:nr]), ds)
            for r in range(nr):  # front-loaded: every prover starts in round 0 (prove/front_loaded.rs:122-137)
                for i, c in enumerate(coeffs[r]):
                    round_coeffs[r][i] ^= o.mul(c, bc)
        final_evals.append(finals)
    unskipped = list(reversed(sumcheck_challenges))
    projected, sums = [], []
    for (cols, n_eff), finals in zip(padded, final_evals):
        projected += [project(v, n_eff, k, unskipped) for v, _ in cols]
        sums += finals[:-1]
    m = len(projected)
    mls = [o.ints_to_arr(p) for p in projected] + [o.ints_to_arr(l_sub)]
    red_coeffs, red_finals = o.bivariate_sumcheck_prove(mls, k, [(i, m) for i in range(m)], sums, reduction_batch_coeff, list(reduction_challenges))
    red_coeffs = [[o.mul(c, reduction_batch_coeff) for c in rc] for rc in red_coeffs]
    return {
        "message": message, "round_coeffs": round_coeffs, "final_evals": final_evals, "reduction_round_coeffs": red_coeffs,
        "reduction_final_evals": red_finals, "skipped_challenges": list(reversed(reduction_challenges)), "unskipped_challenges": unskipped,
        "concat_multilinear_evals": red_finals[:-1],
    }


def _check_round(coeffs, claim, max_degree, what):
    if any(coeffs[max_degree + 1:]):
        raise VerifyError("%s: a round polynomial of too high a degree" % what)
    total = coeffs[0]
    for c in coeffs:
        total ^= c
    if total != claim:  # P(0) + P(1)
        raise VerifyError("%s: a round polynomial does not sum to the running claim" % what)


def verify(shapes, k, zerocheck_challenges, batch_coeffs, univariate_challenge, sumcheck_challenges, reduction_batch_coeff, reduction_challenges, proof):
    rounds, D, _, degrees = batch_shape(shapes, k)
    K = 1 << k
    z = univariate_challenge
    # ---- the message's value at the univariate challenge (verify_zerocheck.rs:92-112)
    if len(proof["message"]) != max(0, D - K):
        raise VerifyError("message length")
    l_full = lagrange_at(D, z)
    claim = 0
    for j, v in enumerate(proof["message"]):
        claim ^= o.mul(v, l_full[K + j])
    # ---- the front-loaded batch of eq-ind sumchecks (front_loaded.rs:106-310); a claim's composition is C(columns) * indicator
    n_rem = [max(s[0], k) - k for s in shapes]
    if len(proof["final_evals"]) != len(shapes) or len(proof["round_coeffs"]) != rounds:
        raise VerifyError("NumberOfFinalEvaluations")
    done = 0

    def finish_claims(r, claim):
        nonlocal done
        while done < len(shapes) and n_rem[done] == r:
            evals, bc = proof["final_evals"][done], batch_coeffs[done]
            if len(evals) != shapes[done][1] + 1:
                raise VerifyError("NumberOfMultilinearEvals")
            scale = bc
            for comp in shapes[done][2]:
                claim ^= o.mul(scale, o.mul(o.circuit_eval(comp[0], list(evals[:-1])), evals[-1]))
                scale = o.mul(scale, bc)
            done += 1
        return claim

    for r in range(rounds):
        claim = finish_claims(r, claim)
        deg = max(d for p in range(done, len(shapes)) for d in degrees[p]) + 1  # (max_degree_remaining, plus the indicator's factor)
        _check_round(proof["round_coeffs"][r], claim, deg, "multilinear round %d" % r)
        claim = o.evaluate_univariate(proof["round_coeffs"][r], sumcheck_challenges[r])
    claim = finish_claims(rounds, claim)
    if done != len(shapes) or claim != 0:
        raise VerifyError("IncorrectBatchEvaluation")
    # ---- the indicator's evaluation of every claim (eq_ind.rs:121-181)
    unskipped = list(reversed(sumcheck_challenges))
    for p in range(len(shapes)):
        want = 1
        for j in range(n_rem[p]):
            want = o.mul(want, eq2(unskipped[rounds - 1 - j], zerocheck_challenges[rounds - 1 - j]))
        if proof["final_evals"][p][-1] != want:
            raise VerifyError("IncorrectEqIndEvaluation")
    # ---- the univariatizing reduction: one bivariate product claim per column (zerocheck.rs:199-289)
    sums = [v for evals in proof["final_evals"] for v in evals[:-1]]
    m = len(sums)
    rb = reduction_batch_coeff
    claim, scale = 0, rb
    for s in sums:
        claim ^= o.mul(scale, s)
        scale = o.mul(scale, rb)
    if len(proof["reduction_round_coeffs"]) != k or len(proof["reduction_final_evals"]) != m + 1:
        raise VerifyError("IncorrectUnivariatizingReductionSumcheck")
    for r in range(k):
        _check_round(proof["reduction_round_coeffs"][r], claim, 2, "reduction round %d" % r)
        claim = o.evaluate_univariate(proof["reduction_round_coeffs"][r], reduction_challenges[r])
    fe = proof["reduction_final_evals"]
    want, scale = 0, rb
    for v in fe[:-1]:
        want ^= o.mul(scale, o.mul(v, fe[-1]))
        scale = o.mul(scale, rb)
    if want != claim:
        raise VerifyError("IncorrectBatchEvaluation (reduction)")
    skipped = list(reversed(reduction_challenges))
    lagrange_mle = 0
    for e, l in zip(eq_expansion(skipped), lagrange_at(K, z)):
        lagrange_mle ^= o.mul(e, l)
    if fe[-1] != lagrange_mle:
        raise VerifyError("IncorrectLagrangeMultilinearEvaluation")
    out = (skipped, unskipped, list(fe[:-1]))
    if (proof["skipped_challenges"], proof["unskipped_challenges"], proof["concat_multilinear_evals"]) != out:
        raise VerifyError("BatchZerocheckOutput differs")
    return out


def column_evals(tables, k, skipped, unskipped):
    """The multilinear extension of every ORIGINAL column at the low n_vars coordinates of skipped || the last n_vars - k of unskipped
    (a table of n_vars < k: at skipped[:n_vars], the high padding adds nothing), by the tensor expansion of the point."""
    out = []
    for t in tables:
        n = t["n_vars"]
        point = list(skipped[:n]) if n < k else list(skipped) + list(unskipped[len(unskipped) - (n - k):])
        e = eq_expansion(point)
        for v, _ in t["cols"]:
            out.append(weighted_rows(np.asarray(v, dtype=np.uint8).reshape(1 << n, 1), e, 0)[0])
    return out
