"""CPU checks of tests/fri_verify_ref.py, the FRI verifier restated as test infrastructure: its folds are pinned against the oracle's
whole-codeword folds, the Python prover's advice verifies for every shape of the device tests, and one flipped bit anywhere in a
proof is rejected with the error the reference gives (fri/error.rs VerificationError, merkle_tree/errors.rs)."""
import numpy as np
import pytest

import fri_verify_ref as fv


def _s(oracle, log_domain):
    return oracle.ntt_s_evals(fv.TW_LEVEL, log_domain)


@pytest.mark.parametrize("log_len,log_domain,n_ch", [(L, D, n) for L, D in [(1, 1), (3, 5), (7, 7), (10, 10), (10, 12)] for n in (1, 2, 3) if n <= L])
def test_fold_chunk_matches_the_oracles_fri_fold(oracle, log_len, log_domain, n_ch):
    """fold_chunk of chunk i == element i of oracle.fri_fold of the whole codeword (log_batch 0)"""
    s = _s(oracle, log_domain)
    code = oracle.random_b128(0xC0DE + 16 * log_len + n_ch, 1 << log_len)
    chs = oracle.random_scalars(0xC4A1 + log_len, n_ch)
    want = oracle.arr(1 << (log_len - n_ch))
    assert oracle.fri_fold(s, fv.TW_LEVEL, log_domain, log_len, 0, chs, code, want) == 0
    vals = fv.ints(code)
    got = [fv.fold_chunk(oracle, s, log_domain, log_len, i, vals[i << n_ch : (i + 1) << n_ch], chs) for i in range(1 << (log_len - n_ch))]
    assert got == fv.ints(want)


@pytest.mark.parametrize("log_len,log_domain,log_batch,n_fold",
                         [(L, D, b, n) for L, D in [(1, 1), (4, 6), (8, 8), (10, 10)] for b in (0, 2) for n in (1, 2, 3) if n <= L])
def test_fold_interleaved_chunk_matches_the_oracles_fold_interleaved(oracle, log_len, log_domain, log_batch, n_fold):
    """fold_interleaved_chunk of chunk i == element i of oracle.fold_interleaved of the whole interleaved codeword"""
    s = _s(oracle, log_domain)
    code = oracle.random_b128(0x1EAF + 64 * log_len + 8 * log_batch + n_fold, 1 << (log_len + log_batch))
    chs = oracle.random_scalars(0xC4A2 + log_len + log_batch, log_batch + n_fold)
    want = oracle.arr(1 << (log_len - n_fold))
    assert oracle.fold_interleaved(s, fv.TW_LEVEL, log_domain, log_len, log_batch, chs, code, want) == 0
    tensor = fv.tensor_expand(oracle, chs[:log_batch])
    vals, w = fv.ints(code), log_batch + n_fold
    got = [fv.fold_interleaved_chunk(oracle, s, log_domain, log_len, log_batch, i, vals[i << w : (i + 1) << w], tensor, chs[log_batch:])
           for i in range(1 << (log_len - n_fold))]
    assert got == fv.ints(want)


@pytest.mark.parametrize("p", [p for p, _ in fv.SHAPES], ids=fv.SHAPE_IDS)
def test_python_prover_verifies(oracle, p):
    _msg, chs, idx, pr = fv.case(oracle, p)
    assert pr.advice.shape[0] == p.layout()[2]
    assert len(idx) == p.n_test_queries and all(0 <= i < 1 << p.index_bits() for i in idx)
    if p.n_test_queries >= 4:
        assert idx[0] == 0 and idx[1] == (1 << p.index_bits()) - 1 and idx[2] == idx[3]
    final = fv.verify(oracle, p, pr.commitments[0], pr.commitments[1:], chs, idx, pr.advice)
    # the fully folded message: every element of the terminate codeword folds to it, and so does the message itself through the
    # oracle's whole-codeword fold
    s = _s(oracle, p.rs_log_len())
    out = oracle.arr(1 << p.log_inv_rate)
    assert oracle.fri_fold(s, fv.TW_LEVEL, p.rs_log_len(), p.rs_log_len(), p.log_batch_size, chs, pr.codewords[0], out) == 0
    assert fv.ints(out) == [final] * (1 << p.log_inv_rate)


P0 = fv.SHAPES[0][0]  # arities (3, 2, 1), three queries: branches of four digests, layers of four


def _tampered(oracle, unit, word=0, bit=5):
    _msg, chs, idx, pr = fv.case(oracle, P0)
    advice = pr.advice.copy()
    advice[unit, word] ^= np.uint64(1 << bit)
    return chs, idx, pr, advice


def _kind(oracle, p, commitments, chs, idx, advice):
    with pytest.raises(fv.FriVerifyError) as e:
        fv.verify(oracle, p, commitments[0], commitments[1:], chs, idx, advice)
    return e.value.kind


def test_one_flipped_bit_is_rejected(oracle):
    header, record, _total = P0.layout()
    arity0 = P0.fold_arities[0]
    places = {
        "an opened value": header + 1,
        "an opened value of the last query, second oracle": header + 2 * record + (1 << arity0) + 2 * 4 + 3,
        "a branch digest": header + (1 << arity0) + 2,
        "a layer digest": P0.terminate_len() + 3,
        "a terminate element": 2,
    }
    for what, unit in places.items():
        chs, idx, pr, advice = _tampered(oracle, unit, word=unit & 1)
        assert _kind(oracle, P0, pr.commitments, chs, idx, advice) == "InvalidProof", what
    _msg, chs, idx, pr = fv.case(oracle, P0)
    for k in range(len(pr.commitments)):
        bad = list(pr.commitments)
        bad[k] = bytes([bad[k][0] ^ 0x10]) + bad[k][1:]
        assert _kind(oracle, P0, bad, chs, idx, pr.advice) == "InvalidProof", "commitment %d" % k


def test_a_wrong_fold_is_an_incorrect_fold(oracle):
    """A prover that commits to an oracle that is not the fold of the one before it, with trees that match what it sends: every
    Merkle check passes, the query that opens the position does not."""
    msg, chs, idx, _pr = fv.case(oracle, P0)
    for k in range(1, P0.n_oracles()):
        shift = sum(P0.fold_arities[1 : k])  # query 1 (index 2^index_bits - 1) reads oracle k at this position
        pos = idx[1] >> shift
        pr = fv.prove(oracle, P0, msg, chs, idx, tamper=(k, pos))
        assert _kind(oracle, P0, pr.commitments, chs, idx, pr.advice) == "IncorrectFold", k


def test_a_terminate_codeword_of_too_high_degree_is_an_incorrect_degree(oracle):
    msg, chs, idx, _pr = fv.case(oracle, P0)
    pr = fv.prove(oracle, P0, msg, chs, idx, tamper=(P0.n_oracles(), 1))
    assert _kind(oracle, P0, pr.commitments, chs, idx, pr.advice) == "IncorrectDegree"
    # without oracles the whole codeword is the advice, and the same check guards it
    p4 = fv.SHAPES[4][0]
    msg, chs, idx, _pr = fv.case(oracle, p4)
    pr = fv.prove(oracle, p4, msg, chs, idx, tamper=(0, 70))
    assert _kind(oracle, p4, pr.commitments, chs, idx, pr.advice) == "IncorrectDegree"


def test_a_short_advice_is_a_transcript_error(oracle):
    _msg, chs, idx, pr = fv.case(oracle, P0)
    assert _kind(oracle, P0, pr.commitments, chs, idx, pr.advice[:-1]) == "TranscriptError"
