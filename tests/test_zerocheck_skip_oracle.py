"""Pins the CPU restatement of the batched univariate-skip zerocheck (tests/zerocheck_skip_ref.py; reference: sumcheck/prove/
batch_zerocheck.rs:166-293, verify_zerocheck.rs:53-166): its verifier, written independently of its prover, accepts the prover's
transcript on satisfying witnesses and rejects a flipped bit anywhere; the claimed evaluations equal an independent multilinear
evaluation of every original column; the fold equals the oracle's fold_right."""
import copy
import functools

import numpy as np
import pytest

import zerocheck_skip_ref as R

LIN3 = ([("var", 0), ("var", 1), ("add", 0, 1), ("var", 2), ("add", 2, 3)],) * 2 + (1,)                                   # a + b + c
MUL3 = ([("var", 0), ("var", 1), ("mul", 0, 1), ("var", 3), ("add", 2, 3)], [("var", 0), ("var", 1), ("mul", 0, 1)], 2)  # a b + d
MULB8 = ([("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("add", 2, 3)], [("var", 0), ("var", 1), ("mul", 0, 1)], 2)  # a b + c
# carry: (xin + cin)(yin + cin) + cin + cout, zout: xin + yin + cin + zout (m3/src/gadgets/add.rs:95-110)
CARRY = ([("var", 0), ("var", 2), ("add", 0, 1), ("var", 1), ("var", 2), ("add", 3, 4), ("mul", 2, 5), ("var", 2), ("add", 6, 7), ("var", 3), ("add", 8, 9)],
         [("var", 0), ("var", 2), ("add", 0, 1), ("var", 1), ("var", 2), ("add", 3, 4), ("mul", 2, 5)], 2)
ZOUT = ([("var", 0), ("var", 1), ("add", 0, 1), ("var", 2), ("add", 2, 3), ("var", 4), ("add", 4, 5)],) * 2 + (1,)


def b1_table(n_vars, seed):
    """Columns a, b, c = a + b, d = a b: a + b + c = 0 and a b + d = 0."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 2, 1 << n_vars, dtype=np.uint8), rng.integers(0, 2, 1 << n_vars, dtype=np.uint8)
    return {"n_vars": n_vars, "cols": [(a, 0), (b, 0), (a ^ b, 0), (a & b, 0)], "comps": [LIN3, MUL3]}


def b8_table(n_vars, seed):
    """B8 columns a, b, c = a b."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, 1 << n_vars, dtype=np.uint8), rng.integers(0, 256, 1 << n_vars, dtype=np.uint8)
    return {"n_vars": n_vars, "cols": [(a, 3), (b, 3), (R.b8_tables()[0][a, b], 3)], "comps": [MULB8]}


def u32_add_table(log_rows, seed):
    """Columns xin, yin, cin, cout, zout of real 32-bit additions (value index = 32 row + bit), n_vars = log_rows + 5."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, 1 << log_rows, dtype=np.uint64).astype(np.uint32)
    y = rng.integers(0, 1 << 32, 1 << log_rows, dtype=np.uint64).astype(np.uint32)
    z = (x.astype(np.uint64) + y).astype(np.uint32)
    cin = x ^ y ^ z
    cout = (x & y) | (cin & (x ^ y))
    cols = [(np.unpackbits(w.view(np.uint8), bitorder="little"), 0) for w in (x, y, cin, cout, z)]
    return {"n_vars": log_rows + 5, "cols": cols, "comps": [CARRY, ZOUT]}


CASES = {
    "b1_9_7": (7, lambda: [b1_table(9, 1)]),
    "b8_9_7": (7, lambda: [b8_table(9, 2)]),
    "u32_add_9_6": (6, lambda: [u32_add_table(4, 3)]),
    "batch_5_7_9_at_7": (7, lambda: [b1_table(5, 4), b8_table(7, 5), u32_add_table(4, 6)]),
    "one_table_n_eq_k": (5, lambda: [b1_table(5, 7)]),
    "batch_equal_sizes_4": (4, lambda: [b8_table(6, 8), b1_table(6, 9), b1_table(8, 10)]),
}


def samples(oracle, seed, tables, k):
    rounds = tables[-1]["n_vars"] - k
    s = oracle.random_scalars(0x2C00 + seed, 2 * rounds + len(tables) + 2 + k)
    return (s[:rounds], s[rounds:rounds + len(tables)], s[rounds + len(tables)], s[rounds + len(tables) + 1:2 * rounds + len(tables) + 1],
            s[2 * rounds + len(tables) + 1], s[2 * rounds + len(tables) + 2:])


@functools.lru_cache(maxsize=None)
def proved(name):
    import oracle

    k, make = CASES[name]
    tables = make()
    args = samples(oracle, sorted(CASES).index(name), tables, k)
    return tables, k, args, R.prove(tables, k, *args)


def shapes(tables):
    return [(t["n_vars"], len(t["cols"]), t["comps"]) for t in tables]


@pytest.mark.parametrize("name", sorted(CASES))
def test_verify_accepts_prove_and_the_claims_are_the_columns_evaluations(name):
    tables, k, args, proof = proved(name)
    skipped, unskipped, evals = R.verify(shapes(tables), k, *args, proof)
    assert len(skipped) == k and len(unskipped) == tables[-1]["n_vars"] - k
    assert len(evals) == sum(len(t["cols"]) for t in tables)
    assert evals == R.column_evals(tables, k, skipped, unskipped)
    assert len(proof["message"]) == (max(d for t in tables for _, _, d in t["comps"]) - 1) << k


FLIPS = ["message", "round_coeffs", "final_evals", "final_evals_indicator", "reduction_round_coeffs", "reduction_final_evals", "reduction_lagrange",
         "concat_multilinear_evals"]


@pytest.mark.parametrize("name,where", [(n, w) for n in ("batch_5_7_9_at_7", "one_table_n_eq_k", "b8_9_7") for w in FLIPS
                                        if (n, w) != ("one_table_n_eq_k", "round_coeffs")])  # (n = k: no multilinear round)
def test_verify_rejects_a_flipped_bit(name, where):
    tables, k, args, proof = proved(name)
    bad = copy.deepcopy(proof)
    if where == "message":
        bad["message"][len(bad["message"]) // 2] ^= 1 << 77
    elif where == "round_coeffs":
        bad["round_coeffs"][-1][1] ^= 1
    elif where == "final_evals":
        bad["final_evals"][0][0] ^= 1 << 127
    elif where == "final_evals_indicator":
        bad["final_evals"][-1][-1] ^= 2
    elif where == "reduction_round_coeffs":
        bad["reduction_round_coeffs"][k // 2][2] ^= 1 << 40
    elif where == "reduction_final_evals":
        bad["reduction_final_evals"][1] ^= 1
    elif where == "reduction_lagrange":
        bad["reduction_final_evals"][-1] ^= 1
    else:
        bad["concat_multilinear_evals"][0] ^= 1
    with pytest.raises(R.VerifyError):
        R.verify(shapes(tables), k, *args, bad)


def test_verify_rejects_a_witness_that_does_not_satisfy(oracle):
    tables = [b1_table(8, 11)]
    tables[0]["cols"][3][0][77] ^= 1  # d != a b in one row
    args = samples(oracle, 99, tables, 6)
    with pytest.raises(R.VerifyError):
        R.verify(shapes(tables), 6, *args, R.prove(tables, 6, *args))


def test_shape_errors():
    with pytest.raises(R.VerifyError, match="ClaimsOutOfOrder"):
        R.batch_shape([(9, 4, [MUL3]), (7, 4, [MUL3])], 7)
    with pytest.raises(R.VerifyError, match="IncorrectSkippedRoundsCount"):
        R.batch_shape([(5, 4, [MUL3]), (6, 4, [MUL3])], 7)
    with pytest.raises(R.VerifyError, match="degree"):
        R.batch_shape([(9, 4, [MUL3[:2] + (3,)])], 7)


@pytest.mark.parametrize("level,n_vars,k", [(0, 13, 7), (0, 10, 1), (0, 11, 8), (3, 10, 6), (3, 8, 1), (3, 12, 8)])
def test_fold_equals_the_oracles_fold_right(oracle, level, n_vars, k):
    rng = np.random.default_rng(17 * n_vars + k + level)
    v = rng.integers(0, 2 if level == 0 else 256, 1 << n_vars, dtype=np.uint8)
    coeffs = oracle.random_scalars(0x2D00 + n_vars + k, 1 << k)
    out = oracle.arr(1 << (n_vars - k))
    assert oracle.fold_right(R.pack(v, level), level, oracle.ints_to_arr(coeffs), out) == 0
    assert oracle.arr_to_ints(out) == R.fold(v, k, coeffs)


def test_padding_and_projection(oracle):
    """A table shorter than k: the padded column repeats, its projection is the padded column itself, and its claimed evaluation is the
    original column's at the low skipped challenges."""
    v = np.arange(8, dtype=np.uint8)
    assert list(R.pad_high(v, 3, 5)) == list(range(8)) * 4
    assert R.project(R.pad_high(v, 3, 5), 5, 5, oracle.random_scalars(1, 4)) == list(range(8)) * 4
