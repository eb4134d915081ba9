"""Pins the CPU restatement of the univariate-skip zerocheck for every arm (tests/univariate_skip_base_ref.py): at base 3 it is
tests/univariate_skip_ref.py; B8 data zero-extended into columns of level 4 .. 7 gives the same outputs as at level 3 (the wide
packing and the coordinate action); a satisfying a b - c table over B32 and over B128 gives a proof the independent verifier of
tests/zerocheck_skip_ref.py accepts, with final evaluations equal to the direct multilinear evaluation of the columns; the fold
is the oracle's fold_right of the packed column.  CPU only."""
import numpy as np
import pytest

import univariate_skip_base_ref as B
import univariate_skip_ref as R
import zerocheck_skip_ref as Z
from test_univariate_skip_oracle import SATISFIED, witness

CASES = [(n, k, d) for k in (1, 3, 6, 7) for d in (1, 2, 3, 4) if d << k <= 256 for n in (k, k + 1)]


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("n_vars,k,d", CASES)
def test_base_3_is_the_b8_restatement(oracle, n_vars, k, d, level):
    seed = 1000 * n_vars + 10 * k + d + 7 * level
    vals = witness(seed, n_vars, level)
    rng = np.random.default_rng(seed)
    vals[2] = rng.integers(0, 2 if level == 0 else 256, 1 << n_vars, dtype=np.uint8)  # (no constraint holds: nonzero messages)
    comps = [s for s, dc in SATISFIED if dc <= d]
    degrees = [dc for _, dc in SATISFIED if dc <= d]
    ch = oracle.random_scalars(0x6C00 + seed, n_vars - k)
    alpha = oracle.random_scalars(0x6C80 + seed, 1)[0]
    cols = [(v, level) for v in vals]
    D = min(256, (d << k) + 5)
    assert B.univariate_evals(3, cols, n_vars, k, comps, degrees, ch, D) == R.univariate_evals(cols, n_vars, k, comps, degrees, ch, D)
    assert B.univariate_evals(3, cols, n_vars, k, comps, degrees, ch, D, alpha) == R.univariate_evals(cols, n_vars, k, comps, degrees, ch, D, alpha)


@pytest.mark.parametrize("level", [4, 5, 6, 7])
@pytest.mark.parametrize("n_vars,k", [(2, 1), (4, 3), (7, 6), (8, 7)])
def test_embedding_invariance(oracle, level, n_vars, k):
    """B8 values zero-extended into level-`level` columns, computed in that arm: the outputs of level 3."""
    d = 3 if 3 << k <= 256 else 2
    rng = np.random.default_rng(31 * level + n_vars)
    vals = [rng.integers(0, 256, 1 << n_vars, dtype=np.uint8) for _ in range(4)]
    comps = [s for s, dc in SATISFIED if dc <= d] + [[("var", 0), ("const", 0x9D), ("mul", 0, 1), ("var", 3), ("pow", 3, 2), ("add", 2, 4)]]
    degrees = [dc for _, dc in SATISFIED if dc <= d] + [2]
    ch = oracle.random_scalars(0x6D00 + level, n_vars - k)
    D = d << k
    want = R.univariate_evals([(v, 3) for v in vals], n_vars, k, comps, degrees, ch, D)
    assert any(any(p) for p in want)
    wide = [(B.wide(v, level), level) for v in vals]
    assert B.univariate_evals(level, wide, n_vars, k, comps, degrees, ch, D) == want
    # and through the packed layout: little-endian values of 2^(level - 3) bytes
    for v, _ in wide:
        packed = B.pack(v, level)
        assert packed.shape[0] == max(1, (1 << n_vars) >> (7 - level))
        assert np.array_equal(B.unpack(packed, level, n_vars), v)
        raw = packed.view(np.uint8).reshape(-1)[: (1 << n_vars) << (level - 3)].reshape(1 << n_vars, -1)
        assert np.array_equal(raw[:, 0], v[:, 0]) and not raw[:, 1:].any()


@pytest.mark.parametrize("level,n_vars,k", [(4, 5, 2), (5, 9, 7), (6, 4, 3), (7, 3, 1)])
def test_wide_fold_matches_the_oracles_fold_right(oracle, level, n_vars, k):
    rng = np.random.default_rng(17 * n_vars + level)
    v = rng.integers(0, 256, (1 << n_vars, 1 << (level - 3)), dtype=np.uint8)
    coeffs = oracle.random_scalars(0x6E00 + n_vars, 1 << k)
    out = oracle.arr(1 << (n_vars - k))
    assert oracle.fold_right(B.pack(v, level), level, oracle.ints_to_arr(coeffs), out) == 0
    assert B.fold(v, k, coeffs) == oracle.arr_to_ints(out)


def product_table(oracle, seed, n_vars, level, cubic=False):
    """A satisfying table: a, b random in T_level, c = a b (and, cubic, d = a b c) -- columns and compositions a b - c (, a b c - d)."""
    rng = np.random.default_rng(seed)
    w = 1 << (level - 3)
    a = [int.from_bytes(rng.bytes(w), "little") for _ in range(1 << n_vars)]
    b = [int.from_bytes(rng.bytes(w), "little") for _ in range(1 << n_vars)]
    c = [B.base_mul(x, y, level) for x, y in zip(a, b)]
    cols = [a, b, c]
    quad = [("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("add", 2, 3)]
    quad_inf = [("var", 0), ("var", 1), ("mul", 0, 1)]
    comps = [(quad, quad_inf, 2)]
    if cubic:
        cols.append([B.base_mul(x, y, level) for x, y in zip(c, c)])
        comps.append(([("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("mul", 2, 3), ("var", 3), ("add", 4, 5)],
                      [("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("mul", 2, 3)], 3))
    return {"n_vars": n_vars, "cols": [(B.from_ints(v, level), level) for v in cols], "comps": comps}


def samples(oracle, seed, tables, k):
    rounds = max(t["n_vars"] for t in tables) - k
    s = oracle.random_scalars(seed, 2 * rounds + len(tables) + 2 + k)
    return (s[:rounds], s[rounds:rounds + len(tables)], s[rounds + len(tables)], s[rounds + len(tables) + 1:2 * rounds + len(tables) + 1],
            s[2 * rounds + len(tables) + 1], s[2 * rounds + len(tables) + 2:])


@pytest.mark.parametrize("level,n_vars,k", [(5, 5, 3), (7, 4, 2), (5, 1, 3)])
def test_satisfying_product_table_passes_the_verifier(oracle, level, n_vars, k):
    tables = [product_table(oracle, 0x70 + level, n_vars, level)]
    if n_vars < k:  # (the batch needs a table of at least k variables)
        tables.append(product_table(oracle, 0x71, k + 1, 3))
    assert B.table_base(tables[0]) == level
    args = samples(oracle, 0x6F00 + level, tables, k)
    proof = B.prove(tables, k, *args)
    assert any(proof["round_coeffs"][0]) if proof["round_coeffs"] else True
    shapes = [(t["n_vars"], len(t["cols"]), t["comps"]) for t in tables]
    skipped, unskipped, evals = Z.verify(shapes, k, *args, proof)
    assert evals == B.column_evals(tables, k, skipped, unskipped)
    # an unsatisfied witness is rejected: the check above is not vacuous
    bad = tables[-1]["cols"][2][0].copy()
    bad.reshape(len(bad), -1)[1, 0] ^= 1
    broken = tables[:-1] + [dict(tables[-1], cols=tables[-1]["cols"][:2] + [(bad, tables[-1]["cols"][2][1])])]
    with pytest.raises(Z.VerifyError):
        Z.verify(shapes, k, *args, B.prove(broken, k, *args))


def test_prove_at_base_3_is_the_b8_prover(oracle):
    """Tables of B1 / B8 columns: the mixed-level prover is zerocheck_skip_ref.prove."""
    k = 3
    rng = np.random.default_rng(0x72)
    quad = ([("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("add", 2, 3), ("const", 0x53), ("add", 4, 5)], [("var", 0), ("var", 1), ("mul", 0, 1)], 2)
    tables = [{"n_vars": n, "cols": [(rng.integers(0, 2 if level == 0 else 256, 1 << n, dtype=np.uint8), level) for _ in range(3)], "comps": [quad]}
              for n, level in ((2, 0), (5, 3))]
    args = samples(oracle, 0x7200, tables, k)
    assert B.prove(tables, k, *args) == Z.prove(tables, k, *args)
    assert B.column_evals(tables, k, [1, 2, 3], [4, 5]) == Z.column_evals(tables, k, [1, 2, 3], [4, 5])


def test_table_base():
    quad = [("var", 0), ("var", 1), ("mul", 0, 1)]
    col = lambda level: (None, level)  # noqa: E731
    assert B.table_base({"cols": [col(0)], "comps": [(quad, quad, 2)]}) == 3
    assert B.table_base({"cols": [col(0), col(5)], "comps": [(quad, quad, 2)]}) == 5
    assert B.table_base({"cols": [col(3)], "comps": [(quad + [("const", 0x100), ("add", 2, 3)], quad, 2)]}) == 4
    assert B.table_base({"cols": [col(4)], "comps": [(quad + [("const", 1 << 64), ("add", 2, 3)], quad, 2)]}) == 7
    assert [B.const_level(c) for c in (0, 1, 2, 3, 4, 15, 16, 255, 256, 1 << 16, 1 << 32, (1 << 64) - 1, 1 << 64)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 6, 7]
