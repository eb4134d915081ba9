"""CPU restatement of the ring-switching reduction, ring_switch::prove (core/src/ring_switch/prove.rs:42-144), composed from the oracle's
pinned pieces:

  mixing / row-batch coefficients   MultilinearQuery::expand = oracle.tensor_expand from ONE
  compute_partial_evals (:147-208)  evaluate_partial_high = oracle.fold_left against the tensor expansion of the suffix: 2^kappa elements
  scale_vertical, mixing per prefix (:210-250, tower_tensor_algebra.rs)   oracle.mul and XOR on the vertical elements
  fold_vertical (tensor_algebra.rs:139-152)   the square transpose of the 2^kappa x 2^kappa limb matrix, then an inner product
  RingSwitchEqInd (ring_switch/eq_ind.rs:81-147)   fill, evals[0] = mixing_coeff, oracle.tensor_expand, oracle.fold_right over the limbs

Pinned by tests/test_ring_switch_oracle.py through the verifier's equations, with evaluations that share nothing with prove(); the GPU
parity tests compare with it.

A case is a dict:
  columns     [(packed (N, 2) uint64 array, tower_level, n_vars)]   2^n_vars values of the level packed into F, n_vars + level >= 7
  pool        list of ints: the coordinates every point is a slice of
  suffixes    [(off, len, kappa)]    suffix = pool[off : off + len], kappa = 7 - tower_level, len = n_vars - kappa
  prefixes    [(off, kappa)]         prefix = pool[off : off + kappa]: the low kappa coordinates of the point
  claims      [(committed_idx, suffix_desc_idx, prefix_desc_idx)]
  mixing      ceil(log2 n_claims) challenges;  row: max kappa challenges"""
import numpy as np

import oracle as o


def eq_expand(r):
    """eq(r)[y] = prod_k (y_k ? r_k : 1 + r_k)."""
    out = o.arr(1 << len(r))
    out[0] = o.ints_to_arr([1])[0]
    if len(r):
        assert o.tensor_expand(out, 0, list(r)) == 0
    return out


def partial_eval(column, tower_level, n_vars, suffix):
    """evaluate_partial_high: the high len(suffix) variables bound to the suffix; 2^(n_vars - len(suffix)) B128 elements as ints."""
    out = o.arr(1 << (n_vars - len(suffix)))
    assert o.fold_left(np.ascontiguousarray(column), tower_level, eq_expand(suffix), out) == 0
    return o.arr_to_ints(out)


def limb(e, i, kappa):
    w = 1 << (7 - kappa)
    return (e >> (i * w)) & ((1 << w) - 1)


def transpose(elems, kappa):
    """TensorAlgebra::transpose: limb c of row r becomes limb r of row c."""
    n, w = 1 << kappa, 1 << (7 - kappa)
    return [sum(limb(elems[c], r, kappa) << (c * w) for c in range(n)) for r in range(n)]


def fold_vertical(elems, kappa, coeffs):
    """TensorAlgebra::fold_vertical: inner product of the transposed element with the first 2^kappa coefficients."""
    acc = 0
    for row, c in zip(transpose(elems, kappa), coeffs[: 1 << kappa]):
        acc ^= o.mul(row, c)
    return acc


def eq_ind(suffix, kappa, mixing_coeff, coeffs):
    """RingSwitchEqInd::multilinear_extension (eq_ind.rs:81-147) as an (2^len, 2) array: the sequence, step by step."""
    evals = o.arr(1 << len(suffix))                       # fill(evals, 0)
    evals[0] = o.ints_to_arr([mixing_coeff])[0]           # evals[0] = mixing_coeff
    if len(suffix):
        assert o.tensor_expand(evals, 0, list(suffix)) == 0
    out = o.arr(1 << len(suffix))
    assert o.fold_right(evals, 7 - kappa, o.ints_to_arr(list(coeffs[: 1 << kappa])), out) == 0
    return out


def eq_ind_from_query(query, kappa, mixing_coeff, coeffs):
    """The same transparent from the suffix's table instead of the suffix -- tensor_expand from evals[0] = m is m times the expansion from
    ONE --, for any (2^n, 2) array in the table's place: out[x] = sum_i coeffs[i] * limb_i(mixing_coeff * query[x])."""
    scaled = o.mul_vec(np.ascontiguousarray(query), np.ascontiguousarray(np.tile(o.ints_to_arr([mixing_coeff]), (query.shape[0], 1))))
    out = o.arr(query.shape[0])
    assert o.fold_right(scaled, 7 - kappa, o.ints_to_arr(list(coeffs[: 1 << kappa])), out) == 0
    return out


def log2_ceil(n):
    return max(0, (n - 1).bit_length())


def prove(case):
    """The transcript and the reduced witness: mixed (per prefix its 2^kappa vertical elements), row_batched_evals (per claim),
    transparents (per claim an (2^len, 2) array), and the coefficient vectors."""
    columns, pool, suffixes, prefixes, claims = case["columns"], case["pool"], case["suffixes"], case["prefixes"], case["claims"]
    assert len(case["mixing"]) == log2_ceil(len(claims))
    mixing_coeffs = o.arr_to_ints(eq_expand(case["mixing"]))
    max_kappa = max([suffixes[c[1]][2] for c in claims], default=0)
    assert len(case["row"]) == max_kappa
    row_coeffs = o.arr_to_ints(eq_expand(case["row"]))
    mixed = [[0] * (1 << kappa) for _off, kappa in prefixes]
    evals, transparents, memo = [], [], {}
    for i, (ci, si, pi) in enumerate(claims):
        col, level, n_vars = columns[ci]
        off, ln, kappa = suffixes[si]
        assert kappa == 7 - level and ln == n_vars - kappa
        if prefixes[pi][1] != kappa:
            raise ValueError("TowerLevelMismatch")
        suffix = pool[off : off + ln]
        if (ci, off, ln) not in memo:
            memo[(ci, off, ln)] = partial_eval(col, level, n_vars, suffix)
        scaled = [o.mul(e, mixing_coeffs[i]) for e in memo[(ci, off, ln)]]  # scale_vertical
        mixed[pi] = [a ^ b for a, b in zip(mixed[pi], scaled)]
        evals.append(fold_vertical(scaled, kappa, row_coeffs))
        transparents.append(eq_ind(suffix, kappa, mixing_coeffs[i], row_coeffs))
    return {"mixed": mixed, "row_batched_evals": evals, "transparents": transparents, "mixing_coeffs": mixing_coeffs, "row_coeffs": row_coeffs}


# ------------------------------------------------------------------------------------------------ the shapes the tests share
def _column(seed, level, n_vars):
    """Random values of the level: every bit pattern of the packed elements is one."""
    return o.random_b128(seed, 1 << (n_vars + level - 7))


def _points(seed, n_points, n_vars):
    return [o.random_scalars(seed + 7919 * p, n_vars) for p in range(n_points)]


def build_case(seed, columns, claim_points):
    """columns: [(level, n_vars)]; claim_points: [(column, point id)] or [(column, prefix point id, suffix point id)] -- every point id
    is one random point of max n_vars coordinates whose low coordinates every column reads: prefix = the low kappa of the prefix point,
    suffix = the next n_vars - kappa of the suffix point.  Suffix and prefix descriptors are the distinct (point, kappa, len) and
    (point, kappa)."""
    claim_points = [(cp[0], cp[1], cp[-1]) for cp in claim_points]
    max_n = max(n for _l, n in columns)
    n_points = 1 + max(max(pp, ps) for _c, pp, ps in claim_points)
    pts = _points(seed, n_points, max_n)
    pool = [x for pt in pts for x in pt]
    cols = [(_column(seed + 31 * c + 1, level, n), level, n) for c, (level, n) in enumerate(columns)]
    suffixes, prefixes, claims, s_ids, p_ids = [], [], [], {}, {}
    for c, pp, ps in claim_points:
        level, n = columns[c]
        kappa = 7 - level
        s_key, p_key = (ps, kappa, n - kappa), (pp, kappa)
        if s_key not in s_ids:
            s_ids[s_key] = len(suffixes)
            suffixes.append((ps * max_n + kappa, n - kappa, kappa))
        if p_key not in p_ids:
            p_ids[p_key] = len(prefixes)
            prefixes.append((pp * max_n, kappa))
        claims.append((c, s_ids[s_key], p_ids[p_key]))
    max_kappa = max(s[2] for s in suffixes)
    return {"columns": cols, "pool": pool, "suffixes": suffixes, "prefixes": prefixes, "claims": claims,
            "mixing": o.random_scalars(seed + 3, log2_ceil(len(claims))), "row": o.random_scalars(seed + 5, max_kappa)}


def seven_claim_case(seed=0x7C1A):
    """Seven claims over four columns at levels 0, 3, 5, 7 with 11, 10, 9, 9 variables: the bit column at two points (two prefixes that
    share kappa = 7, two suffixes), the byte column at two points that share their prefix (one prefix mixes two claims), the B32 column
    at one, the B128 column at two (kappa = 0: the empty prefix, mixed as well)."""
    return build_case(seed, [(0, 11), (3, 10), (5, 9), (7, 9)], [(0, 0), (0, 1), (1, 0, 0), (1, 0, 1), (2, 0), (3, 0, 0), (3, 0, 1)])


def keccak_case(seed=0x6ECC, n_vars=13):
    """The claim graph of the keccak circuit at reduced size: 100 one-bit columns of 2^n_vars values, 175 claims at three points (75
    columns are claimed at two of them), three suffixes, three prefixes."""
    pts = [(c, c % 3) for c in range(100)] + [(c, (c + 1) % 3) for c in range(75)]
    return build_case(seed, [(0, n_vars)] * 100, sorted(pts))


def u32_add_case(seed=0x0ADD, log_rows=10):
    """u32_add: xin, yin, cout, zout as one-bit columns of 32 bits a row; cout is also claimed at the point of its shifted copy: five
    claims over four columns, two suffixes."""
    return build_case(seed, [(0, log_rows + 5)] * 4, [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0)])
