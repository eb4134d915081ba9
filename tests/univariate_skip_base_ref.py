"""TEST INFRASTRUCTURE: CPU restatement of the univariate-skip zerocheck for every arm of core/src/constraint_system/prove.rs:483-490
(3 => B8, 4 => B16, 5 => B32, 6 => B64, 7 => B128), written from the reference's equations; it does not import binius_amd.

The mathematics does not depend on the arm -- P_c(omega_j) is the same field element whichever subfield the prover computes in:
the domain and the Lagrange coefficients L_u(omega_j) stay in B8, Mhat_i(omega_j, x) = sum_u L_u(omega_j) M_i(u + 2^k x) is a
B8 x FBase product (in the tower basis the B8 scalar acts on each byte coordinate: the table univariate_skip_ref.b8_tables(),
vectorised), the composition is evaluated in FBase (o.gf_mul at the base level, o.mul at level 7) and eq(x) * v is a B128 x FBase
product (o.mul).  Brute-force Lagrange over the B8 points; the level-independent parts (Lagrange coefficients, extrapolation, the
multilinear rounds, the reduction, verify) are those of tests/univariate_skip_ref.py and tests/zerocheck_skip_ref.py.

A column is (values, level): level 0 / 3 as in univariate_skip_ref (a uint8 array of 0 / 1 or of bytes), level 4 .. 7 a uint8 array of
shape (2^n_vars, 2^(level - 3)) -- the little-endian bytes of every value.

  univariate_evals(base, cols, n_vars, k, comps, degrees, eq_challenges, D, batch_coeff=None)     the univariate round
  pack / unpack                    values <-> the (len, 2) uint64 layout of bn_hal_multilinear TRANSPARENT, every level
  table_base(table)                the table's arm (prove.rs:458-467): the largest column level and constant level, at least 3
  prove(tables, k, ...)            the whole batched prover for mixed-level tables (the dict of zerocheck_skip_ref.prove)
  column_evals(tables, k, skipped, unskipped)    every ORIGINAL column's multilinear extension at the output point"""
import numpy as np

import oracle as o
import univariate_skip_ref as R
import zerocheck_skip_ref as Z


def as_bytes(values):
    """(N,) or (N, W) uint8 -> (N, W)."""
    v = np.asarray(values, dtype=np.uint8)
    return v.reshape(len(v), -1)


def to_ints(values):
    """The column's values as Python ints."""
    b = as_bytes(values)
    return [int.from_bytes(bytes(row), "little") for row in b]


def wide(values, level):
    """B1 / B8 values (a uint8 array) zero-extended into a column of the given level >= 3."""
    v = np.asarray(values, dtype=np.uint8)
    out = np.zeros((len(v), 1 << (level - 3)), dtype=np.uint8)
    out[:, 0] = v
    return out if level > 3 else v


def from_ints(ints, level):
    """Python ints below 2^(2^level) -> a column of the given level >= 3."""
    w = 1 << (level - 3)
    out = np.frombuffer(b"".join(int(x).to_bytes(w, "little") for x in ints), dtype=np.uint8).reshape(len(ints), w).copy()
    return out if level > 3 else out.reshape(-1)


def pack(values, level):
    """values -> (len, 2) uint64, at least one 16-byte element: B1 eight to the byte, wider values little-endian, back to back."""
    if level in (0, 3):
        return R.pack(np.asarray(values, dtype=np.uint8).reshape(-1), level)
    raw = as_bytes(values).reshape(-1)
    assert as_bytes(values).shape[1] == 1 << (level - 3)
    n_el = max(1, (len(raw) + 15) // 16)
    buf = np.zeros(16 * n_el, dtype=np.uint8)
    buf[: len(raw)] = raw
    return buf.view(np.uint64).reshape(n_el, 2).copy()


def unpack(col, level, n_vars):
    if level in (0, 3):
        return R.unpack(col, level, n_vars)
    w = 1 << (level - 3)
    b = np.ascontiguousarray(col).view(np.uint8).reshape(-1)
    return b[: w << n_vars].reshape(1 << n_vars, w).copy()


def const_level(c):
    level = 0
    while c >> (1 << level):
        level += 1
    return level


def table_base(table):
    levels = [level for _, level in table["cols"]]
    for comp in table["comps"]:
        levels += [const_level(s[1]) for s in comp[0] if s[0] == "const"]
    return max([3] + levels)


def base_mul(a, b, base):
    return o.mul(a, b) if base == 7 else o.gf_mul(a, b, base)


def eval_steps(steps, var, base, count):
    """A composition's steps over T_base on lists of `count` Python ints; var(i) gives the values of variable i."""
    r = []
    for s in steps:
        if s[0] == "var":
            r.append(var(s[1]))
        elif s[0] == "const":
            assert s[1] >> (1 << base) == 0
            r.append([s[1]] * count)
        elif s[0] == "add":
            r.append([a ^ b for a, b in zip(r[s[1]], r[s[2]])])
        elif s[0] == "mul":
            r.append([base_mul(a, b, base) for a, b in zip(r[s[1]], r[s[2]])])
        else:  # pow by repeated multiplication
            acc = [1] * count
            for _ in range(s[2]):
                acc = [base_mul(a, b, base) for a, b in zip(acc, r[s[1]])]
            r.append(acc)
    return r[-1]


def round_evals(base, cols, n_vars, k, steps, degree, eq_ints):
    """R_c(omega_j) for 2^k <= j < d 2^k: sum_x eq(x) C(Mhat_1(omega_j, x), ...), as ints."""
    K = 1 << k
    js = list(range(K, degree * K))
    if not js:
        return []
    W = R.lagrange_matrix(K, js)  # [j, u]
    mul, _ = R.b8_tables()
    n_x = 1 << (n_vars - k)
    cache = {}

    def var(i):
        if i not in cache:
            vals, level = cols[i]
            assert level == 0 or 3 <= level <= base
            blocks = as_bytes(vals).reshape(n_x, K, -1)  # [x, u, coordinate]
            hat = np.zeros((len(js), n_x, blocks.shape[2]), dtype=np.uint8)
            for u in range(K):  # the B8 scalar on each byte coordinate
                hat ^= mul[W[:, u][:, None, None], blocks[None, :, u, :]]
            cache[i] = to_ints(hat.reshape(len(js) * n_x, -1))  # index j * n_x + x
        return cache[i]

    v = eval_steps(steps, var, base, len(js) * n_x)
    out = []
    for jj in range(len(js)):
        acc = 0
        for x in range(n_x):
            acc ^= o.mul(eq_ints[x], v[jj * n_x + x])
        out.append(acc)
    return out


def univariate_evals(base, cols, n_vars, k, comps, degrees, eq_challenges, D, batch_coeff=None):
    eq_ints = R.eq_expansion(eq_challenges)
    per = [R.extrapolate(k, d, D, round_evals(base, cols, n_vars, k, steps, d, eq_ints)) for steps, d in zip(comps, degrees)]
    if batch_coeff is None:
        return per
    out, scale = [0] * (D - (1 << k)), 1
    for p in per:
        out = [a ^ o.mul(scale, b) for a, b in zip(out, p)]
        scale = o.mul(scale, batch_coeff)
    return out


def fold(values, k, coeffs):
    """out[x] = sum_u coeffs[u] M(u + 2^k x), as ints (evaluate_partial_low at the Lagrange coefficients, univariate.rs:139-195)."""
    K = 1 << k
    v = to_ints(values)
    out = []
    for x in range(len(v) >> k):
        acc = 0
        for u in range(K):
            acc ^= o.mul(coeffs[u], v[x * K + u])
        out.append(acc)
    return out


def pad_high(values, n_vars, k):
    """high_pad_small_multilinear (prove/zerocheck.rs:79-119): 2^(k - n_vars) copies, one after the other."""
    v = np.asarray(values, dtype=np.uint8)
    return v if n_vars >= k else np.concatenate([v] * (1 << (k - n_vars)), axis=0)


def project(values, n_eff, k, unskipped):
    """project_to_skipped_variables (prove/zerocheck.rs:472-516): evaluate_partial_high at the last n_eff - k unskipped challenges."""
    q = n_eff - k
    eqq = R.eq_expansion(unskipped[len(unskipped) - q:])
    v = to_ints(values)
    out = []
    for u in range(1 << k):
        acc = 0
        for y in range(1 << q):
            acc ^= o.mul(eqq[y], v[(y << k) + u])
        out.append(acc)
    return out


def prove(tables, k, zerocheck_challenges, batch_coeffs, univariate_challenge, sumcheck_challenges, reduction_batch_coeff, reduction_challenges):
    """zerocheck_skip_ref.prove with every table's univariate round in its own arm and columns of any level."""
    from oracle.zerocheck_ref import eqind_sumcheck_prove

    rounds, D, d_max, degrees = Z.batch_shape([(t["n_vars"], len(t["cols"]), t["comps"]) for t in tables], k)
    K = 1 << k
    assert len(zerocheck_challenges) == rounds and len(sumcheck_challenges) == rounds and len(batch_coeffs) == len(tables) and len(reduction_challenges) == k
    z = univariate_challenge
    l_sub, l_full = R.lagrange_at(K, z), R.lagrange_at(D, z)
    message = [0] * max(0, D - K)
    round_coeffs = [[0] * (d_max + 2) for _ in range(rounds)]
    final_evals, padded = [], []
    for t, bc, ds in zip(tables, batch_coeffs, degrees):
        n_eff = max(t["n_vars"], k)
        nr = n_eff - k
        cols = [(pad_high(v, t["n_vars"], k), level) for v, level in t["cols"]]
        padded.append((cols, n_eff))
        ch = list(zerocheck_challenges[rounds - nr:])  # (constraint_system/prove.rs:470)
        per = univariate_evals(table_base(t), cols, n_eff, k, [c[0] for c in t["comps"]], ds, ch, D)
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


def column_evals(tables, k, skipped, unskipped):
    """The multilinear extension of every ORIGINAL column at the low n_vars coordinates of skipped || the last n_vars - k of unskipped
    (a table of n_vars < k: at skipped[:n_vars]), by the tensor expansion of the point."""
    out = []
    for t in tables:
        n = t["n_vars"]
        point = list(skipped[:n]) if n < k else list(skipped) + list(unskipped[len(unskipped) - (n - k):])
        e = R.eq_expansion(point)
        for v, _ in t["cols"]:
            acc = 0
            for w, x in zip(e, to_ints(v)):
                acc ^= o.mul(w, x)
            out.append(acc)
    return out
