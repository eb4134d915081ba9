"""TEST INFRASTRUCTURE: CPU restatement of the univariate round of the univariate-skip zerocheck
(crates/core/src/protocols/sumcheck/prove/univariate.rs:235-507 zerocheck_univariate_evals, :571-640 extrapolate_round_evals) for
the domain field B8, built from the oracle's pinned field: B8 products from o.gf_mul(a, b, 3) (one 256 x 256 table, used with numpy
indexing), GF(2^128) products from o.mul.  The univariatized columns are brute-force Lagrange over the B8 points omega_j = j and the
extrapolation is plain Lagrange interpolation through all d 2^k points -- no NTT, no GF(2)-linear masks, nothing shared with
binius_amd/csrc/kernels_univariate.hip.

  univariate_evals(cols, n_vars, k, comps, degrees, eq_challenges, D, batch_coeff=None)
      cols: [(values, level)] with values a numpy uint8 array of the 2^n_vars column values (B1 as 0 / 1, B8 as bytes);
      returns per composition [P_c(omega_j) for 2^k <= j < D] or, with batch_coeff, sum_c batch_coeff^c P_c.
  fold(values, k, coeffs)             the univariate round's fold at the Lagrange coefficients (pinned against o.fold_right)
  message_at / claim_at               the two sides of the verifier's equation at a challenge z in GF(2^128)"""
import numpy as np

import oracle as o

_TABLES = None


def b8_tables():
    """(mul[256, 256], inv[256]) of B8 in the tower basis, from the oracle's gf_mul at level 3."""
    global _TABLES
    if _TABLES is None:
        mul = np.zeros((256, 256), dtype=np.uint8)
        for a in range(256):
            for b in range(a, 256):
                mul[a, b] = mul[b, a] = o.gf_mul(a, b, 3)
        inv = np.zeros(256, dtype=np.uint8)
        for a in range(1, 256):
            inv[a] = int(np.nonzero(mul[a] == 1)[0][0])
        _TABLES = (mul, inv)
    return _TABLES


def lagrange_matrix(n, points):
    """W[r, p] = ell_p(omega_{points[r]}) for the Lagrange basis over omega_0 .. omega_{n-1}: the products
    prod_{q != p} (x - omega_q) / (omega_p - omega_q), one factor at a time."""
    mul, inv = b8_tables()
    pts = np.asarray(points, dtype=np.int64)
    W = np.zeros((len(pts), n), dtype=np.uint8)
    for p in range(n):
        num, den = np.ones(len(pts), dtype=np.uint8), 1
        for q in range(n):
            if q != p:
                num = mul[num, pts ^ q]
                den = int(mul[den, p ^ q])
        W[:, p] = mul[num, inv[den]]
    return W


def unpack(col, level, n_vars):
    """A packed column (numpy (len, 2) uint64, the layout of bn_hal_multilinear TRANSPARENT) -> its 2^n_vars values as uint8."""
    b = np.ascontiguousarray(col).view(np.uint8).reshape(-1)
    if level == 3:
        return b[: 1 << n_vars].copy()
    return np.unpackbits(b, bitorder="little")[: 1 << n_vars].astype(np.uint8)


def pack(values, level):
    """The inverse of unpack: values (uint8) -> (len, 2) uint64 array, at least one element."""
    v = np.asarray(values, dtype=np.uint8)
    raw = np.packbits(v, bitorder="little") if level == 0 else v
    n_el = max(1, (len(raw) + 15) // 16)
    buf = np.zeros(16 * n_el, dtype=np.uint8)
    buf[: len(raw)] = raw
    return buf.view(np.uint64).reshape(n_el, 2).copy()


def b8_times_b128(v, e_bytes):
    """v (B8, any shape S) times GF(2^128) elements given as bytes (shape S + (16,)): the product, as bytes.  In the tower basis a
    B8 scalar acts on each of the 16 B8 coordinates (pinned against o.mul by tests/test_univariate_skip_oracle.py)."""
    mul, _ = b8_tables()
    return mul[np.asarray(v)[..., None], e_bytes]


def bytes_to_int(b):
    return int.from_bytes(bytes(np.asarray(b, dtype=np.uint8)), "little")


def int_to_bytes(x):
    return np.frombuffer(int(x).to_bytes(16, "little"), dtype=np.uint8).copy()


def eq_expansion(challenges):
    """The tensor expansion of the zerocheck challenges (challenge t on bit t of x), as ints, through the oracle."""
    eq = o.arr(1 << len(challenges))
    eq[0] = o.ints_to_arr([1])[0]
    o.tensor_expand(eq, 0, list(challenges))
    return o.arr_to_ints(eq)


def eval_steps_b8(steps, var):
    """A composition's steps over B8 on numpy arrays; var(i) gives the values of variable i."""
    mul, _ = b8_tables()
    r = []
    for s in steps:
        if s[0] == "var":
            r.append(var(s[1]))
        elif s[0] == "const":
            assert s[1] < 256
            r.append(np.uint8(s[1]))
        elif s[0] == "add":
            r.append(np.bitwise_xor(r[s[1]], r[s[2]]))
        elif s[0] == "mul":
            r.append(mul[r[s[1]], r[s[2]]])
        else:  # pow by repeated multiplication
            base, acc = r[s[1]], np.uint8(1)
            for _ in range(s[2]):
                acc = mul[acc, base]
            r.append(acc)
    return r[-1]


def round_evals(cols, n_vars, k, steps, degree, eq_ints):
    """R_c(omega_j) for 2^k <= j < d 2^k: sum_x eq(x) C(Mhat_1(omega_j, x), ...), as ints."""
    K, d = 1 << k, degree
    js = list(range(K, d * K))
    if not js:
        return []
    W = lagrange_matrix(K, js)  # [len(js), K]
    mul, _ = b8_tables()
    n_x = 1 << (n_vars - k)
    cache = {}

    def var(i):
        if i not in cache:
            blocks = cols[i][0].reshape(n_x, K)  # [x, u]
            prod = mul[W[:, None, :], blocks[None, :, :]]  # [j, x, u]
            cache[i] = np.bitwise_xor.reduce(prod, axis=2)  # Mhat_i(omega_j, x)
        return cache[i]

    v = np.broadcast_to(eval_steps_b8(steps, var), (len(js), n_x))
    e_bytes = np.stack([int_to_bytes(e) for e in eq_ints])  # [x, 16]
    terms = b8_times_b128(v, e_bytes[None, :, :])  # [j, x, 16]
    sums = np.bitwise_xor.reduce(terms, axis=1)  # [j, 16]
    return [bytes_to_int(s) for s in sums]


def extrapolate(k, degree, D, r):
    """P(omega_j), 2^k <= j < D, of the polynomial of degree < d 2^k that is 0 on omega_0 .. omega_{2^k - 1} and r on the rest of
    omega_0 .. omega_{d 2^k - 1}: plain Lagrange interpolation through all d 2^k points."""
    K, N = 1 << k, degree << k
    if degree < 2:
        return [0] * (D - K)
    vals = [0] * K + list(r)
    out = list(r[: max(0, min(N, D) - K)])
    if D > N:
        W = lagrange_matrix(N, range(N, D))
        for row in W:
            acc = np.zeros(16, dtype=np.uint8)
            for p in range(K, N):
                acc ^= b8_times_b128(np.uint8(row[p]), int_to_bytes(vals[p]))
            out.append(bytes_to_int(acc))
    return out


def lagrange_at(n, z):
    """ell_p(z), p < n, over omega_0 .. omega_{n-1}, z in GF(2^128) outside the domain: plain products with o.mul / o.invert."""
    out = []
    for p in range(n):
        num, den = 1, 1
        for q in range(n):
            if q != p:
                num = o.mul(num, z ^ q)
                den = o.mul(den, p ^ q)
        out.append(o.mul(num, o.invert(den)))
    return out


def fold(values, k, coeffs):
    """The univariate round's fold (evaluate_partial_low at the Lagrange coefficients, univariate.rs:139-195):
    out[x] = sum_u coeffs[u] M(u + 2^k x), as ints."""
    K = 1 << k
    c_bytes = np.stack([int_to_bytes(c) for c in coeffs])  # [u, 16]
    blocks = np.asarray(values, dtype=np.uint8).reshape(-1, K)  # [x, u]
    terms = b8_times_b128(blocks, c_bytes[None, :, :])  # [x, u, 16]
    return [bytes_to_int(s) for s in np.bitwise_xor.reduce(terms, axis=1)]


def message_at(k, D, message, z):
    """The verifier's side (verify_zerocheck.rs:92-112): the univariate message (zeros on the first 2^k points) interpolated over
    omega_0 .. omega_{D-1} and evaluated at z."""
    ell = lagrange_at(D, z)
    acc = 0
    for j, v in enumerate(message, start=1 << k):
        acc ^= o.mul(v, ell[j])
    return acc


def claim_at(vals, n_vars, k, steps, eq_ints, z):
    """What the message must evaluate to at z: sum_x eq(x) C(Mhat_1(z, x), ...), Mhat_i(z, x) = sum_u L_u(z) M_i(u + 2^k x),
    in GF(2^128) (the univariatized columns through fold, the composition through o.circuit_eval)."""
    L = lagrange_at(1 << k, z)
    used = sorted({s[1] for s in steps if s[0] == "var"})
    hat = {i: fold(vals[i], k, L) for i in used}
    total = 0
    for x in range(1 << (n_vars - k)):
        q = [0] * (max(used) + 1)
        for i in used:
            q[i] = hat[i][x]
        total ^= o.mul(eq_ints[x], o.circuit_eval(steps, q))
    return total


def univariate_evals(cols, n_vars, k, comps, degrees, eq_challenges, D, batch_coeff=None):
    eq_ints = eq_expansion(eq_challenges)
    per = [extrapolate(k, d, D, round_evals(cols, n_vars, k, steps, d, eq_ints)) for steps, d in zip(comps, degrees)]
    if batch_coeff is None:
        return per
    out, scale = [0] * (D - (1 << k)), 1
    for p in per:
        out = [a ^ o.mul(scale, b) for a, b in zip(out, p)]
        scale = o.mul(scale, batch_coeff)
    return out
