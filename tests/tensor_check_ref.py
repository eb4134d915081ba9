"""The plain definition of "this table is a tensor expansion up to a constant", and tables that break it in exactly one place.

The weighted shadow of the literal MLE-check (csrc/abi_kernels.cpp "weighted shadow") may replace the caller's indicator table by the
ratios rho_k = t[2^k] / t[0] only if

    t[i] == t[i - 2^k] * rho_k      for every i in [1, n), k the top bit of i

holds everywhere; k_check_tensor / k_check_tensor_head (csrc/kernels_misc.hip) decide that on the device.

  expansion(coords)        the tensor expansion of the coordinates (oracle.tensor_expand)
  failing(table)           every i at which the equation above does not hold, straight from the definition -- one oracle.mul_vec per
                           range, no workgroups, no strides; None where the ratios do not exist
  isolate(table, p, kappa) a table in which the equation fails at i = p and NOWHERE else
  probe_indices(K)         the entries of a 2^K table that stand for one class of the kernel's index logic each
  visits(K, narrowed)      a model of the kernels' partition, and of five ways to get it wrong: what the probes are measured against

Why isolate() works: let k0 be the top bit of p, p no power of two, and scale every entry whose index is congruent to p modulo
2^(k0+1) by kappa (not 0, not 1).  An index i = p + h * 2^(k0+1), h > 0, has its top bit j above k0, and its predecessor i - 2^j
has the same low k0 + 1 bits: both sides of its equation are scaled.  Nor is a scaled index the predecessor of an unscaled one: i
is compared with i - 2^j for j the top bit of i, which lies above the top bit of the predecessor and so above k0 -- adding it keeps
the low k0 + 1 bits.  t[0] and every t[2^j] keep their values (p is no power of two, and neither is p + h * 2^(k0+1)), so every ratio is unchanged.  What
is left is i = p itself, against the unscaled t[p - 2^k0].  Pinned for every index used by tests/test_oracle_tensor_check.py."""
import numpy as np

import oracle as o

M64 = (1 << 64) - 1
KAPPA = 0x6A09E667F3BCC908B2FB1366EA957D3E  # any constant outside {0, 1}


def expansion(coords):
    t = o.arr(1 << len(coords))
    t[0] = (1, 0)
    assert o.tensor_expand(t, 0, list(coords)) == 0
    return t


def _const(value, n):
    c = o.arr(n)
    c[:] = (value & M64, value >> 64)
    return c


def _at(t, i):
    return int(t[i, 0]) | (int(t[i, 1]) << 64)


def scale(table, kappa):
    """Every entry times kappa."""
    return o.mul_vec(np.ascontiguousarray(table), _const(kappa, table.shape[0]))


def failing(table):
    """Sorted list of the i in [1, n) with t[i] != t[i - 2^k] * rho_k; None when t[0], some t[2^k] or t[0] ^ t[2^k] is zero (a
    coordinate 0 or 1: there are no ratios to speak of)."""
    n = table.shape[0]
    K = n.bit_length() - 1
    assert n == 1 << K
    t0 = _at(table, 0)
    heads = [_at(table, 1 << k) for k in range(K)]
    if t0 == 0 or any(h == 0 or h ^ t0 == 0 for h in heads):
        return None
    inv0 = o.invert(t0)
    bad = []
    for k in range(K):
        lo = 1 << k
        want = o.mul_vec(np.ascontiguousarray(table[:lo]), _const(o.mul(heads[k], inv0), lo))
        got = table[lo : 2 * lo]
        bad.extend(int(lo + j) for j in np.flatnonzero((want[:, 0] != got[:, 0]) | (want[:, 1] != got[:, 1])))
    return bad


def isolate(table, p, kappa=KAPPA):
    """The table with every entry of index p modulo 2^(k0+1) scaled by kappa, k0 the top bit of p: for p no power of two the only
    failing comparison is the one at p.  (For p a power of two, or p = 0, use alter(): scaling the whole class would scale t[2^k0]
    AND everything built on it.)"""
    assert p >= 1 and p & (p - 1) and kappa not in (0, 1)
    step = 2 << (p.bit_length() - 1)
    t = table.copy()
    t[p::step] = scale(t[p::step], kappa)
    return t


def alter(table, p, kappa=KAPPA):
    """One entry scaled by kappa.  At p = 2^k0 that is a DEFINING entry: rho_k0 changes, and so does what every i = 2^k0 + 2^j,
    j > k0, is compared with; at p = 0 every ratio changes."""
    t = table.copy()
    t[p : p + 1] = scale(t[p : p + 1], kappa)
    return t


def flip(table, p, bit):
    t = table.copy()
    t[p, bit >> 6] ^= np.uint64(1 << (bit & 63))
    return t


# ---- which entries stand for what
TIDS = (0, 63, 64, 255)
HEAD = (3, 5, 127, 129, 255)


def range_workgroups(k):
    """Workgroups dealt to the range [2^k, 2^(k+1)): one per 4096 entries, at least 1, at most 512."""
    return min(max((1 << k) // 4096, 1), 512)


def range_trips(k):
    """Loop trips of one workgroup of range k: it takes 1024 entries per trip, its range's workgroups together n_wg * 1024."""
    return max((1 << k) // (range_workgroups(k) * 1024), 1)


def where(p):
    """(k, part, trip, j, lane): the range of entry p, and for k >= 8 the workgroup of the range, the loop trip, the slot of the four
    in flight and the lane that compare it; in the head (k < 8) the lane is p itself."""
    k = p.bit_length() - 1
    if k < 8:
        return k, 0, 0, 0, p
    off, stride = p - (1 << k), range_workgroups(k) * 1024
    return k, off % stride // 1024, off // stride, off % 1024 // 256, off % 256


def describe(K, p):
    k, part, trip, j, lane = where(p)
    if k < 8:
        return "K = %d, p = %d: head kernel, range %d, lane %d" % (K, p, k, lane)
    return "K = %d, p = %d: range %d, part %d of %d, trip %d of %d, j = %d, lane %d" % (K, p, k, part, range_workgroups(k), trip, range_trips(k), j, lane)


def visits(K, narrowed=None):
    """A model of the PARTITION of k_check_tensor_head / k_check_tensor / check_tensor_layout -- which entries of a 2^K table get
    compared, as a list with repetitions -- written down from the kernels' index arithmetic; `narrowed` names one way of getting
    that arithmetic wrong so that entries are left out.  It says nothing about the device code (the GPU probes do that): it is here
    so that the CPU suite can show that every such narrowing leaves out an entry the GPU tests probe."""
    n, seen = 1 << K, []
    seen.extend(i for i in range(1, min(n, 128 if narrowed == "head" else 256)))
    if K <= 8:
        return seen
    first, wg = [], 0
    for k in range(42):
        first.append(wg)
        if 8 <= k < K:
            wg += range_workgroups(k)
    for block in range(wg):
        k = 8
        while k + 1 < K and (block > first[k + 1] if narrowed == "lookup" else block >= first[k + 1]):
            k += 1
        lo, hi, n_wg, part = 1 << k, 2 << k, first[k + 1] - first[k], block - first[k]
        if narrowed == "part":
            part %= max(n_wg - 1, 1)
        end = hi - n_wg * 1024 if narrowed == "bound" and hi - lo > n_wg * 1024 else hi
        for tid in range(256):
            i0 = lo + part * 1024 + tid
            while i0 < end and i0 < n:
                seen.extend(i0 + 256 * j for j in range(3 if narrowed == "slot" else 4) if i0 + 256 * j < hi and i0 + 256 * j < n)
                i0 += n_wg * 1024
    return seen


NARROWINGS = ("head", "lookup", "part", "bound", "slot")


def probe_indices(K, tids=TIDS):
    """Ascending, for a table of 2^K entries.  Per range k = 8 .. K - 1, dealt to n_wg workgroups:

        2^k + part * 1024 + trip * n_wg * 1024 + 256 * j + tid,   part in {0, n_wg - 1}, trip in {0, last}, j = 0 .. 3, tid in tids

    kept where below 2^(k+1) and no power of two; the range's last entry and 2^k + 1; and the head's 3, 5, 127, 129, 255."""
    out = set(HEAD)
    for k in range(8, K):
        lo, n_wg, trips = 1 << k, range_workgroups(k), range_trips(k)
        for part in (0, n_wg - 1):
            for trip in (0, trips - 1):
                for j in range(4):
                    for tid in tids:
                        p = lo + part * 1024 + trip * n_wg * 1024 + 256 * j + tid
                        if p < 2 * lo and p & (p - 1):
                            out.add(p)
        out.update((lo + 1, 2 * lo - 1))
    return sorted(out)
