"""The case tables of the route tests of bn_fold_right / bn_fold_left / bn_inner_product, shared by tests/test_oracle_fold_cases.py (which
pins the tables on the CPU) and tests/test_gpu_fold_routes.py (which runs them on the device).

A fold call is answered by one of seven routes (binius_amd/csrc/abi_ops.cpp fold_common / fold_left_dispatch, launch_fold_left / _right in
kernels_misc.hip, launch_fold_right_mfma / _left_mfma in kernels_linmap.hip), an inner product by one of four, and
`Context.fold_counters()` / `Context.inner_product_counters()` say which.  A row names the route and the branches of the answering kernel
that it is there for (its tags), written out by hand; `fold_tags` / `ip_tags` below restate the routing predicates and the kernels'
constants and derive both from the shape alone, and the CPU module holds the two against each other.  A case that was chosen to reach a
branch fails when a threshold moves and it stops reaching it.

Sizes that depend on the number of compute units are written as a rule -- ("pairs", k): the smallest power of two of outputs at which a
workgroup of the matrix-core kernels takes at least k pairs of 32-row blocks; ("stride", k): at which a thread of the scalar kernel takes
at least k outputs; ("mfma", 0 / 1): the longest F x F inner product still on the 9-lane kernel / the shortest on the matrix cores -- and
resolved by `out_len` / `ip_len` for the device at hand (256 units in the CPU module).
"""
from collections import namedtuple

import numpy as np

NOMINAL_CU = 256

FOLD_ROUTES = ("right_mfma", "right_tab", "right_scalar", "left_pe", "left_mfma", "left_tab", "left_scalar")
FOLD_RINGS = ("ring2", "ring4", "ring8", "ring_left2", "ring_left4", "ring_left8")
FOLD_LAST = ("last_grid", "last_prep")  # a record of the last matrix-core launch, not counters
FOLD_INFO = ("n_cu",)                   # the device's compute units, as the launchers see them
IP_ROUTES = ("mfma_split", "split9", "ip32", "scalar")

LEVELS = (0, 3, 4, 5, 6, 7)

# ---------------------------------------------------------------------------------------------- the library's routing, restated
G = 32             # k_fold_tab: matrix entries loaded before any is looked up
TAB_TH = 1024      # k_fold_tab: outputs per workgroup
TAB_MIN_OUT = 1024
MFMA_MIN_OUT = 4096
PE_MAX_OUT = 1 << 10   # kPeMaxLogOut
PE_MIN_VEC = 4096
K_TP = 256         # gram.hpp kTP: points per tile of the matrix-core sum of products


def tab_consts(level):
    """P nibbles per entry, J vectors per 64 KiB LDS chunk, KG entries per lookup group, EB bytes per entry, NU4 16-byte loads per full group."""
    assert level in (3, 4, 5)
    P = (1 << level) // 4
    return {"P": P, "J": 256 // P, "G": min(256 // P, 32), "KG": max(16 // P, 1), "EB": (1 << level) // 8, "NU4": G * ((1 << level) // 8) // 16}


def fold_route(op, level, vec_len, out_len):
    assert op in ("left", "right") and level in LEVELS
    if op == "left":
        if out_len <= PE_MAX_OUT and vec_len >= PE_MIN_VEC:
            return "left_pe"
        if level == 5 and out_len >= MFMA_MIN_OUT and out_len % 64 == 0 and vec_len in (16, 32, 64):
            return "left_mfma"
    elif out_len >= MFMA_MIN_OUT and out_len % 64 == 0 and (vec_len << level) in (512, 1024, 2048):
        return "right_mfma"
    if out_len >= TAB_MIN_OUT and level in (3, 4, 5):
        return op + "_tab"
    return op + "_scalar"


def ring_grid(out_len, n_cu):
    return min(out_len // 64, 2 * n_cu)


def ring_pairs(out_len, n_cu):
    """pairs of 32-row blocks that the busiest workgroup of k_linmap_ring / k_linmap_ring_left takes"""
    return -(-(out_len // 64) // ring_grid(out_len, n_cu))


def scalar_outputs_per_thread(out_len, n_cu):
    grid = min(-(-out_len // 256), 8 * n_cu)
    return -(-out_len // (256 * grid))


def _pairs_class(p):
    return 1 if p == 1 else 2 if p < 4 else 4


def fold_tags(op, level, vec_len, out_len, n_cu=NOMINAL_CU):
    """(route, tags) of a fold of this shape on a device with n_cu compute units."""
    route = fold_route(op, level, vec_len, out_len)
    tags = set()
    if route.endswith("_tab"):
        c = tab_consts(level)
        if op == "left":
            tags.add("tab:left")
        elif c["NU4"] >= 1 and vec_len % c["G"] == 0:
            tags.add("tab:wide@%d" % level)  # (chunks and vec_len are multiples of G: every group is full)
        else:
            tags.add("tab:narrow-right")
        if vec_len > c["J"]:
            tags.add("tab:chunks>=2@%d" % level)
        if vec_len == 1:
            tags.add("tab:vec1")
        if min(vec_len, c["J"]) < c["G"]:
            tags.add("tab:partial-group")
        if out_len > TAB_TH:
            tags.add("tab:blocks>=2")
    elif route.endswith("_scalar"):
        tags.add("scalar@%d" % level)
        if scalar_outputs_per_thread(out_len, n_cu) >= 2:
            tags.add("scalar:stride")
        if out_len == 1:
            tags.add("scalar:out1")
        if vec_len == 1:
            tags.add("scalar:vec1")
    elif route.endswith("_mfma"):
        R = (vec_len << level) // 256
        assert R in (2, 4, 8)
        p = ring_pairs(out_len, n_cu)
        tags.add("%s<%d>:pairs=%d" % ("ring_left" if op == "left" else "ring", R, _pairs_class(p)))
        if op == "right" and p >= 2:
            tags.add("ring:prep<%d>:pairs>=2" % level)
    else:
        tags.add("left:pe-routed")
    return route, frozenset(tags)


def fold_counters(op, level, vec_len, out_len, n_cu):
    """What one accepted call of this shape adds to Context.fold_counters() (FOLD_ROUTES and FOLD_RINGS), and what it leaves in the
    last-launch record (None: the record is not touched)."""
    route = fold_route(op, level, vec_len, out_len)
    d = {k: 0 for k in FOLD_ROUTES + FOLD_RINGS}
    d[route] = 1
    last = None
    if route.endswith("_mfma"):
        d[("ring_left%d" if op == "left" else "ring%d") % ((vec_len << level) // 256)] = 1
        last = {"last_grid": ring_grid(out_len, n_cu), "last_prep": level}
    return d, last


def mfma_applies(n_cu, n_points):
    """bn::mfma_applies (kernels_roundeval_mfma.hip) without its measurement switches: at least one tile per compute unit"""
    return -(-n_points // K_TP) >= n_cu


def ip_route(level, b_len, n_cu=NOMINAL_CU):
    assert level in LEVELS and b_len % (1 << (7 - level)) == 0
    if level == 7 and b_len >= 2 and b_len % 2 == 0:
        return "mfma_split" if mfma_applies(n_cu, b_len // 2) else "split9"
    if level == 5 and b_len >= 8192 and b_len % 512 == 0:
        return "ip32"
    return "scalar"


def ip_tags(level, b_len, n_cu=NOMINAL_CU):
    route = ip_route(level, b_len, n_cu)
    tags = {"ip:%s@%d" % (route, level)}
    if b_len & (b_len - 1):
        tags.add("ip:not-pow2@%d" % level)
    if level == 5:
        if route == "ip32":
            # (k_ip32: a wave takes batches of 512 elements, a workgroup has four waves)
            tags.add("ip32:at-threshold" if b_len == 8192 else "ip32:ragged" if (b_len // 512) % 4 else "ip32:whole")
        elif b_len >= 8192:
            tags.add("ip5:not-512")
        elif b_len >= 7680:
            tags.add("ip5:below-8192")
    if level == 7:
        if b_len % 2:
            tags.add("ip7:odd")
        if b_len <= 3:
            tags.add("ip7:len%d" % b_len)
        half = b_len // 2
        if route == "split9" and mfma_applies(n_cu, half + 1):
            tags.add("ip7:last-on-9-lane")
        if route == "mfma_split" and not mfma_applies(n_cu, half - 1):
            tags.add("ip7:first-on-matrix-cores")
    return route, frozenset(tags)


# ---------------------------------------------------------------------------------------------- the fold cases
FoldCase = namedtuple("FoldCase", "id op level vec_len out route tags")


def _f(op, level, vec_len, out, route, *tags):
    o = out if isinstance(out, int) else "%s%d" % out
    return FoldCase("%s-l%d-v%d-o%s" % (op, level, vec_len, o), op, level, vec_len, out, route, frozenset(tags))


FOLD_CASES = [
    # ---- k_fold_tab, fold_right: the wide loads (byte / halfword / word extraction of mm[k]), one and two LDS chunks
    _f("right", 3, 32, 1024, "right_tab", "tab:wide@3"),
    _f("right", 3, 256, 1024, "right_tab", "tab:wide@3", "tab:chunks>=2@3"),   # 2048-bit rows, below 4096 outputs: not the matrix cores
    _f("right", 3, 512, 2048, "right_tab", "tab:wide@3", "tab:chunks>=2@3", "tab:blocks>=2"),   # four chunks
    _f("right", 4, 32, 1024, "right_tab", "tab:wide@4"),
    _f("right", 4, 128, 1024, "right_tab", "tab:wide@4", "tab:chunks>=2@4"),
    _f("right", 5, 32, 1024, "right_tab", "tab:wide@5"),
    _f("right", 5, 64, 2048, "right_tab", "tab:wide@5", "tab:chunks>=2@5", "tab:blocks>=2"),
    # ---- k_fold_tab, fold_left: the same vector lengths, two workgroups
    _f("left", 3, 32, 2048, "left_tab", "tab:left", "tab:blocks>=2"),
    _f("left", 3, 256, 2048, "left_tab", "tab:left", "tab:chunks>=2@3", "tab:blocks>=2"),
    _f("left", 4, 32, 2048, "left_tab", "tab:left", "tab:blocks>=2"),
    _f("left", 4, 128, 2048, "left_tab", "tab:left", "tab:chunks>=2@4", "tab:blocks>=2"),
    _f("left", 5, 32, 2048, "left_tab", "tab:left", "tab:blocks>=2"),           # 32 B32 columns, below 4096 outputs: not the matrix cores
    _f("left", 5, 64, 2048, "left_tab", "tab:left", "tab:chunks>=2@5", "tab:blocks>=2"),
    # ---- k_fold_tab with fewer vectors than a group: the jj < jn mask, the `on` flag, the break of the lookup groups
    _f("right", 3, 1, 1024, "right_tab", "tab:narrow-right", "tab:vec1", "tab:partial-group"),
    _f("right", 4, 1, 1024, "right_tab", "tab:narrow-right", "tab:vec1", "tab:partial-group"),
    _f("right", 5, 1, 1024, "right_tab", "tab:narrow-right", "tab:vec1", "tab:partial-group"),
    _f("right", 3, 2, 1024, "right_tab", "tab:narrow-right", "tab:partial-group"),
    _f("right", 4, 2, 1024, "right_tab", "tab:narrow-right", "tab:partial-group"),
    _f("right", 5, 2, 1024, "right_tab", "tab:narrow-right", "tab:partial-group"),
    _f("left", 3, 1, 1024, "left_tab", "tab:left", "tab:vec1", "tab:partial-group"),
    _f("left", 4, 1, 1024, "left_tab", "tab:left", "tab:vec1", "tab:partial-group"),
    _f("left", 5, 1, 1024, "left_tab", "tab:left", "tab:vec1", "tab:partial-group"),
    _f("left", 3, 2, 1024, "left_tab", "tab:left", "tab:partial-group"),
    _f("left", 4, 2, 1024, "left_tab", "tab:left", "tab:partial-group"),
    _f("left", 5, 2, 1024, "left_tab", "tab:left", "tab:partial-group"),
    # ---- k_fold: a thread's second output (the grid is capped at 8 workgroups per compute unit)
    _f("right", 0, 2, ("stride", 2), "right_scalar", "scalar@0", "scalar:stride"),
    _f("right", 6, 2, ("stride", 2), "right_scalar", "scalar@6", "scalar:stride"),
    _f("right", 7, 2, ("stride", 2), "right_scalar", "scalar@7", "scalar:stride"),
    _f("left", 0, 2, ("stride", 2), "left_scalar", "scalar@0", "scalar:stride"),
    _f("left", 6, 2, ("stride", 2), "left_scalar", "scalar@6", "scalar:stride"),
    # ---- k_fold: one output under a query as long as the evaluations; one vector element
    _f("right", 0, 1024, 1, "right_scalar", "scalar@0", "scalar:out1"),
    _f("right", 7, 1024, 1, "right_scalar", "scalar@7", "scalar:out1"),
    _f("left", 0, 1024, 1, "left_scalar", "scalar@0", "scalar:out1"),
    _f("left", 7, 1024, 1, "left_scalar", "scalar@7", "scalar:out1"),
    _f("right", 0, 1, 128, "right_scalar", "scalar@0", "scalar:vec1"),
    _f("right", 7, 1, 64, "right_scalar", "scalar@7", "scalar:vec1"),
    _f("left", 0, 1, 128, "left_scalar", "scalar@0", "scalar:vec1"),
    _f("left", 6, 1, 64, "left_scalar", "scalar@6", "scalar:vec1"),
    _f("right", 7, 1, 1, "right_scalar", "scalar@7", "scalar:out1", "scalar:vec1"),
    # ---- k_fold at the levels of the table kernel, below its 1024 outputs
    _f("right", 3, 4, 512, "right_scalar", "scalar@3"),
    _f("left", 4, 4, 512, "left_scalar", "scalar@4"),
    _f("right", 5, 1, 512, "right_scalar", "scalar@5", "scalar:vec1"),
    _f("left", 5, 8, 512, "left_scalar", "scalar@5"),
    # ---- k_linmap_ring<R>: one pair per workgroup; a second pair in the LDS ring behind every table preparation; four pairs
    _f("right", 3, 64, 4096, "right_mfma", "ring<2>:pairs=1"),
    _f("right", 4, 64, 4096, "right_mfma", "ring<4>:pairs=1"),
    _f("right", 5, 64, 4096, "right_mfma", "ring<8>:pairs=1"),
    _f("right", 0, 512, ("pairs", 2), "right_mfma", "ring<2>:pairs=2", "ring:prep<0>:pairs>=2"),
    _f("right", 3, 128, ("pairs", 2), "right_mfma", "ring<4>:pairs=2", "ring:prep<3>:pairs>=2"),
    _f("right", 4, 128, ("pairs", 2), "right_mfma", "ring<8>:pairs=2", "ring:prep<4>:pairs>=2"),
    _f("right", 5, 16, ("pairs", 2), "right_mfma", "ring<2>:pairs=2", "ring:prep<5>:pairs>=2"),
    _f("right", 6, 16, ("pairs", 2), "right_mfma", "ring<4>:pairs=2", "ring:prep<6>:pairs>=2"),
    _f("right", 7, 16, ("pairs", 2), "right_mfma", "ring<8>:pairs=2", "ring:prep<7>:pairs>=2"),
    _f("right", 0, 512, ("pairs", 4), "right_mfma", "ring<2>:pairs=4", "ring:prep<0>:pairs>=2"),
    _f("right", 0, 1024, ("pairs", 4), "right_mfma", "ring<4>:pairs=4", "ring:prep<0>:pairs>=2"),
    _f("right", 0, 2048, ("pairs", 4), "right_mfma", "ring<8>:pairs=4", "ring:prep<0>:pairs>=2"),
    # ---- k_linmap_ring_left<R> (B32 entries only)
    _f("left", 5, 16, 4096, "left_mfma", "ring_left<2>:pairs=1"),
    _f("left", 5, 32, 4096, "left_mfma", "ring_left<4>:pairs=1"),
    _f("left", 5, 64, 4096, "left_mfma", "ring_left<8>:pairs=1"),
    _f("left", 5, 16, ("pairs", 2), "left_mfma", "ring_left<2>:pairs=2"),
    _f("left", 5, 32, ("pairs", 2), "left_mfma", "ring_left<4>:pairs=2"),
    _f("left", 5, 64, ("pairs", 2), "left_mfma", "ring_left<8>:pairs=2"),
    _f("left", 5, 16, ("pairs", 4), "left_mfma", "ring_left<2>:pairs=4"),
    _f("left", 5, 32, ("pairs", 4), "left_mfma", "ring_left<4>:pairs=4"),
    _f("left", 5, 64, ("pairs", 4), "left_mfma", "ring_left<8>:pairs=4"),
    # ---- fold_left with few outputs under a long vector: the partial-evaluation kernel answers
    _f("left", 0, 4096, 1024, "left_pe", "left:pe-routed"),
    _f("left", 5, 4096, 4, "left_pe", "left:pe-routed"),
]
FOLD_BY_ID = {c.id: c for c in FOLD_CASES}
assert len(FOLD_BY_ID) == len(FOLD_CASES)

# every branch that the cases are there for (tests/test_oracle_fold_cases.py: each is claimed by a case)
FOLD_REQUIRED_TAGS = (
    ["tab:wide@3", "tab:wide@4", "tab:wide@5", "tab:narrow-right", "tab:left", "tab:chunks>=2@3", "tab:chunks>=2@4", "tab:chunks>=2@5", "tab:vec1",
     "tab:partial-group", "tab:blocks>=2", "scalar:stride", "scalar:out1", "scalar:vec1", "left:pe-routed"]
    + ["scalar@%d" % l for l in LEVELS]
    + ["%s<%d>:pairs=%d" % (k, R, p) for k in ("ring", "ring_left") for R in (2, 4, 8) for p in (1, 2, 4)]
    + ["ring:prep<%d>:pairs>=2" % l for l in LEVELS]
)


def _pow2_at_least(n):
    return 1 << max(n - 1, 0).bit_length()


def out_len(c, n_cu=NOMINAL_CU):
    """The outputs of fold case `c` on a device with n_cu compute units (the launchers' own formulas: a grid of at most 2 n_cu workgroups
    of 64 outputs a pair; at most 8 n_cu workgroups of 256 threads)."""
    if isinstance(c.out, int):
        return c.out
    rule, k = c.out
    if rule == "pairs":
        n = _pow2_at_least((k - 1) * 64 * 2 * n_cu + 1)  # (more pairs than k - 1 rounds of the grid take)
        assert n >= MFMA_MIN_OUT and ring_pairs(n, n_cu) >= k and ring_pairs(n // 2, n_cu) < k
        return n
    assert rule == "stride"
    n = _pow2_at_least((k - 1) * 256 * 8 * n_cu + 1)
    assert scalar_outputs_per_thread(n, n_cu) >= k and scalar_outputs_per_thread(n // 2, n_cu) < k
    return n


def mat_len(c, n_cu=NOMINAL_CU):
    """128-bit elements of the packed matrix"""
    bits = (c.vec_len * out_len(c, n_cu)) << c.level
    assert bits % 128 == 0, c.id
    return bits // 128


# ---------------------------------------------------------------------------------------------- the inner-product cases
IpCase = namedtuple("IpCase", "id level b route tags")


def _i(level, b, route, *tags):
    return IpCase("ip-l%d-%s" % (level, b if isinstance(b, int) else "%s%d" % b), level, b, route, frozenset(("ip:%s@%d" % (route, level),) + tags))


IP_CASES = [
    # ---- lengths that are no power of two, every level (F x F with an even length is a split sum)
    _i(0, 3 << 9, "scalar", "ip:not-pow2@0"),
    _i(3, 3 << 9, "scalar", "ip:not-pow2@3"),
    _i(4, 3 << 9, "scalar", "ip:not-pow2@4"),
    _i(5, 3 << 9, "scalar", "ip:not-pow2@5"),
    _i(6, 3 << 9, "scalar", "ip:not-pow2@6"),
    _i(7, 3 << 9, "split9", "ip:not-pow2@7"),
    # ---- B32 x F around the bit-sliced kernel's conditions (8192 elements and more, a multiple of 512)
    _i(5, 7680, "scalar", "ip:not-pow2@5", "ip5:below-8192"),
    _i(5, 8192, "ip32", "ip32:at-threshold"),
    _i(5, 8448, "scalar", "ip:not-pow2@5", "ip5:not-512"),
    _i(5, 8704, "ip32", "ip:not-pow2@5", "ip32:ragged"),
    # ---- F x F: odd lengths go to the scalar kernel, two elements are one point per half, the threshold of the matrix cores
    _i(7, 1, "scalar", "ip7:odd", "ip7:len1"),
    _i(7, 2, "split9", "ip7:len2"),
    _i(7, 3, "scalar", "ip:not-pow2@7", "ip7:odd", "ip7:len3"),
    _i(7, (1 << 10) + 1, "scalar", "ip:not-pow2@7", "ip7:odd"),
    _i(7, ("mfma", 0), "split9", "ip:not-pow2@7", "ip7:last-on-9-lane"),
    _i(7, ("mfma", 1), "mfma_split", "ip:not-pow2@7", "ip7:first-on-matrix-cores"),
]
IP_BY_ID = {c.id: c for c in IP_CASES}
assert len(IP_BY_ID) == len(IP_CASES)

IP_REQUIRED_TAGS = (
    ["ip:not-pow2@%d" % l for l in LEVELS] + ["ip:scalar@%d" % l for l in LEVELS]
    + ["ip:split9@7", "ip:mfma_split@7", "ip:ip32@5", "ip5:below-8192", "ip32:at-threshold", "ip5:not-512", "ip32:ragged", "ip7:odd", "ip7:len1", "ip7:len2",
       "ip7:len3", "ip7:last-on-9-lane", "ip7:first-on-matrix-cores"]
)


def ip_len(c, n_cu=NOMINAL_CU):
    """b_len of inner-product case `c`: ("mfma", 0) is the longest even length whose halves have fewer tiles of 256 points than the device has
    compute units, ("mfma", 1) two elements more."""
    if isinstance(c.b, int):
        return c.b
    rule, side = c.b
    assert rule == "mfma" and side in (0, 1)
    half = K_TP * (n_cu - 1) + side
    assert mfma_applies(n_cu, half) == bool(side) and mfma_applies(n_cu, half + 1) and not mfma_applies(n_cu, half - 1)
    return 2 * half


def ip_counters(c, n_cu):
    d = {k: 0 for k in IP_ROUTES}
    d[ip_route(c.level, ip_len(c, n_cu), n_cu)] = 1
    return d


# ---------------------------------------------------------------------------------------------- inputs and references
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def _seed(c):
    table = FOLD_CASES if isinstance(c, FoldCase) else IP_CASES
    return (0xF01D0000 if isinstance(c, FoldCase) else 0x1A9E0000) + 16 * table.index(c)


def fold_inputs(oracle, c, n_cu=NOMINAL_CU):
    """(matrix, vector) of a fold case: SplitMix64 streams of the case's own seeds (not kept: the largest matrix is 32 MiB)."""
    return oracle.random_b128(_seed(c), mat_len(c, n_cu)), oracle.random_b128(_seed(c) + 1, c.vec_len)


def fold_reference(oracle, c, n_cu=NOMINAL_CU):
    """oracle.fold_left / fold_right of the case's inputs: computed once per process, handed out read-only."""
    key = ("fold", c.id, n_cu)
    if key not in _cache:
        mat, vec = fold_inputs(oracle, c, n_cu)
        out = oracle.arr(out_len(c, n_cu))
        assert (oracle.fold_left if c.op == "left" else oracle.fold_right)(mat, c.level, vec, out) == 0
        _cache[key] = _frozen(np.ascontiguousarray(out))
    return _cache[key]


def ip_inputs(oracle, c, n_cu=NOMINAL_CU):
    n_b = ip_len(c, n_cu)
    return oracle.random_b128(_seed(c), n_b >> (7 - c.level)), oracle.random_b128(_seed(c) + 1, n_b)


def ip_reference(oracle, c, n_cu=NOMINAL_CU):
    key = ("ip", c.id, n_cu)
    if key not in _cache:
        a, b = ip_inputs(oracle, c, n_cu)
        rc, want = oracle.inner_product(a, c.level, b)
        assert rc == 0
        _cache[key] = want
    return _cache[key]


def one_hot(vec_len):
    """(vector, j): the field's 1 at one place j of the vector, zero elsewhere"""
    v = np.zeros((vec_len, 2), dtype=np.uint64)
    j = (5 * vec_len) // 8 + 1
    v[j, 0] = 1
    return v, j


def one_hot_expected(mat, level, c, j, n_out):
    """The fold of `mat` with one_hot's vector, without the oracle: entry j of every row (fold_right) or row j (fold_left) of the matrix, every
    packed level-`level` value as the field element it embeds into (its low bits)."""
    mat = np.ascontiguousarray(mat)
    assert (mat.shape[0] * 128) >> level == c.vec_len * n_out
    i = np.arange(n_out, dtype=np.int64)
    idx = j * n_out + i if c.op == "left" else i * c.vec_len + j
    if level == 7:
        return np.ascontiguousarray(mat[idx])
    raw = mat.view(np.uint8).reshape(-1)
    if level == 0:
        vals = (raw[idx >> 3] >> (idx & 7).astype(np.uint8)) & np.uint8(1)
    else:
        vals = raw.view({3: np.uint8, 4: np.uint16, 5: np.uint32, 6: np.uint64}[level])[idx]
    out = np.zeros((n_out, 2), dtype=np.uint64)
    out[:, 0] = vals
    return out
