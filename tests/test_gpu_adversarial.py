"""GPU parity on adversarial operands: patterned data, bases that are odd multiples of 16 bytes, edge scalars, and f32 counts at
the exactness bound of the FP4 Gram kernels.  Every other GPU module feeds the kernels SplitMix64 data in allocator-aligned
arrays with random scalars; a bilinear map that is wrong shows there.  What cannot show there are failures that depend on WHICH
values or addresses arrive, and the hot path is not data-oblivious integer code: sums of GF(2^128) products are counted in the
f32 accumulators of v_mfma_scale_f32_32x32x64_f8f6f4, data nibbles are read as E2M1 codes with bit 3 (the format's sign bit) on a
detour through separate words, and the launchers carry an exactness bound of 2^14 tiles per workgroup.

Everything is compared with the oracle bit for bit.  Helpers: tests/adversarial.py (operand kinds, framed placement); the oracle
functions used at these sizes are pinned on the same operand kinds and scalars by tests/test_oracle_adversarial.py.

Sections: (a) ops x operand kinds at matrix-core sizes, aligned (lead 0) but framed; (b) ops x odd placement (leads 1, 3, 5:
array i of a call sits at (lead + 2 i) mod 16 elements modulo 256 bytes, so no two of a call's first eight arrays share their
offset modulo 256 bytes) on random and dense data; (c) edge scalars; (d) counts at the exactness bound, in a fresh process.
After each op: canaries in front of and behind every array intact, read-only inputs unchanged, outputs equal to the oracle's.

Dispatch conditions (256 CUs): a round evaluation of >= 2^20 points runs k_roundeval_fp4_ws when it has whole tiles and
>= 2 tiles per CU (else k_roundeval_fp4, e.g. ragged lengths); 2^17 .. 2^20 points run the int8 k_roundeval_mfma; a deferred
fold fused with the next evaluation runs k_foldeval_mfma_fp4 from 2^19 elements per array (>= 512 tiles of 256 points, a point
being four input elements), the int8 k_foldeval_mfma below that down to 2^17 points, then the 9-lane and two-round kernels and
the host tail; a prover with several claims runs the group kernel (kernels_group.hip); fold_right with rows of 2048 bits and
>= 4096 outputs, and fold_left at level 5 with 64 columns, run the linear-map kernels (kernels_linmap.hip); products of two full
columns in compute_composite / pairwise_product_reduce run the bit-sliced kernels_mul9.hip / kernels_pairtree.hip."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adversarial as A
import univariate_skip_ref as R
from test_gpu_group import _threads, claim_sums, oracle_single

pytestmark = pytest.mark.gpu

LEADS = (1, 3, 5)
PLACED_KINDS = ("random", "dense")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REF = {}   # oracle results, shared by the parametrised cases that use the same inputs
_DATA = {}  # the large inputs of the placement cases (random and dense only)


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, (1 << 24) + (1 << 21))
    yield ctx
    ctx.close()
    _REF.clear()
    _DATA.clear()


def ref(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def data(kind, seed, n, both=True):
    """The operand pair (or single operand) of a case; kept across the leads for the kinds of section (b)."""
    make = (lambda: A.pair(kind, seed, n)) if both else (lambda: A.operands(kind, seed, n))
    if kind not in PLACED_KINDS:
        return make()
    key = (kind, seed, n, both)
    if key not in _DATA:
        _DATA[key] = make()
    return _DATA[key]


class Stage:
    """The arrays of one call, placed one after the other: lead 0 = every base a multiple of 256 bytes, an odd lead L = array i at
    (L + 2 i) mod 16 elements modulo 256 bytes."""

    def __init__(self, hal, lead):
        self.hal, self.alloc, self.lead, self.i, self.inputs, self.frames = hal, hal.dev_alloc(), lead, 0, [], []

    def _next(self):
        lead = 0 if self.lead == 0 else (self.lead + 2 * self.i) % 16
        self.i += 1
        return lead

    def put(self, arr):
        s, chk = A.place(self.hal, self.alloc, np.ascontiguousarray(arr), self._next())
        self.inputs.append(chk)
        return s

    def out(self, n):
        """(slice, check): the caller calls check(expected)."""
        return A.place(self.hal, self.alloc, int(n), self._next())

    def scratch(self, n):
        s, chk = A.place(self.hal, self.alloc, int(n), self._next())
        self.frames.append(chk)
        return s

    def verify(self):
        for chk in self.inputs:
            chk()
        for chk in self.frames:
            chk(body=False)


def xor_sum(p):
    return int(np.bitwise_xor.reduce(p[:, 0])) | (int(np.bitwise_xor.reduce(p[:, 1])) << 64)


def fast_ip(oracle, a, b):
    got = oracle.fast_inner_product(np.ascontiguousarray(a), np.ascontiguousarray(b), _threads())
    if got is None:  # a host without PCLMULQDQ: the scalar oracle
        rc, got = oracle.inner_product(np.ascontiguousarray(a), 7, np.ascontiguousarray(b))
        assert rc == 0
    return got


# ================================================================== the ops, each as (kind, lead) -> assertions
IP_LEN7 = (1 << 21, 2 * ((1 << 20) + 777), 2 * (131072 + 777))
IP_LEN_SUB = (1 << 20, 1000448)


def op_inner_product(hal, oracle, kind, lead):
    """Level 7: 2^20 points per half (k_roundeval_fp4_ws, split form), 2^20 + 777 (k_roundeval_fp4: the ragged last tile),
    2^17 + 777 (int8 k_roundeval_mfma).  Levels 0, 3, 5 (bit / byte / B32 columns against F: kernels_stream / kernels_ip32): 2^20
    and 1000448 = 512 * 1954 values."""
    a, b = data(kind, 0xA100, max(IP_LEN7))
    st = Stage(hal, lead)
    da, db = st.put(a), st.put(b)
    for n_b in IP_LEN7:
        got = hal.inner_product(da.slice(0, n_b), 7, db.slice(0, n_b))
        assert got == ref(("ip", kind, 7, n_b), lambda: fast_ip(oracle, a[:n_b], b[:n_b])), (kind, lead, n_b)
        g = hal.fp4_last_grids()
        if n_b == IP_LEN7[0]:
            assert g["re_ws"] == 1 and g["re_grid"] * g["re_tiles"] >= (n_b // 2) // 256, g
        elif n_b == IP_LEN7[1]:
            assert g["re_ws"] == 0 and g["re_grid"] * g["re_tiles"] >= (n_b // 2 + 255) // 256, g
    for level in (0, 3, 5):
        for n_b in IP_LEN_SUB:
            n_a = n_b >> (7 - level)
            got = hal.inner_product(da.slice(0, n_a), level, db.slice(0, n_b))
            want = ref(("ip", kind, level, n_b), lambda: fast_ip(oracle, A.unpack_subfield(a[:n_a], level), b[:n_b]))
            assert got == want, (kind, lead, level, n_b)
    if kind == "zero":
        assert got == 0
    st.verify()


def challenges_for(oracle, n_vars, seed=0xC4A1):
    stream = oracle.random_scalars(seed + n_vars, n_vars + 1)
    return stream[0], stream[1:]


def op_sumcheck(hal, oracle, kind, lead, sizes=(20, 22), challenge_sets=None):
    """SumcheckPlan (one claim) at n = 20 and 22 from ONE upload (the n = 20 instance is the first 2^20 elements).  n = 22: round 0
    on k_roundeval_fp4_ws (2^21 points), rounds 1 .. 4 fused on k_foldeval_mfma_fp4 (2^22 .. 2^19 elements), n = 20: rounds 1, 2;
    then int8 k_foldeval_mfma, the 9-lane rounds, the two-round launches (armed) and the host tail."""
    from binius_amd._host import SumcheckPlan

    n_max = max(sizes)
    mls = data(kind, 0xA200, 1 << n_max)
    st = Stage(hal, lead)
    d = [st.put(x) for x in mls]
    scratch = st.scratch(2 << (n_max - 1))
    for n in sizes:
        sub = [x[: 1 << n] for x in mls]
        dn = [s.slice(0, 1 << n) for s in d]
        claim = ref(("claim", kind, n), lambda: fast_ip(oracle, sub[0], sub[1]))
        assert hal.inner_product(dn[0], 7, dn[1]) == claim, (kind, lead, n)
        for name, (bc, ch) in (challenge_sets or {"random": challenges_for(oracle, n)}).items():
            want = ref(("sumcheck", kind, n, name), lambda: oracle_single(oracle, sub, n, [(0, 1)], [claim], bc, ch))
            plan = SumcheckPlan(hal, n, dn, scratch.slice(0, 2 << (n - 1)), [(0, 1)], [claim], bc, ch)
            c0 = hal.arm_counters()
            plan.run()
            c1 = hal.arm_counters()
            got = (plan.round_coeffs(), plan.final_evals())
            for r in range(n):
                assert list(got[0][r]) == list(want[0][r]), "round %d differs from the oracle (%s, lead %d, n = %d, challenges %s)" % (r, kind, lead, n, name)
            assert list(got[1]) == list(want[1]), (kind, lead, n, name)
            # the small rounds went through the two-round launches and, where the host can take over, the host tail
            assert c1["two_round"] > c0["two_round"], (c0, c1)
            if c1["ht_max"]:
                assert c1["ht_started"] == c0["ht_started"] + 1, (c0, c1)
            g = hal.fp4_last_grids()
            assert g["fe_grid"] > 0 and g["fe_grid"] * g["fe_tiles"] >= 512, g
            if n >= 21:
                assert g["re_ws"] == 1, g
    st.verify()


BOOL_BITS = 0b0110_1001_1100_0101_1010  # the boolean indicator point of the MLE-check case


def eq_point(oracle, n, boolean):
    if boolean:
        return [(BOOL_BITS >> i) & 1 for i in range(n)]
    return oracle.random_scalars(0xA3E9, n)


def eq_half_table(oracle, n, boolean):
    def make():
        t = oracle.arr(1 << (n - 1))
        t[0] = (1, 0)
        assert oracle.tensor_expand(t, 0, eq_point(oracle, n, boolean)[: n - 1]) == 0
        return t

    return ref(("eq_half", n, boolean), make)


def op_mlecheck(hal, oracle, kind, lead, boolean=False):
    """MlecheckPlan at n = 20.  A point without 0 / 1 coordinates: the weighted prover (the indicator folded into one factor, then
    the matrix-core rounds); a BOOLEAN point (the table is one-hot): the literal prover, three-factor 9-lane kernels."""
    from binius_amd._host import MlecheckPlan

    n = 20
    half = 1 << (n - 1)
    mls = data(kind, 0xA300, 1 << n)
    point = eq_point(oracle, n, boolean)
    eq_half = eq_half_table(oracle, n, boolean)
    top = point[n - 1]

    def claim():  # sum_x eq(x) a(x) b(x), eq = eq_half (x) (1 - top, top)
        ab = oracle.mul_vec(np.ascontiguousarray(mls[0]), np.ascontiguousarray(mls[1]))
        return oracle.mul(fast_ip(oracle, ab[:half], eq_half), 1 ^ top) ^ oracle.mul(fast_ip(oracle, ab[half:], eq_half), top)

    sums = [ref(("mle_claim", kind, boolean), claim)]
    bc, ch = challenges_for(oracle, n, 0xC4A2)
    want = ref(("mlecheck", kind, boolean),
               lambda: oracle.bivariate_mlecheck_prove([x.copy() for x in mls], n, eq_half.copy(), point, [(0, 1)], sums, bc, ch))
    st = Stage(hal, lead)
    d = [st.put(x) for x in mls]
    d_eq = st.put(eq_half)
    scratch = st.scratch(3 * half)
    if lead == 0 and not boolean:  # the device's own expansion of the point is the oracle's table
        tmp, chk = st.out(half)
        hal.fill(tmp.slice(0, 1), 1)
        hal.tensor_expand(0, point[: n - 1], tmp)
        chk(eq_half)
    plan = MlecheckPlan(hal, n, d, d_eq, point, scratch, [(0, 1)], sums, bc, ch)
    plan.run()
    assert plan.last_mode() == (0 if boolean else 1)
    assert plan.round_coeffs() == want[0], (kind, lead, boolean)
    assert plan.final_evals() == want[1], (kind, lead, boolean)
    if kind == "zero":
        assert sums == [0]
    st.verify()


GROUP_COMPS = [(0, 4), (1, 5), (2, 6), (0, 7)]  # k = 4 claims over m = 8, multilinear 0 shared, 3 in no claim
GROUP_KINDS = {
    "mixed1": ("dense", "sparse", "nib8", "nib7", "limb1", "sub3", "zero", "limb2"),
    "mixed2": ("limb0", "limb3", "sub0", "sub5", "same", "dense", "sparse", "nib8"),  # ("same": a copy of multilinear 0)
    "random": ("random",) * 8,
    "dense": ("dense",) * 8,
}


def group_data(which):
    def make():
        out = []
        for j, k in enumerate(GROUP_KINDS[which]):
            out.append(out[0].copy() if k == "same" else A.operands(k, 0xA400 + j, 1 << 20))
        return out

    if which in PLACED_KINDS:
        if ("group", which) not in _DATA:
            _DATA[("group", which)] = make()
        return _DATA[("group", which)]
    return make()


def op_group(hal, oracle, which, lead):
    """One prover with four claims over eight multilinears at n = 20, every multilinear of a different kind: the group kernel's
    fused, evaluate-only and fold-only jobs, then the hosted rounds."""
    from binius_amd._host import SumcheckPlan

    n, m = 20, 8
    mls = group_data(which)
    bc, ch = challenges_for(oracle, n, 0x6A0C)
    sums = ref(("group_sums", which), lambda: claim_sums(oracle, mls, GROUP_COMPS))
    want = ref(("group", which), lambda: oracle_single(oracle, mls, n, GROUP_COMPS, sums, bc, ch))
    st = Stage(hal, lead)
    d = [st.put(x) for x in mls]
    scratch = st.scratch(m << (n - 1))
    c0 = hal.group_counters()
    plan = SumcheckPlan(hal, n, d, scratch, GROUP_COMPS, sums, bc, ch)
    plan.run()
    c1 = hal.group_counters()
    assert plan.round_coeffs() == want[0], (which, lead)
    assert plan.final_evals() == want[1], (which, lead)
    assert c1["evals"] - c0["evals"] == n and c1["launches"] > c0["launches"], (c0, c1)
    st.verify()


def mixed_columns(n, seed):
    """Two columns of n = 16 segments: segment s holds operand kind s (13 kinds, then random): element-wise ops see every kind,
    against its partner of pair(), in one launch."""
    seg = n // 16
    kinds = list(A.KINDS) + ["random"] * 3

    def make():
        parts = [A.pair(k, seed + 2 * s, seg) for s, k in enumerate(kinds)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    if ("mixed", n, seed) not in _DATA:
        _DATA[("mixed", n, seed)] = make()
    return _DATA[("mixed", n, seed)]


def op_compute_composite(hal, oracle, kind, lead):
    """a * b over 2^20 elements (kernels_mul9.hip, the two-batch kernel) and over the ragged 500001."""
    a, b = mixed_columns(1 << 20, 0xA500) if kind == "mixed" else data(kind, 0xA500, 1 << 20)
    expr = hal.compile_expr([("var", 0), ("var", 1), ("mul", 0, 1)])
    try:
        for n in (1 << 20, 500001):
            st = Stage(hal, lead)
            da, db = st.put(a[:n]), st.put(b[:n])
            do, chk = st.out(n)
            hal.compute_composite([da, db], do, expr)
            chk(ref(("mul", kind, 1 << 20), lambda: oracle.mul_vec(np.ascontiguousarray(a), np.ascontiguousarray(b)))[:n])
            st.verify()
    finally:
        expr.free()


def op_pairwise(hal, oracle, kind, lead):
    """pairwise_product_reduce of 2^20 elements: twenty rounds of outputs, each framed."""
    x = mixed_columns(1 << 20, 0xA600)[0] if kind == "mixed" else data(kind, 0xA600, 1 << 20, both=False)
    n, log = 1 << 20, 20

    def want():
        exp = [oracle.arr(n >> (r + 1)) for r in range(log)]
        assert oracle.pairwise_product_reduce(np.ascontiguousarray(x), exp) == 0
        return exp

    exp = ref(("pairwise", kind), want)
    st = Stage(hal, lead)
    dx = st.put(x)
    outs = [st.out(n >> (r + 1)) for r in range(log)]
    hal.pairwise_product_reduce(dx, [o for o, _ in outs])
    for (_, chk), e in zip(outs, exp):
        chk(e)
    st.verify()


FOLD_SHAPES = [(True, 5, 64)] + [(False, level, 2048 >> level) for level in (0, 3, 5)]  # (left, level, vector length): 2048-bit rows


def op_folds(hal, oracle, mat_kind, vec_kind, lead, vec=None):
    """fold_right with rows of 2048 bits at levels 0, 3, 5 and fold_left at level 5 with 64 columns, 4096 outputs: the linear map
    on the matrix cores (kernels_linmap.hip), whose table is built from the vector."""
    out_len = 4096
    for left, level, vec_len in FOLD_SHAPES:
        mat = A.operands(mat_kind, 0xA700 + level, (out_len * vec_len) >> (7 - level))
        v = A.operands(vec_kind, 0xA710 + level, vec_len) if vec is None else vec(vec_len)
        exp = oracle.arr(out_len)
        assert (oracle.fold_left if left else oracle.fold_right)(mat, level, v, exp) == 0
        st = Stage(hal, lead)
        dm, dv = st.put(mat), st.put(v)
        do, chk = st.out(out_len)
        (hal.fold_left if left else hal.fold_right)(dm, level, dv, do)
        chk(exp)
        st.verify()


AB_PLUS_C = [("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("add", 2, 3)]
AB = [("var", 0), ("var", 1), ("mul", 0, 1)]


def op_hal_round_evals(hal, oracle, kind, lead):
    """(a * b + c) * eq at n = 20, High-to-Low, evaluation points 1 and infinity (leading form a * b): the general bit-sliced kernel
    of abi_hal.cpp on 2^19 vertices."""
    n = 20
    a, b = data(kind, 0xA800, 1 << n)
    c = data(kind, 0xA802, 1 << n, both=False)
    eq = eq_half_table(oracle, n, False)
    ev = [{"steps": AB_PLUS_C, "steps_inf": AB, "start": 1, "end": 3, "eq_ind": eq}]

    def want():
        rc, w = oracle.hal_round_evals(1, n, None, [("folded", np.ascontiguousarray(v), 0) for v in (a, b, c)], ev, [])
        assert rc == 0
        return w

    st = Stage(hal, lead)
    d = [st.put(v) for v in (a, b, c)]
    d_eq = st.put(eq)
    e1, e2 = hal.compile_expr(AB_PLUS_C), hal.compile_expr(AB)
    try:
        got = hal.hal_round_evals(1, n, None, [("folded", s, 0) for s in d],
                                  [{"composition": e1, "composition_at_infinity": e2, "start": 1, "end": 3, "eq_ind": d_eq}], [])
    finally:
        e1.free()
        e2.free()
    assert got == ref(("hal_round_evals", kind), want), (kind, lead)
    st.verify()


# ---- the ops of section (b) only
def op_extrapolate(hal, oracle, kind, lead):
    """extrapolate_line_batch: two pairs of (1 << 17) + 77 elements, flushed by the read-back (the stream kernel)."""
    n = (1 << 17) + 77
    z = oracle.random_scalars(0xA900, 1)[0]
    x = [A.operands(kind, 0xA900 + j, n) for j in range(4)]
    st = Stage(hal, lead)
    outs = []
    for j in range(4):  # evals_0 are outputs (folded in place), evals_1 inputs
        if j < 2:
            s, chk = st.out(n)
            hal.copy_h2d(x[j], s)
            outs.append((s, chk))
        else:
            outs.append((st.put(x[j]), None))
    hal.extrapolate_line_batch([outs[0][0], outs[1][0]], [outs[2][0], outs[3][0]], z)
    for j in range(2):
        exp = x[j].copy()
        assert oracle.extrapolate_line(exp, x[2 + j], z) == 0
        outs[j][1](exp)
    st.verify()


def op_tensor_expand(hal, oracle, kind, lead, coords=None):
    """tensor_expand of 2^4 given values by 12 coordinates (2^16 outputs)."""
    log_n, coords = 4, coords if coords is not None else oracle.random_scalars(0xAA00, 12)
    n = 1 << (log_n + len(coords))
    head = A.operands(kind, 0xAA01, 1 << log_n)
    exp = oracle.arr(n)
    exp[: 1 << log_n] = head
    assert oracle.tensor_expand(exp, log_n, coords) == 0
    st = Stage(hal, lead)
    s, chk = st.out(n)
    hal.copy_h2d(head, s.slice(0, 1 << log_n))
    hal.tensor_expand(log_n, coords, s)
    chk(exp)
    return exp


def op_fri_fold(hal, oracle, kind, lead, challenges=None):
    import binius_amd

    log_len, log_batch, n_fold, tw_level = 16, 2, 2, 5
    log_domain = log_len + 1
    s_ev = binius_amd.ntt_s_evals(tw_level, log_domain)
    assert np.array_equal(s_ev, oracle.ntt_s_evals(tw_level, log_domain))
    x = data(kind, 0xAB00, 1 << (log_len + log_batch), both=False)
    ch = challenges if challenges is not None else oracle.random_scalars(0xAB01, log_batch + n_fold)
    out_len = 1 << (log_len - n_fold)

    def want():
        exp = oracle.arr(out_len)
        assert oracle.fri_fold(s_ev, tw_level, log_domain, log_len, log_batch, ch, np.ascontiguousarray(x), exp) == 0
        return exp

    st = Stage(hal, lead)
    din = st.put(x)
    dout, chk = st.out(out_len)
    hal.fri_fold(s_ev, tw_level, log_domain, log_len, log_batch, ch, din, dout)
    chk(ref(("fri", kind, tuple(ch)), want))
    st.verify()


def op_ntt(hal, oracle, kind, lead):
    """Forward and inverse additive NTT of 2^16 B32 and 2^16 B128 values in place, the data `lead` elements into its block."""
    import binius_amd

    log_y, tw = 16, 5
    s_ev = binius_amd.ntt_s_evals(tw, log_y + 1)
    for elem_level in (5, 7):
        n_el = (1 << log_y) >> (7 - elem_level)
        x = A.operands(kind, 0xAC00 + elem_level, n_el)

        def want():
            e = x.copy()
            assert oracle.ntt_forward(e, elem_level, tw, s_ev, log_y + 1, 0, log_y, 0) == 0
            return e

        st = Stage(hal, lead)
        s, chk = st.out(n_el)
        hal.copy_h2d(x, s)
        hal.ntt_forward(s.ptr, elem_level, tw, s_ev, log_y + 1, 0, log_y, 0)
        chk(ref(("ntt", kind, elem_level), want))
        hal.ntt_inverse(s.ptr, elem_level, tw, s_ev, log_y + 1, 0, log_y, 0)
        chk(x)


def op_merkle(hal, oracle, kind, lead):
    """merkle_build of 2^13 leaves of 4 elements (leaves and node array placed) and groestl256_leaves of the same leaves."""
    n_leaves, batch = 1 << 13, 4
    x = data(kind, 0xAD00, n_leaves * batch, both=False)

    def want():
        rc, nodes = oracle.merkle_build(np.ascontiguousarray(x), batch)
        assert rc == 0
        return np.ascontiguousarray(nodes).view(np.uint64).reshape(-1, 2)

    exp = ref(("merkle", kind), want)
    st = Stage(hal, lead)
    dx = st.put(x)
    nodes, chk_nodes = st.out(2 * (2 * n_leaves - 1))
    leaves, chk_leaves = st.out(2 * n_leaves)
    hal.merkle_build(dx, batch, nodes)
    chk_nodes(exp)
    hal.groestl256_leaves(dx, batch, leaves)
    chk_leaves(exp[: 2 * n_leaves])
    st.verify()


def op_univariate(hal, oracle, kind, lead):
    """zerocheck_univariate_evals, k = 7, n = 13, one-bit and B8 columns: columns and the indicator table placed."""
    from test_gpu_univariate_skip import comp_set

    n_vars, k = 13, 7
    comps, degrees = comp_set(2)
    D = max(degrees) << k
    ch = oracle.random_scalars(0xAE00, n_vars - k)
    for level in (0, 3):
        rng = np.random.default_rng(0xAE + level)
        if kind == "dense":  # columns of ones with a few zeros (bytes: 0xFF with one bit cleared)
            vals = [(1 - (rng.integers(0, 64, 1 << n_vars) == 0)).astype(np.uint8) if level == 0
                    else (0xFF ^ (1 << rng.integers(0, 8, 1 << n_vars))).astype(np.uint8) for _ in range(5)]
        else:
            vals = [rng.integers(0, 2 if level == 0 else 256, 1 << n_vars, dtype=np.uint8) for _ in range(5)]
        want = ref(("univariate", kind, level), lambda: R.univariate_evals([(v, level) for v in vals], n_vars, k, comps, degrees, ch, D))
        st = Stage(hal, lead)
        cols = [(st.put(R.pack(v, level)), level) for v in vals]
        d_eq = st.put(oracle.ints_to_arr(R.eq_expansion(ch)))
        assert hal.zerocheck_univariate_evals(n_vars, k, cols, comps, degrees, d_eq, D) == want, (kind, lead, level)
        st.verify()


# ================================================================== (a) ops x operand kinds, aligned
@pytest.mark.parametrize("kind", A.KINDS)
def test_inner_product_on_operand_kinds(hal, oracle, kind):
    op_inner_product(hal, oracle, kind, 0)


@pytest.mark.parametrize("kind", A.KINDS)
def test_sumcheck_plan_on_operand_kinds(hal, oracle, kind):
    op_sumcheck(hal, oracle, kind, 0)


@pytest.mark.parametrize("kind", A.KINDS)
def test_mlecheck_plan_on_operand_kinds(hal, oracle, kind):
    op_mlecheck(hal, oracle, kind, 0)


def test_mlecheck_plan_with_a_boolean_indicator_point(hal, oracle):
    op_mlecheck(hal, oracle, "random", 0, boolean=True)


@pytest.mark.parametrize("which", ["mixed1", "mixed2"])
def test_claim_group_with_a_different_kind_per_multilinear(hal, oracle, which):
    op_group(hal, oracle, which, 0)


def test_bit_sliced_products_on_every_operand_kind(hal, oracle):
    """compute_composite a * b and pairwise_product_reduce are element-wise: one column pair of sixteen segments holds every kind."""
    op_compute_composite(hal, oracle, "mixed", 0)
    op_pairwise(hal, oracle, "mixed", 0)


@pytest.mark.parametrize("mat_kind", ["dense", "sparse"])
@pytest.mark.parametrize("vec_kind", ["dense", "sparse"])
def test_linear_map_folds_with_dense_and_sparse_operands(hal, oracle, mat_kind, vec_kind):
    op_folds(hal, oracle, mat_kind, vec_kind, 0)


@pytest.mark.parametrize("kind", A.KINDS)
def test_hal_round_evals_on_operand_kinds(hal, oracle, kind):
    op_hal_round_evals(hal, oracle, kind, 0)


# ================================================================== (b) ops x odd placement
@pytest.mark.parametrize("kind", PLACED_KINDS)
@pytest.mark.parametrize("lead", LEADS)
def test_matrix_core_ops_at_odd_bases(hal, oracle, kind, lead):
    op_inner_product(hal, oracle, kind, lead)
    op_sumcheck(hal, oracle, kind, lead)
    op_mlecheck(hal, oracle, kind, lead)
    op_group(hal, oracle, kind, lead)
    op_hal_round_evals(hal, oracle, kind, lead)


@pytest.mark.parametrize("lead", LEADS)
def test_bit_sliced_products_at_odd_bases(hal, oracle, lead):
    """(the mixed columns hold random and dense segments)"""
    op_compute_composite(hal, oracle, "mixed", lead)
    op_pairwise(hal, oracle, "mixed", lead)


@pytest.mark.parametrize("kind", PLACED_KINDS)
@pytest.mark.parametrize("lead", LEADS)
def test_layer_ops_at_odd_bases(hal, oracle, kind, lead):
    op_folds(hal, oracle, kind, kind, lead)
    op_extrapolate(hal, oracle, kind, lead)
    op_tensor_expand(hal, oracle, kind, lead)
    op_fri_fold(hal, oracle, kind, lead)
    op_ntt(hal, oracle, kind, lead)
    op_merkle(hal, oracle, kind, lead)
    op_univariate(hal, oracle, kind, lead)


# ================================================================== (c) edge scalars
def test_sumcheck_plan_with_edge_challenges(hal, oracle):
    """n = 22, every round's challenge equal to z for each edge scalar, and once a vector that cycles through them, so that each value
    meets the fused FP4 rounds (the LDS nibble tables are built from z), the armed two-round launches (z arrives through the command
    block) and the host tail (z multiplies in the host's basis).  z = 0 keeps the lower halves, z = 1 the upper halves."""
    n = 22
    bc = oracle.random_scalars(0xAF00, 1)[0]
    sets = {"all %#x" % z: (bc, [z] * n) for z in A.EDGE_SCALARS}
    sets["cycle"] = (bc, [A.EDGE_SCALARS[(r + 3) % len(A.EDGE_SCALARS)] for r in range(n)])
    op_sumcheck(hal, oracle, "random", 0, sizes=(n,), challenge_sets=sets)
    mls = data("random", 0xA200, 1 << n)
    assert _REF[("sumcheck", "random", n, "all 0x0")][1] == oracle.arr_to_ints(np.stack([mls[0][0], mls[1][0]]))
    assert _REF[("sumcheck", "random", n, "all 0x1")][1] == oracle.arr_to_ints(np.stack([mls[0][-1], mls[1][-1]]))


@pytest.mark.parametrize("bc", [0, 1, A.ALL_ONES])
def test_two_claim_prover_with_edge_batching_coefficients(hal, oracle, bc):
    """Two claims over three multilinears at n = 20 (the group kernel; finalize.hpp branches on a coefficient of 1): batched with 0
    (the second claim vanishes from every round polynomial), 1 and all ones."""
    from binius_amd._host import SumcheckPlan

    n, comps = 20, [(0, 1), (2, 1)]
    mls = [data("random", 0xB000 + j, 1 << n, both=False) for j in range(3)]
    ch = oracle.random_scalars(0xB010, n)
    sums = ref(("bc_sums",), lambda: claim_sums(oracle, mls, comps))
    want = oracle_single(oracle, mls, n, comps, sums, bc, ch)
    st = Stage(hal, 0)
    d = [st.put(x) for x in mls]
    scratch = st.scratch(3 << (n - 1))
    plan = SumcheckPlan(hal, n, d, scratch, comps, sums, bc, ch)
    plan.run()
    assert plan.round_coeffs() == want[0] and plan.final_evals() == want[1]
    if bc == 0:
        one = oracle_single(oracle, mls[:2], n, [(0, 1)], sums[:1], 1, ch)
        assert plan.round_coeffs() == one[0]
    st.verify()


@pytest.mark.parametrize("z", [0, 1])
def test_fri_fold_with_constant_challenges(hal, oracle, z):
    op_fri_fold(hal, oracle, "random", 0, challenges=[z] * 4)


def test_tensor_expand_with_boolean_and_zero_coordinates(hal, oracle):
    """A boolean point: the expansion is the given values at one offset and zero elsewhere; a single zero coordinate zeroes the
    half of the table that has its bit set."""
    bits = [1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0, 1]
    exp = op_tensor_expand(hal, oracle, "random", 0, coords=bits)
    at = sum(b << i for i, b in enumerate(bits)) << 4
    assert exp[at : at + 16].all(axis=None) and not exp[:at].any() and not exp[at + 16 :].any()
    coords = oracle.random_scalars(0xB100, 12)
    coords[5] = 0
    exp = op_tensor_expand(hal, oracle, "random", 0, coords=coords)
    idx = np.arange(exp.shape[0])
    assert not exp[((idx >> (4 + 5)) & 1) == 1].any() and exp[((idx >> (4 + 5)) & 1) == 0].any()


def test_linear_map_folds_with_a_one_hot_vector(hal, oracle):
    """fold_right / fold_left with a vector that is 1 in one place: the output is one column / row of the matrix."""

    def one_hot(n):
        v = np.zeros((n, 2), dtype=np.uint64)
        v[(5 * n) // 8 + 1, 0] = 1
        return v

    op_folds(hal, oracle, "random", None, 0, vec=one_hot)


# ================================================================== (d) counts at the exactness bound
BOUND_ENV = {"BN_FP4_WS_GRID": "2", "BN_FE_FP4_GRID": "1"}


def bound_case():
    """The child process of test_counts_at_the_exactness_bound (the grid switches are read once per process)."""
    import binius_amd
    import oracle
    from binius_amd._host import SumcheckPlan

    oracle.build()
    assert all(os.environ.get(k) == v for k, v in BOUND_ENV.items())
    n = 24
    tiles_max = 1 << 14
    a, b = A.pair("dense", 0xD000, 1 << n)
    extra = 2 * ((1 << 23) + 256)  # a split inner product of 2^23 + 256 points per half: 2^15 + 1 tiles
    # (a and b continued by their own first elements: the longer inner product reads past the 2^24)
    full_a, full_b = np.concatenate([a, a[: extra - (1 << n)]]), np.concatenate([b, b[: extra - (1 << n)]])
    with binius_amd.Context(0, 2 * extra + (1 << n) + 8 * A.FRAME) as hal:
        st = Stage(hal, 0)
        da, db = st.put(full_a), st.put(full_b)
        scratch = st.scratch(1 << n)
        # 1. the round evaluation alone (split form, no MIX): two workgroups of 2^14 tiles
        claim = fast_ip(oracle, a, b)
        assert hal.inner_product(da.slice(0, 1 << n), 7, db.slice(0, 1 << n)) == claim
        g = hal.fp4_last_grids()
        assert (g["re_ws"], g["re_grid"], g["re_tiles"]) == (1, 2, tiles_max), g
        # 2. round 0 (MIX: the infinity operands are a_lo ^ a_hi) on two workgroups of 2^14 tiles, then the first fused fold +
        #    evaluation on ONE workgroup of 2^14 tiles; challenge 0 = 1 keeps the folded arrays dense (a' = a_hi)
        bc, ch = challenges_for(oracle, n)
        ch = [1] + list(ch[1:])
        plan = SumcheckPlan(hal, n, [da.slice(0, 1 << n), db.slice(0, 1 << n)], scratch, [(0, 1)], [claim], bc, ch)
        plan.run()
        g = hal.fp4_last_grids()
        assert (g["re_ws"], g["re_grid"], g["re_tiles"]) == (1, 2, tiles_max), g  # (round 0: the last FP4 round evaluation)
        # every fused FP4 launch ran on the one workgroup asked for (the last: 2^19 elements, 512 tiles), and the largest share a
        # workgroup took is 2^14 tiles -- the 2^24-element launch, the only one with that many tiles
        assert (g["fe_grid"], g["fe_tiles"], g["fe_max_tiles"], g["re_max_tiles"]) == (1, 512, tiles_max, tiles_max), g
        want = oracle_single(oracle, [a, b], n, [(0, 1)], [claim], bc, ch)
        got = (plan.round_coeffs(), plan.final_evals())
        for r in range(n):
            assert list(got[0][r]) == list(want[0][r]), "round %d differs from the oracle" % r
        assert list(got[1]) == list(want[1])
        # 3. the other side of the bound: 2^15 + 1 tiles on two workgroups would be 2^14 + 1 each -- the override is dropped, the
        #    launch runs on one workgroup per CU, and the result is still the oracle's
        assert hal.inner_product(da, 7, db) == fast_ip(oracle, full_a, full_b)
        g = hal.fp4_last_grids()
        assert g["re_ws"] == 1 and g["re_grid"] > 2 and g["re_grid"] * g["re_tiles"] >= (1 << 15) + 1, g
        assert g["re_max_tiles"] == tiles_max, g
        st.verify()
    print("bound case ok")


@pytest.mark.last
def test_counts_at_the_exactness_bound():
    """The FP4 Gram kernels keep a sum of GF(2) products as an f32 count and read its parity; their launchers give a workgroup
    at most 2^14 tiles = 2^22 points ("the f32 counts stay exact").  No other test comes within a factor of sixteen of that bound
    (random data: a count is about a quarter of the points; the largest share of a workgroup is 2^20 points at n = 28).

    Here: n = 24, `dense` operands (127 of 128 bits set), BN_FP4_WS_GRID = 2 and BN_FE_FP4_GRID = 1 in a fresh process (the
    switches are read once), so that the claim's inner product and round 0 run k_roundeval_fp4_ws on two workgroups of exactly
    2^14 tiles each, and the first fused fold + evaluation (2^24 elements per array = 2^22 points) runs k_foldeval_mfma_fp4 on ONE
    workgroup of 2^14 tiles; bn_fp4_last_grids confirms the grids ran as asked (an override past the bound is silently dropped).

    The largest count.  An accumulator entry (row bit p of an operand combination U, column bit q of a combination V) is
    sum_j U_j[p] V_j[q] * 2^(e_p + e_q) over the workgroup's points j, the codes being 0.5, 1, 2 (e = -1, 0, 1): one term per
    point, every term the same power of two, so the entry is count * 2^e with count <= 2^22 and -2 <= e <= 2.  An f32 holds
    every integer up to 2^24 and scaling by a power of two is exact, so the entry -- and every partial sum on the way -- is exact
    as long as count <= 2^24: the bound leaves a factor of FOUR, not more.  With `dense` data a plain-limb combination has bit p
    set in all points but the ~2^22 / 128 whose cleared bit is p, so the entries of the plain blocks (limb w of u against limb w'
    of v) reach counts of 2^22 - 2^16 +- a little, with both parities occurring -- 22 significant bits.  The Karatsuba
    combinations (u0 ^ u1, u0 ^ u2, ..., and in round 0's infinity operands a_lo ^ a_hi) are XORs of dense words and therefore
    SPARSE here: their entries stay below 2^22 / 64.  (No data makes every combination dense at once: of x, y, x ^ y at most two
    have a given bit set.)  After the fold with challenge 1 the arrays are the dense upper halves, so the fused kernel's plain
    blocks reach the top as well.  What rounding at the top would do: an accumulator that kept fewer than 22 bits would flip
    parities of exactly these entries, and the transcript would differ from the oracle's.

    The other side: an inner product of 2^15 + 1 tiles per half would be 2^14 + 1 tiles per workgroup on the same two-workgroup
    grid; the launcher drops the override (one workgroup per CU instead) and the result is the oracle's.  A fused launch of more
    than 2^14 tiles on one workgroup needs 2^25 elements per array (the sizes are powers of two), beyond this module's sizes:
    its launcher applies the same test to the override (kernels_foldeval_fp4.hip).  The group kernel has no grid switch; its
    bound (kernels_group.hip) is reached only from n = 31 on 256 CUs."""
    env = dict(os.environ, **BOUND_ENV)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_adversarial as t; t.bound_case()" % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert "bound case ok" in p.stdout, p.stdout[-2000:]
