"""Every entry point sees device memory exactly as eager execution would leave it -- whatever the library has deferred when it is
called.  tests/deferred_states.py reaches the four states on purpose and proves from the counters that
they are reached:

  S1  a fold pending in the single-claim state         S3  a hosted session, nothing pending
  S2  a fold parked as a claim-group fold              S4  a hosted session, the device one write-back behind
                                                       S4x2  S4 after a second fold: the write-back covers more than the arrays

A. The range-scoped entry points (BN_FLUSH_FOR, group_flush_touching), where the hand-written range decides what runs first: state x
   role x placement.  A placement puts the op's range over the whole array, over exactly one element at an isolated boundary of it,
   or exactly beside it (the deferred work must then STAY deferred).
B. The blanket-flush entry points (BN_FLUSH), so that none reads or writes ahead of its flush: each with a live array as an operand.
C. Every bn_* entry point of include/binius_amd.h that takes device memory is in one of the tables or in EXEMPT with a reason (CPU).

Every expected value is the oracle's on the host model; after every case one more execute / fold / execute of the prover must still
give the oracle's round values, and every byte of the case's region must equal the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deferred_states as ds
import fri_verify_ref as fv

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAPPING = ("whole", "first", "last")
ADJACENT = ("adj_before", "adj_after")


def placements(state, kind):
    """whole, and the boundaries of the row that a spare buffer isolates (deferred_states.ISOLATED): a range over "first" / "last"
    touches ONE element of the row and otherwise spare memory only.  (x1 begins where src0 ends: that boundary is not isolated.)"""
    if kind not in ds.ISOLATED[state]:
        return ()
    before, after = ds.ISOLATED[state][kind]
    return ("whole",) + (("first", "adj_before") if before else ()) + (("last", "adj_after") if after else ())


@pytest.fixture(scope="module")
def contexts():
    c = ds.Contexts()
    yield c
    c.close()


def H(buf):
    """the model's copy of a buffer, for an oracle call"""
    return np.ascontiguousarray(buf.host).copy()


def place(pv, st, kind, placement, small):
    """The range of a role: a Buf of `st` (the arrays are where the preview, driven to the state, says they are).  whole: the first
    array of the row; otherwise `small` elements around an isolated boundary of the row."""
    rows, spare_before, spare_after = pv.row(kind)
    first, last = rows[0], rows[-1]
    if placement == "whole":
        return ds.Buf(st, first.off, first.n, kind)
    off = {"first": first.off + 1 - small, "adj_before": first.off - small, "last": last.end - 1, "adj_after": last.end}[placement]
    b = ds.Buf(st, off, small, kind + ":" + placement)
    lo = spare_before.off if placement in ("first", "adj_before") else last.end - 1
    hi = first.off + 1 if placement in ("first", "adj_before") else spare_after.end
    assert lo <= b.off and b.end <= hi, "a placement outside the spare buffer and the one element it may touch"
    return b


def log2(n):
    assert n and n & (n - 1) == 0
    return n.bit_length() - 1


_S_EVALS = {}


def s_evals(oracle, log_domain=10):
    if log_domain not in _S_EVALS:
        _S_EVALS[log_domain] = oracle.ntt_s_evals(5, log_domain)
    return _S_EVALS[log_domain]


def same(hal, out):
    assert np.array_equal(hal.copy_d2h(out.dev), out.host), "%s differs from the oracle's" % out.name


# ------------------------------------------------------------------------------------------------ A: the range-scoped entry points
# A role: fn(oracle, pv, st, placement) -> call; call() issues the entry point on the device, applies the oracle's result to the
# model and returns check(), which compares what the entry point returned or wrote with the model.
def fri_fold_in(kind):
    def role(oracle, pv, st, placement):
        rng = place(pv, st, kind, placement, 16)
        out = st.take(rng.n >> 2, "fri_fold out")
        chs = oracle.random_scalars(0xF01D, 2)

        def call():
            st.hal.fri_fold(s_evals(oracle), 5, 10, log2(rng.n), 0, chs, rng.dev, out.dev)
            o = oracle.arr(out.n)
            assert oracle.fri_fold(s_evals(oracle), 5, 10, log2(rng.n), 0, chs, H(rng), o) == 0
            out.host[:] = o
            return lambda: same(st.hal, out)

        return call

    return role


def fri_fold_out(kind):
    def role(oracle, pv, st, placement):
        rng = place(pv, st, kind, placement, 16)
        src = st.take(4 * rng.n, "fri_fold in")
        chs = oracle.random_scalars(0xF02D, 2)

        def call():
            st.hal.fri_fold(s_evals(oracle), 5, 10, log2(src.n), 0, chs, src.dev, rng.dev)
            o = oracle.arr(rng.n)
            assert oracle.fri_fold(s_evals(oracle), 5, 10, log2(src.n), 0, chs, H(src), o) == 0
            rng.host[:] = o
            return lambda: None  # (the written range is part of the final byte comparison: reading it here would hide a stale continuation)

        return call

    return role


def merkle_elems(oracle, pv, st, placement):
    rng = place(pv, st, "live", placement, 16)
    nodes = st.take(2 * (2 * (rng.n // 4) - 1), "merkle nodes")

    def call():
        st.hal.merkle_build(rng.dev, 4, nodes.dev)
        rc, want = oracle.merkle_build(H(rng), 4)
        assert rc == 0
        nodes.host[:] = fv.units(want)
        return lambda: same(st.hal, nodes)

    return call


def merkle_nodes(kind):
    def role(oracle, pv, st, placement):
        n_leaves = pv.row(kind)[0][0].n // 4 if placement == "whole" else 8  # 2 * (2 * n_leaves - 1): all but two of the array's elements / 30
        n_nodes = 2 * (2 * n_leaves - 1)
        rng = place(pv, st, kind, placement, n_nodes)
        rng = rng.sub(0, n_nodes)
        elems = st.take(4 * n_leaves, "merkle elems")

        def call():
            st.hal.merkle_build(elems.dev, 4, rng.dev)
            rc, want = oracle.merkle_build(H(elems), 4)
            assert rc == 0
            rng.host[:] = fv.units(want)
            return lambda: None

        return call

    return role


def fri_query_codeword(oracle, pv, st, placement):
    rng = place(pv, st, "live", placement, 16)
    arity = 2 if placement == "whole" else 1
    L, depth = log2(rng.n) - arity, 1
    nodes = st.take(2 * ((2 << L) - 1), "query tree")
    term = st.take(4, "terminate")
    idx = [0, (1 << L) - 1, 5 % (1 << L)]

    def tree():
        rc, t = oracle.merkle_build(np.ascontiguousarray(pv.mem[rng.off : rng.end]).copy(), 1 << arity)
        assert rc == 0
        return t

    nodes.host[:] = fv.units(tree())  # (built from the MODEL of what the array will hold; uploaded with the region, before the state)

    def call():
        got = st.hal.fri_query_openings([(rng.dev, nodes.dev, L, arity, depth, 0)], term.dev, idx, L)
        assert np.array_equal(rng.host, pv.mem[rng.off : rng.end])
        t = tree()
        want = [term.host, fv.units(fv.tree_layer(t, depth))]
        for i in idx:
            want.append(rng.host[i << arity : (i + 1) << arity])
            want.append(fv.units(np.stack(fv.tree_branch(t, i, depth))))
        want = np.concatenate(want)

        def check():
            assert L - depth > 0 and np.array_equal(got, want), "openings differ from the model's"

        return check

    return call


def fri_query_terminate(oracle, pv, st, placement):
    rng = place(pv, st, "live", placement, 16)

    def call():
        got = st.hal.fri_query_openings([], rng.dev, [0, 0], 0)
        want = H(rng)

        def check():
            assert np.array_equal(got, want), "the terminate codeword differs from the model's"

        return check

    return call


def copy_d2d_into(kind):
    def role(oracle, pv, st, placement):
        rng = place(pv, st, kind, placement, 16)
        src = st.take(rng.n, "copy source")

        def call():
            st.hal.copy_d2d(src.dev, rng.dev)
            rng.host[:] = src.host
            return lambda: None

        return call

    return role


def copy_d2h_of(oracle, pv, st, placement):
    rng = place(pv, st, "live", placement, 1)

    def call():
        got = st.hal.copy_d2h(rng.dev)
        want = H(rng)

        def check():
            assert np.array_equal(got, want), "the elements read differ from the model's"

        return check

    return call


def gather_one(oracle, pv, st, placement):
    """one item of at most 64 elements (the mailbox route): the item IS the window, so its last / first element is the array's"""
    rng = place(pv, st, "live", placement, 40)
    item = min(64, rng.n)  # (whole: the array's last 64 elements from d_src = its first, so that the call's range covers all of it)

    def call():
        got = st.hal.gather_d2h(rng.dev, [rng.n - item], item)
        want = H(rng)[rng.n - item :]

        def check():
            assert np.array_equal(got.reshape(-1, 2), want), "the gathered item differs from the model"

        return check

    return call


def gather_three(oracle, pv, st, placement):
    """three items (the pinned-buffer route); the largest offset's item ends on the window's last element"""
    rng = place(pv, st, "live", placement, 40)
    offs = [0, 5, rng.n - 4]

    def call():
        got = st.hal.gather_d2h(rng.dev, offs, 4)
        want = np.stack([H(rng)[o : o + 4] for o in offs])

        def check():
            assert np.array_equal(got, want), "the gathered items differ from the model"

        return check

    return call


# name -> (entry point, role, row the range is placed on, does it write there)
ROLES_A = {
    "fri_fold.data_in=live": ("bn_fri_fold", fri_fold_in("live"), "live", False),
    "fri_fold.data_out=live": ("bn_fri_fold", fri_fold_out("live"), "live", True),
    "fri_fold.data_out=x1": ("bn_fri_fold", fri_fold_out("x1"), "x1", True),
    "merkle_build.elems=live": ("bn_merkle_build", merkle_elems, "live", False),
    "merkle_build.nodes=x1": ("bn_merkle_build", merkle_nodes("x1"), "x1", True),
    "merkle_build.nodes=live": ("bn_merkle_build", merkle_nodes("live"), "live", True),  # (x1 has no isolated first element: 2 * (2 n - 1) ends here)
    "gather_d2h.one_item=live": ("bn_gather_d2h", gather_one, "live", False),
    "gather_d2h.three_items=live": ("bn_gather_d2h", gather_three, "live", False),
    "fri_query_openings.codeword=live": ("bn_fri_query_openings", fri_query_codeword, "live", False),
    "fri_query_openings.terminate=live": ("bn_fri_query_openings", fri_query_terminate, "live", False),
    "copy_d2d.dst=x1": ("bn_copy_d2d", copy_d2d_into("x1"), "x1", True),
    "copy_d2d.dst=src0": ("bn_copy_d2d", copy_d2d_into("src0"), "src0", True),
    "copy_d2h.src=live": ("bn_copy_d2h", copy_d2h_of, "live", False),
}
def cases_a():
    out = []
    for state in ds.STATES:
        for name, (_entry, _fn, kind, _w) in ROLES_A.items():
            ps = placements(state, kind)  # (none for src0 where nothing is folded out of place: S3, S4x2)
            if name == "merkle_build.nodes=live":
                ps = ("first", "adj_before")
            out += [(state, name, p) for p in ps]
    return out


def forced_out(state, name, kind, placement, d):
    """What the counters must show the foreign call forced out -- and, beside the array, that it forced nothing out."""
    overlapping = placement in OVERLAPPING
    hosted = {k: v for k, v in d.items() if k.startswith("hosted")}
    if state == "S1":
        assert not d, ("the single-claim state's fold is no group fold", d)  # (flush_legacy runs it whatever the range)
    elif state == "S2":
        assert d.get("flushed_folds", 0) == (1 if overlapping else 0) and not hosted, d
    elif state == "S3":
        assert "hosted_writebacks" not in d and "flushed_folds" not in d, d  # (nothing is pending: a write into the arrays only ends the hosting)
    else:
        wb = d.get("hosted_writebacks", 0)
        assert "flushed_folds" not in d, d
        if not overlapping:
            assert wb == 0, d
        elif kind == "live" or state == "S4x2":  # (S4x2: x1 is the upper half of what the owed write-back covers)
            # (a host read inside ONE current array is answered from the host's copies, as the mailbox mirror answers in S2: the value
            # check alone stands for it)
            assert wb == 1 or (name == "copy_d2h.src=live" and wb == 0), d
        # x1 and src0 (the inputs) in S4: the host folded its copies when the fold was issued; the owed write-back reads neither and writes
        # neither, so a write there forces nothing and may force nothing -- what it must not do is disturb the arrays: the
        # continuation and the final bytes say so.


@gpu
@pytest.mark.parametrize("state,name,placement", cases_a(), ids=lambda v: str(v))
def test_range_scoped_entry_point(contexts, oracle, state, name, placement):
    hal = contexts.get(state)
    _entry, role, kind, _writes = ROLES_A[name]
    box = {}
    st = ds.reach(hal, oracle, state, seed=len(name) + 7 * ds.STATES.index(state), stage=lambda pv, st_: box.update(call=role(oracle, pv, st_, placement)))
    before = hal.group_counters()
    check = box["call"]()
    d = ds.moved(before, hal.group_counters())
    check()
    forced_out(state, name, kind, placement, d)
    st.continuation()
    st.check_bytes()


# ------------------------------------------------------------------------------------------------ B: the blanket-flush entry points
# An op: fn(oracle, pv, st) -> call, as a role of A.  a, b: the first two live arrays of the preview (2^7 elements each in S2 / S4).
def live_bufs(pv, st):
    return [ds.Buf(st, x.off, x.n, "live%d" % j) for j, x in enumerate(pv.live)]


def value_check(got_box, want, what):
    def check():
        assert got_box[0] == want, "%s differs from the oracle's" % what

    return check


def expansion(oracle, coords):
    q = oracle.arr(1 << len(coords))
    q[0, 0] = 1
    if coords:
        assert oracle.tensor_expand(q, 0, list(coords)) == 0
    return q


def staged(st, arr, name):
    b = st.take(arr.shape[0], name)
    b.host[:] = arr
    return b


def op_inner_product(oracle, pv, st):
    a, b = live_bufs(pv, st)[:2]

    def call():
        got = [st.hal.inner_product(a.dev, 7, b.dev)]
        rc, want = oracle.inner_product(H(a), 7, H(b))
        assert rc == 0
        return value_check(got, want, "inner product")

    return call


def op_fold(which):
    def op(oracle, pv, st):
        a = live_bufs(pv, st)[0]
        vec, out = st.take(8, "vec"), st.take(a.n // 8, which + " out")

        def call():
            getattr(st.hal, which)(a.dev, 7, vec.dev, out.dev)
            o = oracle.arr(out.n)
            assert getattr(oracle, which)(H(a), 7, H(vec), o) == 0
            out.host[:] = o
            return lambda: same(st.hal, out)

        return call

    return op


def op_tensor_expand(oracle, pv, st):
    a = live_bufs(pv, st)[0]
    coords = oracle.random_scalars(0x7E50, 2)

    def call():
        st.hal.tensor_expand(log2(a.n) - 2, coords, a.dev)
        data = H(a)
        assert oracle.tensor_expand(data, log2(a.n) - 2, coords) == 0
        a.host[:] = data
        return lambda: None

    return call


COMPOSITE = [("var", 0), ("var", 1), ("mul", 0, 1), ("add", 2, 0)]


def op_compute_composite(oracle, pv, st):
    a, b = live_bufs(pv, st)[:2]
    out = st.take(a.n, "composite out")

    def call():
        cache = st.hal.__dict__.setdefault("_deferred_visibility_exprs", {})
        if "composite" not in cache:
            cache["composite"] = st.hal.compile_expr(COMPOSITE)
        st.hal.compute_composite([a.dev, b.dev], out.dev, cache["composite"])
        o = oracle.arr(out.n)
        assert oracle.compute_composite([H(a), H(b)], o, COMPOSITE) == 0
        out.host[:] = o
        return lambda: same(st.hal, out)

    return call


def op_pairwise_product_reduce(oracle, pv, st):
    a = live_bufs(pv, st)[0]
    outs = [st.take(a.n >> (r + 1), "pairwise round %d" % r) for r in range(log2(a.n))]

    def call():
        st.hal.pairwise_product_reduce(a.dev, [o.dev for o in outs])
        hs = [oracle.arr(o.n) for o in outs]
        assert oracle.pairwise_product_reduce(H(a), hs) == 0
        for o, h in zip(outs, hs):
            o.host[:] = h
        return lambda: [same(st.hal, o) for o in outs]

    return call


def op_ntt(which):
    def op(oracle, pv, st):
        a = live_bufs(pv, st)[0]

        def call():
            getattr(st.hal, which)(a.dev.ptr, 7, 5, s_evals(oracle), 10, 0, log2(a.n), 0)
            data = H(a)
            assert getattr(oracle, which)(data, 7, 5, s_evals(oracle), 10, 0, log2(a.n), 0) == 0
            a.host[:] = data
            return lambda: None

        return call

    return op


def op_groestl256_leaves(oracle, pv, st):
    a = live_bufs(pv, st)[0]
    out = st.take(2 * (a.n // 4), "leaf digests")

    def call():
        st.hal.groestl256_leaves(a.dev, 4, out.dev)
        rc, nodes = oracle.merkle_build(H(a), 4)
        assert rc == 0
        out.host[:] = fv.units(nodes[: a.n // 4])
        return lambda: same(st.hal, out)

    return call


def op_groestl256_compress_layer(oracle, pv, st):
    a = live_bufs(pv, st)[0]  # 2^6 digests
    out = st.take(a.n // 2, "compressed layer")

    def call():
        st.hal.groestl256_compress_layer(a.dev, out.dev)
        ds_ = fv.digests(H(a))
        want = b"".join(oracle.groestl256_compress2(ds_[2 * i], ds_[2 * i + 1]) for i in range(len(ds_) // 2))
        out.host[:] = np.frombuffer(want, dtype=np.uint64).reshape(-1, 2)
        return lambda: same(st.hal, out)

    return call


def op_hal_fold_multilinear(oracle, pv, st):
    a = live_bufs(pv, st)[0]
    out = st.take(a.n, "hal fold out")
    z = oracle.random_scalars(0x4A1F, 1)[0]

    def call():
        n = st.hal.hal_fold_multilinear(1, log2(a.n), ("folded", a.dev, 0), z, None, out.dev)
        rc, want = oracle.hal_fold_multilinear(1, log2(a.n), ("folded", H(a), 0), z)
        assert rc == 0 and n == want.shape[0]
        out.host[:n] = want
        return lambda: same(st.hal, out)

    return call


AB = [("var", 0), ("var", 1), ("mul", 0, 1)]


def op_hal_round_evals(oracle, pv, st):
    a, b = live_bufs(pv, st)[:2]

    def call():
        cache = st.hal.__dict__.setdefault("_deferred_visibility_exprs", {})
        if "ab" not in cache:
            cache["ab"] = st.hal.compile_expr(AB)
        c = cache["ab"]
        got = [st.hal.hal_round_evals(1, log2(a.n), None, [("folded", a.dev, 0), ("folded", b.dev, 0)],
                                      [{"composition": c, "composition_at_infinity": c, "start": 1, "end": 3, "eq_ind": None}], [])]
        rc, want = oracle.hal_round_evals(1, log2(a.n), None, [("folded", H(a), 0), ("folded", H(b), 0)],
                                          [{"steps": AB, "steps_inf": AB, "start": 1, "end": 3, "eq_ind": None}], [])
        assert rc == 0
        return value_check(got, want, "round evaluations")

    return call


def op_mle_evaluate_batch(oracle, pv, st):
    a, b = live_bufs(pv, st)[:2]
    point = oracle.random_scalars(0x3E7A, log2(a.n))
    lo, hi = staged(st, expansion(oracle, point[:3]), "point lo"), staged(st, expansion(oracle, point[3:]), "point hi")

    def call():
        got = [st.hal.mle_evaluate_batch([(a.dev, 7, log2(a.n), 0), (b.dev, 7, log2(b.n), 0)], [(lo.dev, 3, hi.dev, len(point) - 3)])]
        want = [oracle.mle_evaluate(H(x), log2(x.n), point) for x in (a, b)]
        return value_check(got, want, "evaluations")

    return call


def op_partial_eval_high_batch(oracle, pv, st):
    import evalcheck_ref

    a, b = live_bufs(pv, st)[:2]
    suffix = oracle.random_scalars(0x9E4A, 3)
    query = staged(st, evalcheck_ref.eq_expand(suffix), "query")
    outs = [st.take(a.n >> 3, "projection %d" % j) for j in range(2)]

    def call():
        st.hal.partial_eval_high_batch([(a.dev, 7, log2(a.n)), (b.dev, 7, log2(b.n))], query.dev, 3, [o.dev for o in outs])
        for x, o in zip((a, b), outs):
            o.host[:] = evalcheck_ref.project(H(x), 7, log2(x.n), suffix)
        return lambda: [same(st.hal, o) for o in outs]

    return call


def op_partial_eval_high_lincomb_batch(oracle, pv, st):
    import evalcheck_lincomb_ref
    import evalcheck_ref

    a, b = live_bufs(pv, st)[:2]
    suffix = oracle.random_scalars(0x9E4B, 3)
    c0, c1, offset = oracle.random_scalars(0x9E4C, 3)
    query = staged(st, evalcheck_ref.eq_expand(suffix), "query")
    out = st.take(a.n >> 3, "lincomb projection")

    def call():
        st.hal.partial_eval_high_lincomb_batch([(log2(a.n), [(a.dev, 7, c0), (b.dev, 7, c1)], offset)], query.dev, 3, [out.dev])
        out.host[:] = evalcheck_lincomb_ref.project_lincomb([(H(a), 7, c0), (H(b), 7, c1)], offset, log2(a.n), suffix)
        return lambda: same(st.hal, out)

    return call


def op_merge_multilins(oracle, pv, st):
    from oracle import piop_ref

    a, b = live_bufs(pv, st)[:2]
    msg = st.take(4 * a.n, "message")

    def call():
        st.hal.merge_multilins([a.dev, b.dev], msg.dev, log2(a.n) + 2)
        msg.host[:] = piop_ref.merge_multilins([H(a), H(b)], log2(a.n) + 2)
        return lambda: same(st.hal, msg)

    return call


def op_product_tree_layers(oracle, pv, st):
    import gkr_gpa_ref

    a = live_bufs(pv, st)[0]
    arena = st.take(a.n, "tree arena")

    def call():
        got = [st.hal.product_tree_layers([log2(a.n)], [a.dev], [arena.dev])]
        layers = gkr_gpa_ref.product_layers(H(a), log2(a.n))
        arena.host[1:] = gkr_gpa_ref.heap_arena(layers)[1:]  # (element 0 of the arena is not defined: whatever it held stays)
        want = [oracle.arr_to_ints(layers[0])[0]]

        def check():
            assert got[0] == want, "the product differs from the oracle's"
            assert np.array_equal(st.hal.copy_d2h(arena.dev)[1:], arena.host[1:]), "the layers differ from the oracle's"

        return check

    return call


def op_pad_with_ones(oracle, pv, st):
    import gkr_gpa_ref

    a = live_bufs(pv, st)[0]
    out = st.take(2 * a.n, "padded")

    def call():
        st.hal.pad_with_ones([log2(a.n) + 1], [a.dev], [out.dev])
        out.host[:] = gkr_gpa_ref.pad_ones(H(a), log2(a.n) + 1)
        return lambda: same(st.hal, out)

    return call


def op_univariate_fold_batch(oracle, pv, st):
    """the live array as a packed B8 column (the op takes levels 0 and 3): 2^(7 + 4) values, skip_rounds 2"""
    a = live_bufs(pv, st)[0]
    n_vars, k = log2(a.n) + 4, 2
    coeffs = oracle.random_scalars(0x0F01D, 1 << k)
    out = st.take(1 << (n_vars - k), "univariate fold out")

    def call():
        st.hal.univariate_fold_batch([(a.dev, 3, n_vars)], k, coeffs, [out.dev])
        o = oracle.arr(out.n)
        assert oracle.fold_right(H(a), 3, oracle.ints_to_arr(coeffs), o) == 0
        out.host[:] = o
        return lambda: same(st.hal, out)

    return call


def op_ring_switch_eq_ind_batch(oracle, pv, st):
    """output INTO the live array"""
    import ring_switch_ref

    a = live_bufs(pv, st)[0]
    kappa = 2
    mixing = oracle.random_scalars(0x5C1A, 1)[0]
    coeffs = oracle.random_scalars(0x5C1B, 1 << kappa)
    query = staged(st, expansion(oracle, oracle.random_scalars(0x5C1C, log2(a.n))), "suffix table")

    def call():
        st.hal.ring_switch_eq_ind_batch([(query.dev, log2(a.n), kappa, mixing)], coeffs, [a.dev])
        a.host[:] = ring_switch_ref.eq_ind_from_query(H(query), kappa, mixing, coeffs)
        return lambda: None

    return call


def op_xor_reduce(oracle, pv, st):
    import binius_amd
    from binius_amd._ffi import F128, from_f128

    a = live_bufs(pv, st)[0]
    group_len, n_groups = 16, a.n // 16

    def call():
        out = (F128 * group_len)()
        rc = binius_amd.lib().bn_xor_reduce(st.hal._h, C.c_void_p(a.dev.ptr), n_groups, group_len, out)
        assert rc == 0
        got = [[from_f128(out[i]) for i in range(group_len)]]
        want = oracle.arr_to_ints(np.bitwise_xor.reduce(H(a).reshape(n_groups, group_len, 2), axis=0))
        return value_check(got, want, "xor reduction")

    return call


def op_fill(oracle, pv, st):
    a = live_bufs(pv, st)[0]
    v = oracle.random_scalars(0xF111, 1)[0]

    def call():
        st.hal.fill(a.dev.slice(1, a.n - 1), v)  # (its first and last element stay the fold's)
        a.host[1 : a.n - 1] = oracle.ints_to_arr([v])[0]
        return lambda: None

    return call


def op_copy_h2d(oracle, pv, st):
    a = live_bufs(pv, st)[0]
    data = oracle.random_b128(0xC0B1, a.n - 2)

    def call():
        st.hal.copy_h2d(data, a.dev.slice(1, a.n - 1))
        a.host[1 : a.n - 1] = data
        return lambda: None

    return call


def op_bits_to_b128(oracle, pv, st):
    """output INTO the live array"""
    import gkr_exp_ref

    a = live_bufs(pv, st)[0]
    bits = (oracle.splitmix_words(0xB175, a.n) & np.uint64(1)).astype(np.uint8)
    src = staged(st, gkr_exp_ref.pack_bits(bits), "bit column")

    def call():
        st.hal.bits_to_b128([log2(a.n)], [src.dev], [a.dev])
        a.host[:] = gkr_exp_ref.bits_to_b128(bits)
        return lambda: None

    return call


def op_exp_circuit_layers(oracle, pv, st):
    """the live array as the dynamic base"""
    import gkr_exp_ref

    a = live_bufs(pv, st)[0]
    bits = [(oracle.splitmix_words(0xE4B0 + k, a.n) & np.uint64(1)).astype(np.uint8) for k in range(2)]
    cols = [staged(st, gkr_exp_ref.pack_bits(b), "exponent bits %d" % k) for k, b in enumerate(bits)]
    arena = st.take(2 * a.n, "exp layers")

    def call():
        st.hal.exp_circuit_layers([log2(a.n)], [[c.dev for c in cols]], [a.dev], [arena.dev])
        arena.host[:] = np.concatenate(gkr_exp_ref.exp_layers(bits, H(a), "dynamic"))
        return lambda: same(st.hal, arena)

    return call


def op_flush_witness_batch(oracle, pv, st):
    """the live array as a B128 column under a selector of ones"""
    import flush_ref

    a = live_bufs(pv, st)[0]
    ones = np.ones(a.n, dtype=np.uint8)
    sel = staged(st, flush_ref.pack_bits(ones), "selector")
    coeff, const = oracle.random_scalars(0xF1A5, 2)
    out = st.take(a.n, "flush witness")

    def call():
        got = [st.hal.flush_witness_batch([log2(a.n)], [[sel.dev]], [[(a.dev, 7, coeff)]], [const], [out.dev])]
        prefix, want = flush_ref.flush_witness(log2(a.n), [ones], [(H(a), 7, coeff)], const)
        assert prefix == a.n
        out.host[:] = want

        def check():
            assert got[0] == [prefix], "prefix length differs from the restatement's"
            same(st.hal, out)

        return check

    return call


def op_derive_columns_batch(oracle, pv, st):
    """the XOR of two live arrays as B128 columns"""
    import derive_ref

    a, b = live_bufs(pv, st)[:2]
    offset = oracle.random_scalars(0xDE21, 1)[0]
    out = st.take(a.n, "derived column")

    def call():
        st.hal.derive_columns_batch([{"kind": "xor", "level": 7, "n_vars": log2(a.n), "terms": [a.dev, b.dev], "offset": offset, "out": out.dev}])
        terms = [derive_ref.unpack(H(x), 7, log2(x.n)) for x in (a, b)]
        out.host[:] = derive_ref.pack(derive_ref.xor_combination(terms, offset, 7, log2(a.n)), 7)
        return lambda: same(st.hal, out)

    return call


def op_generate_columns_batch(oracle, pv, st):
    """output INTO the live array: the powers of a B128 base"""
    import generate_ref

    a = live_bufs(pv, st)[0]
    base = oracle.random_scalars(0x6E4E, 1)[0]

    def call():
        st.hal.generate_columns_batch([{"kind": "powers", "level": 7, "n_vars": log2(a.n), "value": base, "out": a.dev}])
        a.host[:] = generate_ref.pack(generate_ref.powers(base, 7, log2(a.n)), 7)
        return lambda: None

    return call


SQUARE = [("var", 0), ("var", 0), ("mul", 0, 1)]


def op_zerocheck_univariate_evals(oracle, pv, st):
    """the live array as a packed B8 column: 2^(7 + 4) values, skip_rounds 2"""
    import univariate_skip_ref as R

    a = live_bufs(pv, st)[0]
    n_vars, k = log2(a.n) + 4, 2
    ch = oracle.random_scalars(0x7A00, n_vars - k)
    eq = staged(st, oracle.ints_to_arr(R.eq_expansion(ch)), "eq")

    def call():
        got = [st.hal.zerocheck_univariate_evals(n_vars, k, [(a.dev, 3)], [SQUARE], [2], eq.dev, 2 << k)]
        want = R.univariate_evals([(R.unpack(H(a), 3, n_vars), 3)], n_vars, k, [SQUARE], [2], ch, 2 << k)
        return value_check(got, want, "univariate round evaluations")

    return call


def op_zerocheck_univariate_evals_base(oracle, pv, st):
    """the live array as a B128 column under a composition over B128"""
    import univariate_skip_base_ref as RB
    import univariate_skip_ref as R

    a = live_bufs(pv, st)[0]
    n_vars, k = log2(a.n), 2
    ch = oracle.random_scalars(0x7A01, n_vars - k)
    eq = staged(st, oracle.ints_to_arr(R.eq_expansion(ch)), "eq")

    def call():
        got = [st.hal.zerocheck_univariate_evals_base(7, n_vars, k, [(a.dev, 7)], [SQUARE], [2], eq.dev, 2 << k)]
        want = RB.univariate_evals(7, [(RB.unpack(H(a), 7, n_vars), 7)], n_vars, k, [SQUARE], [2], ch, 2 << k)
        return value_check(got, want, "univariate round evaluations")

    return call


OPS_B = {
    "inner_product": ("bn_inner_product", op_inner_product),
    "fold_left": ("bn_fold_left", op_fold("fold_left")),
    "fold_right": ("bn_fold_right", op_fold("fold_right")),
    "tensor_expand": ("bn_tensor_expand", op_tensor_expand),
    "compute_composite": ("bn_compute_composite", op_compute_composite),
    "pairwise_product_reduce": ("bn_pairwise_product_reduce", op_pairwise_product_reduce),
    "ntt_forward": ("bn_ntt_forward", op_ntt("ntt_forward")),
    "ntt_inverse": ("bn_ntt_inverse", op_ntt("ntt_inverse")),
    "groestl256_leaves": ("bn_groestl256_leaves", op_groestl256_leaves),
    "groestl256_compress_layer": ("bn_groestl256_compress_layer", op_groestl256_compress_layer),
    "hal_fold_multilinear": ("bn_hal_fold_multilinear", op_hal_fold_multilinear),
    "hal_round_evals": ("bn_hal_round_evals", op_hal_round_evals),
    "mle_evaluate_batch": ("bn_mle_evaluate_batch", op_mle_evaluate_batch),
    "partial_eval_high_batch": ("bn_partial_eval_high_batch", op_partial_eval_high_batch),
    "partial_eval_high_lincomb_batch": ("bn_partial_eval_high_lincomb_batch", op_partial_eval_high_lincomb_batch),
    "merge_multilins": ("bn_merge_multilins", op_merge_multilins),
    "product_tree_layers": ("bn_product_tree_layers", op_product_tree_layers),
    "pad_with_ones": ("bn_pad_with_ones", op_pad_with_ones),
    "univariate_fold_batch": ("bn_univariate_fold_batch", op_univariate_fold_batch),
    "ring_switch_eq_ind_batch": ("bn_ring_switch_eq_ind_batch", op_ring_switch_eq_ind_batch),
    "xor_reduce": ("bn_xor_reduce", op_xor_reduce),
    "fill": ("bn_fill", op_fill),
    "copy_h2d": ("bn_copy_h2d", op_copy_h2d),
    "bits_to_b128": ("bn_bits_to_b128", op_bits_to_b128),
    "exp_circuit_layers": ("bn_exp_circuit_layers", op_exp_circuit_layers),
    "flush_witness_batch": ("bn_flush_witness_batch", op_flush_witness_batch),
    "derive_columns_batch": ("bn_derive_columns_batch", op_derive_columns_batch),
    "generate_columns_batch": ("bn_generate_columns_batch", op_generate_columns_batch),
    "zerocheck_univariate_evals": ("bn_zerocheck_univariate_evals", op_zerocheck_univariate_evals),
    "zerocheck_univariate_evals_base": ("bn_zerocheck_univariate_evals_base", op_zerocheck_univariate_evals_base),
}


@gpu
@pytest.mark.parametrize("name", list(OPS_B))
@pytest.mark.parametrize("state", ["S2", "S4"])
def test_blanket_flush_entry_point(contexts, oracle, state, name):
    hal = contexts.get(state)
    box = {}
    st = ds.reach(hal, oracle, state, seed=0xB00 + len(name), stage=lambda pv, st_: box.update(call=OPS_B[name][1](oracle, pv, st_)))
    before = hal.group_counters()
    check = box["call"]()
    d = ds.moved(before, hal.group_counters())
    check()
    # every one of them operates on a live array: what was waiting has run
    if state == "S2":
        assert d.get("flushed_folds", 0) == 1, d
    else:
        assert d.get("hosted_writebacks", 0) == 1, d
    st.continuation()
    st.check_bytes()


# ------------------------------------------------------------------------------------------------ C: completeness (CPU)
# Entry points that take device memory and are in neither table, each with the reason.
EXEMPT = {
    "bn_arena_base": "returns the arena's address: touches no device memory",
    "bn_host_scratch": "returns pinned host memory: touches no device memory",
    "bn_extrapolate_line": "the deferring call itself: the states are made of it (deferred_states.Prover.fold)",
    "bn_extrapolate_line_batch": "the deferring call itself: the states are made of it (deferred_states.Prover.fold)",
    "bn_extrapolate_line_batch_scaled": "the deferring call itself, with a scale: never a claim-group fold (group_fold_applies), covered by the sumcheck suites",
    "bn_kernel_launch": "the prover's own evaluation: every case's execute() and continuation",
}

# Entry points that are declared with a context but no device memory among their arguments: outside the tables by construction.  Listed here so
# that one which grows a device pointer has to move into a table, each with the reason.
NO_DEVICE_MEMORY = {
    "bn_fold_counters": "read-only query of host counters (which kernel answered bn_fold_left / bn_fold_right): no device memory, launches and flushes nothing",
    "bn_inner_product_counters": "read-only query of host counters (which kernel answered bn_inner_product): no device memory, launches and flushes nothing",
    "bn_hal_counters": "read-only query of host counters (which route answered bn_hal_round_evals, the branches inside it): no device memory, launches and flushes nothing",
}

DEVICE_ARG = re.compile(r"\bvoid\s*\*\s*(?:const\s*)?\*?\s*d_\w+|\b(?:void|bn_hal_multilinear|bn_memmap)\s*\*\s*(?:jobs|cols|points|mls|ml|maps|oracles)\b")


def device_entry_points(device=True):
    """every `int bn_*(bn_ctx *ctx, ...)` of the public header with a device pointer, or a table of them, among its arguments
    (device=False: those without one)"""
    text = open(os.path.join(ROOT, "include", "binius_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = []
    for m in re.finditer(r"\bint\s+(bn_\w+)\s*\(\s*bn_ctx\s*\*\s*ctx\s*,([^;]*?)\)\s*;", text, flags=re.S):
        if bool(DEVICE_ARG.search(m.group(2))) == device:
            names.append(m.group(1))
    return names


def test_entry_point_tables_are_complete():
    """A new entry point that takes device memory fails here until someone decides where it belongs: a role of A (range-scoped), an
    op of B (blanket flush) or EXEMPT with the reason."""
    names = device_entry_points()
    assert len(names) >= 40 and "bn_gather_d2h" in names and "bn_mle_evaluate_batch" in names and "bn_generate_columns_batch" in names, names
    covered = {entry for entry, _fn, _kind, _w in ROLES_A.values()} | {entry for entry, _fn in OPS_B.values()}
    assert not covered & set(EXEMPT), "an entry point is both tested and exempt: %s" % sorted(covered & set(EXEMPT))
    missing = [n for n in names if n not in covered and n not in EXEMPT]
    assert not missing, "entry points that take device memory and are in no table of this file: %s" % missing
    stale = [n for n in list(covered) + list(EXEMPT) if n not in names]
    assert not stale, "names in the tables that the header no longer declares: %s" % stale
    assert all(isinstance(r, str) and len(r) > 10 for r in EXEMPT.values())
    # the queries that take no device memory are declared, are in no table, and stay without a device pointer
    hostonly = device_entry_points(device=False)
    for n, reason in NO_DEVICE_MEMORY.items():
        assert n in hostonly and n not in names and n not in covered and n not in EXEMPT and len(reason) > 10, n
    # the issue's list for B
    for op in ("inner_product", "fold_left", "fold_right", "tensor_expand", "compute_composite", "pairwise_product_reduce", "ntt_forward", "groestl256_leaves",
               "hal_fold_multilinear", "hal_round_evals", "mle_evaluate_batch", "partial_eval_high_batch", "partial_eval_high_lincomb_batch", "merge_multilins",
               "product_tree_layers", "pad_with_ones", "univariate_fold_batch", "ring_switch_eq_ind_batch", "xor_reduce", "fill"):
        assert op in OPS_B


def test_case_tables_cover_every_state_and_placement():
    cases = cases_a()
    assert len(set(cases)) == len(cases)
    for state in ds.STATES:
        for name, (_e, _f, kind, _w) in ROLES_A.items():
            got = {p for s, n, p in cases if s == state and n == name}
            if kind not in ds.ISOLATED[state]:
                assert not got
            else:
                assert got & set(OVERLAPPING) and got & set(ADJACENT), (state, name, got)
