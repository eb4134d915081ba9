"""GPU parity of bn_fold_right / bn_fold_left / bn_inner_product on every branch of the kernels that answer them, on the cases of
tests/fold_cases.py: k_fold_tab's wide and entry-sized loads, its LDS chunks and partial groups; k_fold's grid stride, single output and
single vector element; k_linmap_ring<R> / k_linmap_ring_left<R> with one, two and four pairs of blocks per workgroup behind every table
preparation; the fold_left calls handed to the partial-evaluation kernel; k_ip32, k_inner_product and the two split kernels around their
thresholds.  The branches are reached by shape, and `Context.fold_counters()` / `Context.inner_product_counters()` (bn_fold_counters,
bn_inner_product_counters) say which kernel answered: every case asserts the counter difference of its one call.

Every case: the output is the oracle's, bit for bit; nothing is compared with the device's own output.  Matrix, vector and output sit at
odd multiples of 16 bytes between canary frames (tests/adversarial.py); the inputs must be unchanged and every frame intact.  Sizes that
depend on the number of compute units are computed for the device the test runs on, and the test asserts that they give the pairs per
workgroup / outputs per thread they are there for.  The tables and the oracle are pinned on the CPU by tests/test_oracle_fold_cases.py.
"""
import numpy as np
import pytest

import adversarial as A
import fold_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def n_cu():
    """The compute units of the device as the library's launchers see them (bn_fold_counters reports them beside the counters)."""
    import binius_amd

    with binius_amd.Context(0, 64) as ctx:
        n = ctx.fold_counters()["n_cu"]
    assert 32 <= n <= 4096  # (4096 outputs are one pair per workgroup)
    return n


@pytest.fixture(scope="module")
def hal(n_cu):
    import binius_amd

    # the largest case: matrix, vector and output, each between two frames
    need = max(F.mat_len(c, n_cu) + c.vec_len + F.out_len(c, n_cu) for c in F.FOLD_CASES)
    need = max(need, max(2 * F.ip_len(c, n_cu) for c in F.IP_CASES))
    ctx = binius_amd.Context(0, need + 3 * (2 * A.FRAME + 16) + 64)
    yield ctx
    ctx.close()


def moved(before, after):
    """The difference of two counter readings, the last-launch record of the folds apart."""
    assert sorted(before) == sorted(after)
    assert after["n_cu"] == before["n_cu"]
    return {k: after[k] - before[k] for k in before if k not in F.FOLD_LAST + F.FOLD_INFO}


def check_shape_on_this_device(c, n_cu):
    """The size rules give, on this device, what they are named after; every other case is answered by the same route on every device."""
    n_out = F.out_len(c, n_cu)
    route, tags = F.fold_tags(c.op, c.level, c.vec_len, n_out, n_cu)
    assert route == c.route
    if isinstance(c.out, tuple) and c.out[0] == "pairs":
        assert F.ring_pairs(n_out, n_cu) >= c.out[1] and F.ring_grid(n_out, n_cu) == 2 * n_cu
    elif isinstance(c.out, tuple):
        assert F.scalar_outputs_per_thread(n_out, n_cu) >= c.out[1]
    elif not route.endswith("_mfma"):
        assert tags == c.tags
    return n_out


def run_fold(hal, c, mat, vec, want, n_cu):
    """One call of case `c` on (mat, vec) between canary frames: output `want`, inputs unchanged, counters moved by the case's route only."""
    n_out = want.shape[0]
    alloc = hal.dev_alloc()
    dm, chk_m = A.place(hal, alloc, mat, 1)
    dv, chk_v = A.place(hal, alloc, vec, 3)
    do, chk_o = A.place(hal, alloc, n_out, 5)
    chk_o()  # (the body holds the canary)
    c0 = hal.fold_counters()
    (hal.fold_left if c.op == "left" else hal.fold_right)(dm, c.level, dv, do)
    c1 = hal.fold_counters()
    chk_o(want)
    chk_m()
    chk_v()
    delta, last = F.fold_counters(c.op, c.level, c.vec_len, n_out, n_cu)
    assert delta[c.route] == 1
    assert moved(c0, c1) == delta, "case %s: the call moved %s" % (c.id, {k: v for k, v in moved(c0, c1).items() if v})
    if last is None:
        assert {k: c1[k] for k in F.FOLD_LAST} == {k: c0[k] for k in F.FOLD_LAST}
    else:
        assert {k: c1[k] for k in F.FOLD_LAST} == last, "case %s: the matrix-core launch was %s" % (c.id, {k: c1[k] for k in F.FOLD_LAST})
        # what the record says about the launch that ran: pairs of blocks of its busiest workgroup
        pairs = -(-(n_out // 64) // c1["last_grid"])
        want_pairs = c.out[1] if isinstance(c.out, tuple) else 1
        assert pairs >= want_pairs and (want_pairs > 1 or pairs == 1), "case %s ran %d pairs per workgroup" % (c.id, pairs)
    return moved(c0, c1)


@pytest.mark.parametrize("case", F.FOLD_CASES, ids=lambda c: c.id)
def test_fold_case(hal, oracle, n_cu, case):
    c = case
    check_shape_on_this_device(c, n_cu)
    mat, vec = F.fold_inputs(oracle, c, n_cu)
    d = run_fold(hal, c, mat, vec, F.fold_reference(oracle, c, n_cu), n_cu)
    print("%s: %s" % (c.id, ", ".join(k for k, v in d.items() if v)))


RING_TWICE = [c for c in F.FOLD_CASES if c.route.endswith("_mfma") and isinstance(c.out, tuple)]
assert len(RING_TWICE) == 15


@pytest.mark.parametrize("case", RING_TWICE, ids=lambda c: c.id)
def test_ring_case_with_a_one_hot_vector(hal, oracle, n_cu, case):
    """The workgroups' second and later pairs with a vector that is 1 in one place: the output is one entry of every row (fold_right) or one
    row (fold_left) of the matrix, taken out of it in numpy -- a wrong table shows on every block, a wrong ring slot on the later ones."""
    c = case
    n_out = check_shape_on_this_device(c, n_cu)
    mat, _ = F.fold_inputs(oracle, c, n_cu)
    vec, j = F.one_hot(c.vec_len)
    run_fold(hal, c, mat, vec, F.one_hot_expected(mat, c.level, c, j, n_out), n_cu)


def test_routes_back_to_back_share_the_scratch(hal, oracle, n_cu):
    """A matrix-core fold, a table fold and the matrix-core fold again on one context: the linear map's table lives in the context's scratch,
    which the calls in between may use too.  Each output equals the call's own."""
    seq = ["right-l3-v128-opairs2", "right-l3-v256-o1024", "right-l3-v128-opairs2", "left-l5-v64-opairs2", "left-l0-v4096-o1024", "left-l5-v64-o2048",
           "left-l5-v64-opairs2"]
    assert [F.FOLD_BY_ID[k].route for k in seq] == ["right_mfma", "right_tab", "right_mfma", "left_mfma", "left_pe", "left_tab", "left_mfma"]
    cases = [F.FOLD_BY_ID[k] for k in seq]
    alloc = hal.dev_alloc()
    placed = {}
    for k in sorted(set(seq)):
        c = F.FOLD_BY_ID[k]
        mat, vec = F.fold_inputs(oracle, c, n_cu)
        lead = 1 + 2 * (len(placed) % 4)
        placed[k] = (A.place(hal, alloc, mat, lead), A.place(hal, alloc, vec, lead + 6), A.place(hal, alloc, F.out_len(c, n_cu), lead + 8))
    c0 = hal.fold_counters()
    for c in cases:  # (no read-back between the calls)
        (dm, _), (dv, _), (do, _) = placed[c.id]
        (hal.fold_left if c.op == "left" else hal.fold_right)(dm, c.level, dv, do)
    c1 = hal.fold_counters()
    for k, ((_, chk_m), (_, chk_v), (_, chk_o)) in placed.items():
        chk_o(F.fold_reference(oracle, F.FOLD_BY_ID[k], n_cu))
        chk_m()
        chk_v()
    d = moved(c0, c1)
    assert {k: v for k, v in d.items() if v} == {"right_mfma": 2, "right_tab": 1, "left_mfma": 2, "left_pe": 1, "left_tab": 1, "ring4": 2, "ring_left8": 2}


def test_the_same_output_buffer_after_another_route(hal, oracle, n_cu):
    """matrix cores, nibble tables, matrix cores into ONE output buffer, read back after each call: what a call leaves is its own result."""
    big, small = F.FOLD_BY_ID["right-l4-v128-opairs2"], F.FOLD_BY_ID["right-l4-v128-o1024"]
    n_big, n_small = F.out_len(big, n_cu), F.out_len(small, n_cu)
    alloc = hal.dev_alloc()
    (mb, vb), (ms, vs) = F.fold_inputs(oracle, big, n_cu), F.fold_inputs(oracle, small, n_cu)
    dmb, dvb = A.place(hal, alloc, mb, 7)[0], A.place(hal, alloc, vb, 9)[0]
    dms, dvs = A.place(hal, alloc, ms, 11)[0], A.place(hal, alloc, vs, 13)[0]
    do, chk_o = A.place(hal, alloc, n_big, 15)
    hal.fold_right(dmb, 4, dvb, do)
    first = chk_o(F.fold_reference(oracle, big, n_cu)).copy()
    hal.fold_right(dms, 4, dvs, do.slice(0, n_small))
    chk_o(np.concatenate([F.fold_reference(oracle, small, n_cu), first[n_small:]]))
    hal.fold_right(dmb, 4, dvb, do)
    chk_o(first)


def test_rejected_folds_move_no_counter(hal, oracle):
    import binius_amd

    alloc = hal.dev_alloc()
    dm, chk_m = A.place(hal, alloc, oracle.random_b128(0xBAD0, 64), 1)
    dv, chk_v = A.place(hal, alloc, oracle.random_b128(0xBAD1, 4), 3)
    do, chk_o = A.place(hal, alloc, 64, 5)
    c0, i0 = hal.fold_counters(), hal.inner_product_counters()
    for fold in (hal.fold_left, hal.fold_right):
        for level, n_out in ((7, 32), (7, 8), (1, 64), (2, 64), (8, 16)):  # wrong out_len (twice); no such tower level in this library
            with pytest.raises(binius_amd.BnError) as e:
                fold(dm, level, dv, do.slice(0, n_out))
            assert e.value.kind == "InputValidation"
        with pytest.raises(binius_amd.BnError):
            fold(dv, 7, dm, do.slice(0, 1))  # query larger than the evaluations
    for level, na, nb in ((4, 8, 32), (8, 8, 8), (2, 8, 8 << 5), (1, 1, 64), (7, 4, 3)):
        with pytest.raises(binius_amd.BnError) as e:
            hal.inner_product(dm.slice(0, na), level, do.slice(0, nb) if nb <= 64 else alloc.alloc(nb))
        assert e.value.kind == "InputValidation"
    assert hal.fold_counters() == c0 and hal.inner_product_counters() == i0
    chk_m()
    chk_v()
    chk_o()


# ---------------------------------------------------------------------------------------------- inner product
@pytest.mark.parametrize("case", F.IP_CASES, ids=lambda c: c.id)
def test_inner_product_case(hal, oracle, n_cu, case):
    c = case
    n_b = F.ip_len(c, n_cu)
    route, _ = F.ip_tags(c.level, n_b, n_cu)
    assert route == c.route
    if isinstance(c.b, tuple):
        assert F.mfma_applies(n_cu, n_b // 2) == bool(c.b[1]) and -(-(n_b // 2) // F.K_TP) == n_cu - 1 + c.b[1]
    a, b = F.ip_inputs(oracle, c, n_cu)
    alloc = hal.dev_alloc()
    da, chk_a = A.place(hal, alloc, a, 1)
    db, chk_b = A.place(hal, alloc, b, 3)
    c0, f0 = hal.inner_product_counters(), hal.fold_counters()
    got = hal.inner_product(da, c.level, db)
    c1 = hal.inner_product_counters()
    assert got == F.ip_reference(oracle, c, n_cu)
    chk_a()
    chk_b()
    assert {k: c1[k] - c0[k] for k in c0} == F.ip_counters(c, n_cu), "case %s: the call moved %s" % (c.id, {k: c1[k] - c0[k] for k in c0})
    assert hal.fold_counters() == f0
    print("%s: %s" % (c.id, route))


def test_inner_products_in_a_row_start_from_zero(hal, oracle, n_cu):
    """The four kernels XOR into the same accumulator slots: calls of different routes one after the other each return their own sum."""
    ids = ["ip-l5-8704", "ip-l7-2", "ip-l5-8448", "ip-l7-mfma1", "ip-l7-1", "ip-l7-mfma0", "ip-l5-8192"]
    alloc = hal.dev_alloc()
    placed = []
    for k in ids:
        c = F.IP_BY_ID[k]
        a, b = F.ip_inputs(oracle, c, n_cu)
        placed.append((c, A.place(hal, alloc, a, 1)[0], A.place(hal, alloc, b, 3)[0]))
    c0 = hal.inner_product_counters()
    for _ in range(2):
        for c, da, db in placed:
            assert hal.inner_product(da, c.level, db) == F.ip_reference(oracle, c, n_cu), c.id
    c1 = hal.inner_product_counters()
    assert {k: c1[k] - c0[k] for k in c0} == {"mfma_split": 2, "split9": 4, "ip32": 4, "scalar": 4}
