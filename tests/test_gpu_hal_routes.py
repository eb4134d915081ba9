"""GPU parity of bn_hal_round_evals on every route and every branch inside the routes, on the cases of tests/hal_cases.py: the interpreter
kernel (one variable, below the rows' floor in both orders, its grid stride), rows + compiled circuits with the points side by side (both
orders, the second launch of the rows kernel past 24 rows, its grid stride over Low-to-High pairs) and point by point (halves in place, a
truncated multilinear written, Low-to-High), the monomial route (constants, lone columns below and on the streaming sum, three factors,
jobs under an indicator, its refusals) with the strided matrix-core launch of Low-to-High pairs at every stride pair, the constraint set's
two launches narrow and wide, wide requests dealt out, the coefficient form and Transparent multilinears.  The routes are reached by the
request's shape, and `Context.hal_counters()` (bn_hal_counters) says which ran: every case asserts the counter difference of its call.

Every case, on a context created with the case's switches: the values are the oracle's, bit for bit -- nothing is compared with the device's
own output; the difference of the counters is the one tests/hal_cases.py derives from the request; a second identical call (the plan cache of
the constraint set and the constant tables are reused) gives the same values and the same difference; multilinears, tensor query and
indicator sit at odd multiples of 16 bytes between canary frames (tests/adversarial.py), unchanged afterwards with every frame intact.  Sizes
that depend on the number of compute units are computed for the device the test runs on, and the test asserts that they give what they
are named after.  The table and the oracle are pinned on the CPU by tests/test_oracle_hal_cases.py.
"""
import os

import pytest

import adversarial as A
import hal_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def n_cu():
    """The compute units of the device as the library's launchers see them (bn_hal_counters reports them beside the counters)."""
    import binius_amd

    with binius_amd.Context(0, 64) as ctx:
        n = ctx.hal_counters()["n_cu"]
        assert n == ctx.fold_counters()["n_cu"]
    assert 32 <= n <= 4096
    return n


def context_for(c, elements):
    """A fresh context with the case's switches in the environment while it is created (they are read then)."""
    import binius_amd

    old = {k: os.environ.get(k) for k in c.env}
    os.environ.update(c.env)
    try:
        return binius_amd.Context(0, elements)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_shape_on_this_device(c, n_cu):
    """The size rules give, on this device, what they are named after; every case keeps its route and tags."""
    req = H.request(c, n_cu)
    half = 1 << (req.n_vars - 1)
    assert H.hal_tags(req, n_cu) == (c.route, c.tags)
    if isinstance(c.n_vars, tuple):
        rule, k = c.n_vars
        if rule == "mfma":
            assert H.mfma_applies(n_cu, half) == bool(k) and H.mfma_applies(n_cu, 2 * half) and not H.mfma_applies(n_cu, half // 2)
        elif rule == "groups":
            assert -(-half // (2 * H.K_TP)) > 2 * n_cu
        elif rule == "interp":
            assert half > 1024 * n_cu
        else:
            launches, _ = H.rows_plan(req)
            assert half // 256 > -(-8 * n_cu // max(launches))
    return req


def counters_moved(before, after):
    assert sorted(before) == sorted(after) and after["n_cu"] == before["n_cu"]
    return {k: after[k] - before[k] for k in before if k not in H.HAL_INFO}


@pytest.mark.parametrize("case", H.HAL_CASES, ids=lambda c: c.id)
def test_hal_case(oracle, n_cu, case):
    c = case
    req = check_shape_on_this_device(c, n_cu)
    mls, query, eq, points, evs = H.inputs(oracle, c, n_cu)
    want = H.reference(oracle, c, n_cu)
    arrays = [m[1] for m in mls] + [x for x in (query, eq) if x is not None]
    hal = context_for(c, sum(a.shape[0] + 2 * A.FRAME + 32 for a in arrays) + 4096)
    try:
        alloc = hal.dev_alloc()
        checks, d_mls = [], []
        for j, m in enumerate(mls):
            d, chk = A.place(hal, alloc, m[1] if m[1].shape[0] else 0, 1 + 2 * (j % 8))  # (an empty multilinear: a block of canary, none of it read)
            checks.append(chk)
            d_mls.append((m[0], d) + tuple(m[2:]))
        d_q = d_eq = None
        if query is not None:
            d_q, chk = A.place(hal, alloc, query, 3)
            checks.append(chk)
        if eq is not None:
            d_eq, chk = A.place(hal, alloc, eq, 7)
            checks.append(chk)
        exprs, d_evs = [], []
        for e in evs:
            comp, inf = hal.compile_expr(e["steps"]), hal.compile_expr(e["steps_inf"])
            exprs += [comp, inf]
            d_evs.append({"composition": comp, "composition_at_infinity": inf, "start": e["start"], "end": e["end"], "eq_ind": d_eq if e["eq_ind"] is not None else None})
        expect = H.hal_counters(req, n_cu)
        assert expect[c.route] >= 1
        c0 = hal.hal_counters()
        got = hal.hal_round_evals(c.order, req.n_vars, d_q, d_mls, d_evs, points)
        c1 = hal.hal_counters()
        again = hal.hal_round_evals(c.order, req.n_vars, d_q, d_mls, d_evs, points)
        c2 = hal.hal_counters()
        for x in exprs:
            x.free()
        print("%s (n_vars %d): %s" % (c.id, req.n_vars, ", ".join("%s %d" % kv for kv in H.moved(counters_moved(c0, c1)).items())))
        assert got == want, "case %s: values differ from the oracle's" % c.id
        assert counters_moved(c0, c1) == expect, "case %s: the call moved %s, its request gives %s" % (c.id, H.moved(counters_moved(c0, c1)), H.moved(expect))
        assert again == want, "case %s: the second call's values differ" % c.id
        assert counters_moved(c1, c2) == expect, "case %s: the second call moved %s" % (c.id, H.moved(counters_moved(c1, c2)))
        for chk in checks:
            chk()
    finally:
        hal.close()


def test_requests_without_a_value_and_rejected_requests_move_no_counter(oracle):
    import binius_amd

    with binius_amd.Context(0, 1 << 12) as hal:
        alloc = hal.dev_alloc()
        x = alloc.alloc(16)
        hal.copy_h2d(oracle.random_b128(1, 16), x)
        comp = hal.compile_expr(H.AB)
        mls = [("folded", x, 0), ("folded", x, 0)]
        c0 = hal.hal_counters()
        assert hal.hal_round_evals(1, 4, None, mls, [{"composition": comp, "composition_at_infinity": comp, "start": 2, "end": 2, "eq_ind": None}], []) == [[]]
        with pytest.raises(binius_amd.BnError):  # five points need two domain points
            hal.hal_round_evals(1, 4, None, mls, [{"composition": comp, "composition_at_infinity": comp, "start": 0, "end": 5, "eq_ind": None}], [7])
        with pytest.raises(binius_amd.BnError):  # composition over more variables than multilinears
            hal.hal_round_evals(0, 4, None, mls[:1], [{"composition": comp, "composition_at_infinity": comp, "start": 0, "end": 3, "eq_ind": None}], [])
        assert hal.hal_counters() == c0
        got = hal.hal_round_evals(1, 4, None, mls, [{"composition": comp, "composition_at_infinity": comp, "start": 1, "end": 3, "eq_ind": None}], [])
        assert got == oracle.hal_round_evals(1, 4, None, [("folded", oracle.random_b128(1, 16), 0)] * 2, [{"steps": H.AB, "steps_inf": H.AB, "start": 1, "end": 3, "eq_ind": None}], [])[1]
        assert H.moved(counters_moved(c0, hal.hal_counters())) == {"monomials": 1, "mono_product2": 1}
        comp.free()
