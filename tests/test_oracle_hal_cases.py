"""Pins of the case table of tests/hal_cases.py, on the CPU, so that tests/test_gpu_hal_routes.py checks what it was written to check:

* every row's hand-written route and branch tags are what the restated predicates of binius_amd/csrc/abi_hal.cpp give for its request on a
  device of 256 compute units, and the sizes written as rules resolve to what the rules are named after on other devices too;
* every route and every branch the table is there for is claimed by a row, and every counter of bn_hal_counters is moved by one;
* the names of Context.hal_counters() follow the enum of include/binius_amd.h, and the restated constants are the sources';
* the oracle is right on the inputs that are new here: on the small rows oracle.hal_round_evals equals the pure-Python evaluation of the
  definition (tests/test_oracle_hal.py: one hypercube point at a time, sharing only the scalar product), and a Low-to-High request on
  interleaved arrays equals the High-to-Low request on the split arrays -- the identity that lets the large Low-to-High rows trust the C
  restatement.
"""
import os
import re

import numpy as np
import pytest

import hal_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("case", H.HAL_CASES, ids=lambda c: c.id)
def test_case_claims_what_its_request_gives(case):
    c = case
    req = H.request(c)
    route, tags = H.hal_tags(req)
    assert route == c.route, "case %s is answered by %s" % (c.id, route)
    assert tags == c.tags, "case %s: claimed %s, its request gives %s" % (c.id, sorted(c.tags), sorted(tags))
    d = H.hal_counters(req)
    assert d[route] >= 1
    if route == "in_parts":
        assert d["in_parts"] == 1 and sum(d[k] for k in H.HAL_ROUTES) == 1 + len(H.deal_parts(req)) >= 3
    else:
        assert sum(d[k] for k in H.HAL_ROUTES) == 1
    # what the entry point checks before it routes: a pass of the general code carries the request or it is dealt out
    assert len(req.evs) >= 1 and all(e.start < e.end for e in req.evs)
    assert req.n_points == max(max(e.end for e in req.evs) - 3, 0) <= H.MAX_PTS
    for e in req.evs:
        assert len(e.steps) <= 64 and len(e.steps_inf) <= 64 and H.expr_n_vars(e.steps) <= len(req.mls)
    assert set(c.env) <= {"BN_HAL_COEF", "BN_HAL_EQ_SET", "BN_CIRCUIT_MULTIPASS"}


def test_every_route_and_branch_is_claimed_by_a_case():
    claimed = set().union(*(c.tags for c in H.HAL_CASES))
    missing = [t for t in H.HAL_REQUIRED_TAGS if t not in claimed]
    assert not missing, "no case claims %s" % missing
    assert claimed <= set(H.HAL_REQUIRED_TAGS), "tags that no one asked for: %s" % sorted(claimed - set(H.HAL_REQUIRED_TAGS))
    assert {c.route for c in H.HAL_CASES} == set(H.HAL_ROUTES)
    # every counter is moved by a row -- and every route also by a row that is not a part of a wide request
    total = {k: 0 for k in H.HAL_ROUTES + H.HAL_BRANCHES}
    for c in H.HAL_CASES:
        for k, v in H.hal_counters(H.request(c)).items():
            total[k] += v
    assert all(total.values()), "counters no row moves: %s" % [k for k, v in total.items() if not v]
    # the wide requests: their parts land on two routes, in both orders; one under an indicator is one constraint set
    for cid, parts in (("parts-h2l", {"monomials", "interpreter"}), ("parts-l2h", {"rows_batched", "interpreter"}), ("eqset-wide-off", {"monomials"})):
        assert {H.hal_route(p) for p in H.deal_parts(H.request(H.HAL_BY_ID[cid]))} == parts
    assert H.moved(H.hal_counters(H.request(H.HAL_BY_ID["eqset-wide"]))) == {"eq_set": 1}


def test_the_issue_s_rows_are_in_the_table():
    by = H.HAL_BY_ID
    shape = lambda cid: (by[cid].order, H.n_vars_of(by[cid]))
    assert shape("interp-n1") == (H.H2L, 1) and shape("interp-n10-h2l") == (H.H2L, 10) and shape("interp-n10-l2h") == (H.L2H, 10)
    assert shape("rows-n11-h2l") == (H.H2L, 11) and shape("rows-n11-l2h") == (H.L2H, 11)
    assert [shape(k) for k in ("perpoint-in-place", "perpoint-truncated", "perpoint-l2h")] == [(H.H2L, 21), (H.H2L, 21), (H.L2H, 21)]
    assert shape("mono-n2") == (H.H2L, 2) and shape("mono-lone-n18") == (H.H2L, 18) and shape("mono-lone-n19") == (H.H2L, 19)
    d = lambda cid: H.moved(H.hal_counters(H.request(by[cid])))
    assert d("rows-25") == {"rows_batched": 1, "rows_launches": 2, "rows_written": 25}
    assert d("perpoint-in-place")["rows_in_place"] == 3 and d("perpoint-truncated")["rows_in_place"] == 2 and "rows_in_place" not in d("perpoint-l2h")
    assert d("perpoint-l2h")["rows_written"] == 9
    assert d("mono-lone-n18") == {"monomials": 1, "mono_product2": 2} and d("mono-lone-n19") == {"monomials": 1, "mono_product2": 1, "mono_xor_sum": 4}
    assert d("strided-mfma1") == {"monomials": 1, "mono_strided": 4} and d("strided-mfma0")["rows_batched"] == 1
    assert d("mono-mixed-eq") == {"monomials": 1, "mono_product2": 3, "mono_product3": 1}
    assert d("transparent-mono")["transparent"] == 1 and d("transparent-rows")["transparent"] == 1
    # sixteen distinct monomials, eight to a composition; thirteen in one
    jobs = {(v, e.eq) for e in by["mono-16-jobs"].evs for v, _ in H.expand_poly(e.steps)}
    assert len(jobs) == 16 and all(len(H.expand_poly(e.steps)) == 8 for e in by["mono-16-jobs"].evs)
    assert H.expand_poly(H.THIRTEEN) is None and len(H.expand_poly(H.P(*H._PAIRS[:12]))) == 12
    assert not H.sum_plan_accepts(H.SEVENTEEN_SUMMANDS) and H.sum_plan_accepts(H.P(*([(0,), (1,)] * 8))) and H.expand_poly(H.SEVENTEEN_SUMMANDS) == [((0,), 1)]


def test_sizes_written_as_rules():
    by = H.HAL_BY_ID
    assert H.n_vars_of(by["strided-mfma1"]) == 17 and H.n_vars_of(by["strided-mfma0"]) == 16 and H.n_vars_of(by["rows-l2h-ab-eq"]) == 17
    assert H.n_vars_of(by["strided-groups2"]) == 20 and H.n_vars_of(by["interp-grid-stride"]) == 20 and H.n_vars_of(by["rows-l2h-grid"]) == 18
    # one n_vars above the threshold a workgroup still takes ONE group of two tiles (2 n_cu workgroups): the second comes at 2^19 points
    assert H.strided_groups_per_workgroup(1 << 17, 256) == 1 and H.strided_groups_per_workgroup(1 << 18, 256) == 1 and H.strided_groups_per_workgroup(1 << 19, 256) == 2
    assert H.interp_points_per_thread(1 << 18, 256) == 1 and H.interp_points_per_thread(1 << 19, 256) == 2
    assert H.rows_blocks_per_workgroup(1 << 16, 8, 256) == 1 and H.rows_blocks_per_workgroup(1 << 17, 8, 256) == 2
    # other devices: the rules still give what they are named after, and the rows keep their routes and tags
    for n_cu in (64, 104, 120, 228, 256, 304):
        for c in H.HAL_CASES:
            if isinstance(c.n_vars, int):
                continue
            req = H.request(c, n_cu)
            half = 1 << (req.n_vars - 1)
            assert H.hal_tags(req, n_cu) == (c.route, c.tags), (c.id, n_cu)
            rule, k = c.n_vars
            if rule == "mfma":
                assert H.mfma_applies(n_cu, half) == bool(k) and H.mfma_applies(n_cu, 2 * half) and not H.mfma_applies(n_cu, half // 2)
            elif rule == "groups":
                assert H.strided_groups_per_workgroup(half, n_cu) >= k > H.strided_groups_per_workgroup(half // 2, n_cu)
            elif rule == "interp":
                assert H.interp_points_per_thread(half, n_cu) >= k > H.interp_points_per_thread(half // 2, n_cu) and half > 1024 * n_cu
            else:
                launches, _ = H.rows_plan(req)
                assert max(H.rows_blocks_per_workgroup(half, n, n_cu) for n in launches) >= k and half // 256 > -(-8 * n_cu // max(launches))


def test_restated_constants_are_the_sources():
    src = lambda *p: open(os.path.join(ROOT, "binius_amd", "csrc", *p)).read()
    hal, internal, circuit, rows = src("abi_hal.cpp"), src("internal.hpp"), src("abi_circuit.cpp"), src("kernels_hal.hip")
    assert "constexpr size_t kMaxTerms = %d;" % H.MAX_TERMS in hal and "pl.jobs.size() > %d" % H.MAX_MONO_JOBS in hal
    assert "constexpr int kHalMaxMl = %d, kHalMaxEv = %d, kHalMaxPts = %d;" % (H.MAX_ML, H.MAX_EV, H.MAX_PTS) in internal
    assert "constexpr int kHalMaxRows = %d;" % H.MAX_ROWS in internal and "values_asked(r) > %d" % H.MAX_PASS_VALUES in hal
    assert "row_len >= %d" % H.ROWS_FLOOR in circuit and "summands.size() + stack.size() > %d" % H.MAX_SUMMANDS in circuit
    assert "r.batch_points = r.half <= ((uint64_t)1 << 19);" in hal and H.BATCH_POINTS_MAX_HALF == 1 << 19
    assert "job.vars.size() == 1 && half >= ((uint64_t)1 << 18)" in hal and H.XOR_SUM_MIN_HALF == 1 << 18
    assert "const uint64_t cap = (uint64_t)n_cu * 4;" in rows and "const uint64_t cap = ((uint64_t)n_cu * 8 + a.n_jobs - 1) / a.n_jobs;" in rows


def test_counter_names_follow_the_header():
    import binius_amd._ffi as f

    text = open(os.path.join(ROOT, "include", "binius_amd.h")).read()
    enum = re.search(r"enum\s*\{([^}]*BN_HALCNT_N\b[^}]*)\}", text).group(1)
    names = {m.group(1): int(m.group(2)) for m in re.finditer(r"BN_HALCNT_(\w+)\s*=\s*(\d+)", enum)}
    assert names.pop("N") == len(f.Context.HAL_COUNTERS) == len(names)
    assert [k for k, _ in sorted(names.items(), key=lambda kv: kv[1])] == [k.upper() for k in f.Context.HAL_COUNTERS]
    assert f.Context.HAL_COUNTERS == H.HAL_ROUTES + H.HAL_BRANCHES + H.HAL_INFO
    assert "bn_hal_counters" in f.ABI_SYMBOLS
    rust = open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read()
    assert "pub const BN_HALCNT_N: usize = %d;" % len(f.Context.HAL_COUNTERS) in rust


def test_the_polynomial_expansion_restated():
    K = H.K1
    assert H.expand_poly(H.AB_PLUS_C) == [((2,), 1), ((0, 1), 1)]
    assert H.expand_poly(H.P((0, 1), K)) == [((), K), ((0, 1), 1)]
    assert H.expand_poly(H.P((K, 0, 1))) == [((0, 1), K)]
    assert H.expand_poly(H.P((0,), (0,))) == [] and H.expand_poly(H.P((0, 1, 2, 3))) is None
    assert H.expand_poly([("var", 1), ("pow", 0, 3)]) == [((1, 1, 1), 1)] and H.expand_poly([("var", 1), ("pow", 0, 4)]) is None
    assert H.expand_poly([("var", 0), ("var", 1), ("add", 0, 1), ("mul", 2, 2)]) == [((0, 0), 1), ((1, 1), 1)]   # (a + b)^2: the cross terms cancel


# ---------------------------------------------------------------------------------------------- the oracle on the new inputs
SMALL = [c for c in H.HAL_CASES if isinstance(c.n_vars, int) and c.n_vars <= 8]


@pytest.mark.parametrize("case", SMALL + [H.HAL_BY_ID["interp-n10-l2h"]._replace(id="interp-n6-l2h", n_vars=6), H.HAL_BY_ID["rows-25"]._replace(id="rows-25-n5", n_vars=5),
                                          H.HAL_BY_ID["mono-16-jobs"]._replace(id="mono-16-jobs-n4", n_vars=4), H.HAL_BY_ID["strided-mfma1"]._replace(id="strided-n5", n_vars=5),
                                          H.HAL_BY_ID["parts-l2h"]._replace(id="parts-l2h-n5", n_vars=5)], ids=lambda c: c.id)
def test_oracle_equals_the_definition_on_the_small_rows(oracle, case):
    """The rows of at most eight variables, and the compositions of the larger ones (seventeen summands, sixteen monomials, nine evaluators,
    a constant under an indicator, an empty multilinear) at a few variables: the C restatement against one point at a time in Python."""
    from test_oracle_hal import py_round_evals

    c = case
    assert len(SMALL) >= 5
    mls, query, _eq, points, evs = H.inputs(oracle, c)
    assert query is None
    n_vars = H.n_vars_of(c)
    rc, got = oracle.hal_round_evals(c.order, n_vars, None, mls, evs, points)
    assert rc == 0
    cols = [(oracle.arr_to_ints(m[1]) if m[1].shape[0] else [], m[1].shape[0], m[2]) for m in mls]
    assert got == py_round_evals(c.order, n_vars, cols, evs, points)
    assert any(v for vals in got for v in vals)


@pytest.mark.parametrize("cid", ["strided-mfma1", "rows-l2h-grid", "perpoint-l2h"])
def test_low_to_high_on_interleaved_arrays_is_high_to_low_on_the_split_ones(oracle, cid):
    """At n_vars = 12, with the requests of the large Low-to-High rows: pairs (2i, 2i + 1) of y are pairs (i, i + half) of x when
    y[0::2], y[1::2] = x[:half], x[half:]."""
    c = H.HAL_BY_ID[cid]._replace(n_vars=12)
    mls, _q, _eq, points, evs = H.inputs(oracle, c)
    half = 1 << 11
    split = []
    for kind, y, sfx in mls:
        assert kind == "folded" and y.shape[0] == 2 * half
        split.append((kind, np.ascontiguousarray(np.concatenate([y[0::2], y[1::2]])), sfx))
    rc0, a = oracle.hal_round_evals(H.L2H, 12, None, mls, evs, points)
    rc1, b = oracle.hal_round_evals(H.H2L, 12, None, split, evs, points)
    assert rc0 == 0 and rc1 == 0 and a == b and any(v for vals in a for v in vals)
