"""The case table of the route tests of bn_hal_round_evals, shared by tests/test_oracle_hal_cases.py (which pins the table on the CPU) and
tests/test_gpu_hal_routes.py (which runs it on the device).

A request is answered by one of seven routes (binius_amd/csrc/abi_hal.cpp: route_coef, route_eq_set, route_in_parts, route_monomials,
route_rows_batched, route_rows_per_point, route_interpreter) with further branches inside them, and `Context.hal_counters()`
(bn_hal_counters) says which.  A row names the route and the branches it is there for (its tags), written out by hand; `hal_route`,
`hal_counters` and `hal_tags` below restate the routing predicates and derive the route, the counter difference of one call and the tags
from the request alone, and the CPU module holds the two against each other.  A case that was chosen to reach a branch fails when a
threshold moves and it stops reaching it.

Restated: is_wide, the decline conditions of round_evals_coef and round_evals_eq_set (without the widths of their launches -- 512 element-wise
jobs, 1024 group jobs and slots -- which no row comes near), expand_poly and plan_monomials with the 12-term, 15-job and factor limits,
circuit_multipass_applies' 1024-row floor and the 16 summands of sum_plan (without the planner's 24 live temporaries: the rows' circuits
have a handful of steps), batch_points, the in-place rule and the 24-row flush of build_rows, the dealing of round_evals_in_parts,
bn::mfma_applies and the grids of launch_hal_round_evals, launch_hal_rows and the strided matrix-core launch.  The measurement switches
of mfma_applies (BN_EVAL, BN_MFMA_MIN_TILES) are taken as unset.

Sizes that depend on the number of compute units are written as a rule -- ("mfma", 1): the smallest n_vars whose half cube fills one
256-point tile per unit, ("mfma", 0): one below it; ("groups", 2): the smallest n_vars at which a workgroup of the strided matrix-core launch
takes a second group of two tiles; ("interp", 2): at which a thread of the interpreter kernel takes a second point; ("rows", 2): at which a
workgroup of the rows kernel takes a second block of 256 outputs, for the rows of the case -- and resolved by `n_vars_of` for the device at
hand (256 units in the CPU module).
"""
import zlib
from collections import namedtuple

import numpy as np

NOMINAL_CU = 256
L2H, H2L = 0, 1

HAL_ROUTES = ("coef", "eq_set", "in_parts", "monomials", "rows_batched", "rows_per_point", "interpreter")
HAL_BRANCHES = ("mono_strided", "mono_product2", "mono_product3", "mono_xor_sum", "mono_const", "rows_launches", "rows_written", "rows_in_place", "transparent")
HAL_INFO = ("n_cu",)

# ---------------------------------------------------------------------------------------------- the library's constants, restated
MAX_TERMS = 12          # abi_hal.cpp kMaxTerms: monomials of one composition
MAX_MONO_JOBS = 15      # plan_monomials: distinct (monomial, indicator) jobs of a request
MAX_ML, MAX_EV, MAX_PTS = 16, 8, 13   # internal.hpp kHalMaxMl, kHalMaxEv, kHalMaxPts
MAX_PASS_VALUES = 32    # values of one pass of the general code
MAX_ROWS = 24           # kHalMaxRows: jobs of one launch of k_hal_rows
ROWS_FLOOR = 1024       # circuit_multipass_applies: shortest row of rows + compiled circuits
MAX_SUMMANDS = 16       # abi_circuit.cpp sum_plan
BATCH_POINTS_MAX_HALF = 1 << 19
XOR_SUM_MIN_HALF = 1 << 18
K_TP = 256              # gram.hpp kTP: points per tile of the matrix-core sum of products

Ev = namedtuple("Ev", "steps steps_inf start end eq")   # eq: which indicator table the evaluator is under (any true value; equal = the same table), or None / False
Req = namedtuple("Req", "order n_vars mls evs n_points env")
# mls: ("full",) | ("trunc", stored length, suffix) | ("transparent", tower level, query variables)


def P(*terms):
    """Steps of a sum of monomials: a term is a tuple of variable indices, or (constant, variables...) with an int constant >= 2^32 in
    front, or a bare int constant.  The monomials' products nest to the left, the sum nests to the left."""
    steps, tops = [], []
    for t in terms:
        if isinstance(t, int):
            steps.append(("const", t))
            tops.append(len(steps) - 1)
            continue
        cst = None
        if t and t[0] >= 1 << 32:
            cst, t = t[0], t[1:]
        top = None
        if cst is not None:
            steps.append(("const", cst))
            top = len(steps) - 1
        for v in t:
            steps.append(("var", v))
            if top is None:
                top = len(steps) - 1
            else:
                steps.append(("mul", top, len(steps) - 1))
                top = len(steps) - 1
        tops.append(top)
    acc = tops[0]
    for t in tops[1:]:
        steps.append(("add", acc, t))
        acc = len(steps) - 1
    return steps


K1 = 0x0123456789ABCDEF0FEDCBA987654321
K2 = 0x1234567890ABCDEF1122334455667788
AB, ABC, LIN_A = P((0, 1)), P((0, 1, 2)), P((0,))
AB_PLUS_C, ABC_PLUS_A, AB_PLUS_A = P((0, 1), (2,)), P((0, 1, 2), (0,)), P((0, 1), (0,))


# ---------------------------------------------------------------------------------------------- expand_poly
def _cmul(x, y):
    if x == 1:
        return y
    if y == 1:
        return x
    raise AssertionError("a case multiplies two constants: the table's compositions keep their constants apart")


def expand_poly(steps):
    """abi_hal.cpp expand_poly: the composition as [(variables sorted, coefficient)], shorter monomials first, or None where the library
    gives up (a monomial of more than three variables, a power above 3, more than 4 * 12 terms on the way or 12 at the end)."""
    def add_term(p, t):
        if t[1] == 0:
            return
        for i, (v, c) in enumerate(p):
            if v == t[0]:
                if c ^ t[1]:
                    p[i] = (v, c ^ t[1])
                else:
                    del p[i]
                return
        p.append(t)

    def mul(x, y):
        r = []
        for vx, cx in x:
            for vy, cy in y:
                if len(vx) + len(vy) > 3:
                    return None
                add_term(r, (tuple(sorted(vx + vy)), _cmul(cx, cy)))
        return r if len(r) <= 4 * MAX_TERMS else None

    val = []
    for i, s in enumerate(steps):
        if s[0] == "var":
            r = [((s[1],), 1)]
        elif s[0] == "const":
            r = []
            add_term(r, ((), s[1]))
        elif s[0] == "add":
            if s[1] >= i or s[2] >= i:
                return None
            r = list(val[s[1]])
            for t in val[s[2]]:
                add_term(r, t)
        elif s[0] == "mul":
            if s[1] >= i or s[2] >= i:
                return None
            r = mul(val[s[1]], val[s[2]])
            if r is None:
                return None
        elif s[0] == "pow":
            if s[1] >= i or s[2] > 3:
                return None
            r = [((), 1)]
            for _ in range(s[2]):
                r = mul(r, val[s[1]])
                if r is None:
                    return None
        else:
            return None
        val.append(r)
    if not steps:
        return []
    fin = sorted(val[-1], key=lambda t: (len(t[0]), t[0]))
    return fin if len(fin) <= MAX_TERMS else None


def expr_n_vars(steps):
    return max([s[1] + 1 for s in steps if s[0] == "var"] or [0])


def sum_plan_accepts(steps):
    """abi_circuit.cpp sum_plan: the summands of the root, at most 16 of them at any moment of the expansion"""
    if not steps:
        return False
    stack, summands = [len(steps) - 1], 0
    while stack:
        s = steps[stack.pop()]
        if s[0] == "add":
            stack += [s[1], s[2]]
        else:
            summands += 1
        if summands + len(stack) > MAX_SUMMANDS:
            return False
    return True


# ---------------------------------------------------------------------------------------------- the routing predicates
def mfma_applies(n_cu, n_points):
    return -(-n_points // K_TP) >= n_cu


def _on(req, knob):
    return req.env.get(knob, "1") != "0"


def _is_full(req, m):
    return m[0] == "full" or (m[0] == "trunc" and m[1] >= 1 << req.n_vars)


def _total(req):
    return sum(max(e.end - e.start, 0) for e in req.evs)


def is_wide(req):
    return len(req.mls) > MAX_ML or len(req.evs) > MAX_EV or _total(req) > MAX_PASS_VALUES


def coef_declines(req):
    """round_evals_coef, and route_coef in front of it"""
    if not (req.order == H2L and _on(req, "BN_HAL_COEF") and _on(req, "BN_GROUP")) or req.n_vars < 2 or not req.evs:
        return "order or switch"
    if not all(_is_full(req, m) for m in req.mls):
        return "multilinear not full"
    pt_hi = 0
    for e in req.evs:
        if e.eq != req.evs[0].eq or e.start < 1 or e.start > e.end:
            return "indicator or point 0"
        if expr_n_vars(e.steps) > len(req.mls) or expr_n_vars(e.steps_inf) > len(req.mls):
            return "variables"
        pt_hi = max(pt_hi, e.end)
    if req.n_points != (pt_hi - 3 if pt_hi > 3 else 0) or _total(req) == 0:
        return "points"
    deg = 0
    for e in req.evs:
        want1 = (e.start <= 1 < e.end) or e.end > 3
        want_inf = e.start <= 2 < e.end
        for want, steps in ((want1, e.steps), (want_inf, e.steps_inf)):
            if not want:
                continue
            p = expand_poly(steps)
            if p is None:
                return "not a polynomial of degree 3"
            deg = max([deg] + [len(v) for v, _ in p])
    if pt_hi <= 3 and deg < 3:
        return "degree below 3 without domain points"
    return None


def eq_set_declines(req, wide):
    """route_eq_set and round_evals_eq_set"""
    if not (wide or (req.evs and req.evs[0].eq)):
        return "narrow without an indicator"
    if not (req.order == H2L and req.n_points == 0 and _on(req, "BN_HAL_EQ_SET")):
        return "order, domain points or switch"
    if not req.evs or not req.evs[0].eq or not _on(req, "BN_GROUP"):
        return "no indicator"
    if not all(_is_full(req, m) for m in req.mls):
        return "multilinear not full"
    for e in req.evs:
        if e.eq != req.evs[0].eq or e.start < 1 or e.end > 3:
            return "indicator or points"
    for e in req.evs:
        for steps in (e.steps, e.steps_inf):
            p = expand_poly(steps)
            if p is None or any(len(v) > 2 or any(x >= len(req.mls) for x in v) for v, _ in p):
                return "monomial of more than two columns"
    return None


def point_range(req):
    return min(e.start for e in req.evs), max(e.end for e in req.evs)


def plan_monomials(req, n_cu):
    """abi_hal.cpp plan_monomials: the jobs [(variables, under the indicator, held by a form at infinity)] in the order they are launched,
    or the reason it refuses"""
    l2h = req.order == L2H
    lo, hi = point_range(req)
    all_full = all(m[0] == "transparent" or _is_full(req, m) for m in req.mls)
    if l2h and not mfma_applies(n_cu, 1 << (req.n_vars - 1)):
        return "Low-to-High below the matrix-core threshold"
    if not (all_full and lo >= 1 and hi <= 3 and req.n_vars >= 2):
        return "truncated, points or n_vars"
    jobs = []
    for e in req.evs:
        p1, pinf = expand_poly(e.steps), expand_poly(e.steps_inf)
        if p1 is None or pinf is None:
            return "more than 12 terms"
        for which, p in ((0, p1), (1, pinf)):
            for v, _ in p:
                if len(v) + (1 if e.eq else 0) > (2 if l2h else 3):
                    return "factors"
                for j in jobs:
                    if j[0] == v and j[1] == e.eq:
                        break
                else:
                    j = [v, e.eq, False]
                    jobs.append(j)
                if which:
                    j[2] = True
        if len(jobs) > MAX_MONO_JOBS:
            return "more than 15 jobs"
    return [tuple(j) for j in jobs]


def rows_ok(req):
    """plan_scratch (its scratch granted)"""
    half = 1 << (req.n_vars - 1)
    if not (_on(req, "BN_CIRCUIT_MULTIPASS") and req.evs[0].steps and half >= ROWS_FLOOR and _total(req) <= MAX_PASS_VALUES):
        return False
    return all(sum_plan_accepts(s) for e in req.evs for s in (e.steps, e.steps_inf))


def general_route(req, n_cu):
    if not isinstance(plan_monomials(req, n_cu), str):
        return "monomials"
    if rows_ok(req):
        return "rows_batched" if 1 << (req.n_vars - 1) <= BATCH_POINTS_MAX_HALF else "rows_per_point"
    return "interpreter"


def hal_route(req, n_cu=NOMINAL_CU):
    """The route that answers the request (a request that asks for no value is answered by none: None)."""
    if _total(req) == 0:
        return None
    if coef_declines(req) is None:
        return "coef"
    wide = is_wide(req)
    if eq_set_declines(req, wide) is None:
        return "eq_set"
    if wide:
        return "in_parts"
    return general_route(req, n_cu)


def deal_parts(req):
    """round_evals_in_parts: the requests the evaluators of a wide one are dealt out to"""
    parts, e0 = [], 0
    while e0 < len(req.evs):
        used, e1, pts, pt_hi = [], e0, 0, 0
        while e1 < len(req.evs) and e1 - e0 < MAX_EV:
            e = req.evs[e1]
            fresh = []
            for steps in (e.steps, e.steps_inf):
                for s in steps:
                    if s[0] == "var" and s[1] not in used and s[1] not in fresh:
                        fresh.append(s[1])
            cnt = e.end - e.start
            fits = len(used) + len(fresh) <= MAX_ML and pts + cnt <= MAX_PASS_VALUES
            if not fits and e1 > e0:
                break
            assert fits
            used += fresh
            pts += cnt
            pt_hi = max(pt_hi, e.end)
            e1 += 1
        local = {v: i for i, v in enumerate(used)}
        sub = lambda steps: [("var", local[s[1]]) if s[0] == "var" else s for s in steps]
        evs = [Ev(sub(e.steps), sub(e.steps_inf), e.start, e.end, e.eq) for e in req.evs[e0:e1]]
        parts.append(req._replace(mls=[req.mls[v] for v in used], evs=evs, n_points=pt_hi - 3 if pt_hi > 3 else 0))
        e0 = e1
    return parts


def rows_plan(req):
    """build_rows: (jobs per launch of k_hal_rows, halves read in place)"""
    half = 1 << (req.n_vars - 1)
    batch = half <= BATCH_POINTS_MAX_HALF
    used = {s[1] for e in req.evs for steps in (e.steps, e.steps_inf) for s in steps if s[0] == "var"}
    lo, hi = point_range(req)
    written = in_place = 0
    for k, m in enumerate(req.mls):
        if k not in used:
            continue
        for p in range(lo, hi):
            if not any(e.start <= p < e.end for e in req.evs):
                continue
            if not batch and req.order == H2L and (m[0] == "transparent" or _is_full(req, m)) and p <= 1:
                in_place += 1
            else:
                written += 1
    launches = [MAX_ROWS] * (written // MAX_ROWS) + ([written % MAX_ROWS] if written % MAX_ROWS else [])
    return launches, in_place


def hal_counters(req, n_cu=NOMINAL_CU):
    """What one call adds to Context.hal_counters() (HAL_ROUTES and HAL_BRANCHES)."""
    d = {k: 0 for k in HAL_ROUTES + HAL_BRANCHES}
    route = hal_route(req, n_cu)
    if route is None:
        return d
    d[route] += 1
    if route == "in_parts":
        for part in deal_parts(req):
            for k, v in hal_counters(part, n_cu).items():
                d[k] += v
    if route not in ("monomials", "rows_batched", "rows_per_point", "interpreter"):
        return d
    d["transparent"] = sum(1 for m in req.mls if m[0] == "transparent")
    half = 1 << (req.n_vars - 1)
    if route == "monomials":
        for v, eq, at_inf in plan_monomials(req, n_cu):
            if not v and not eq:
                d["mono_const"] += 1
            elif req.order == H2L and not eq and len(v) == 1 and half >= XOR_SUM_MIN_HALF:
                d["mono_xor_sum"] += 3 if at_inf else 1
            elif req.order == L2H:
                d["mono_strided"] += 1
            else:
                d["mono_product3" if len(v) + (1 if eq else 0) == 3 else "mono_product2"] += 1
    elif route != "interpreter":
        launches, in_place = rows_plan(req)
        d["rows_launches"], d["rows_written"], d["rows_in_place"] = len(launches), sum(launches), in_place
    return d


# ---------------------------------------------------------------------------------------------- the launchers' grids
def interp_points_per_thread(half, n_cu):
    """launch_hal_round_evals: at most 4 workgroups of 256 threads per unit"""
    grid = min(-(-half // 256), 4 * n_cu)
    return -(-half // (256 * grid))


def rows_blocks_per_workgroup(half, n_jobs, n_cu):
    """launch_hal_rows: at most ceil(8 n_cu / n_jobs) workgroups of 256 threads per job"""
    blocks = -(-half // 256)
    grid = min(blocks, max(-(-8 * n_cu // n_jobs), 1))
    return -(-blocks // grid)


def strided_groups_per_workgroup(half, n_cu):
    """k_roundeval_mfma: groups of two 256-point tiles, at most 2 n_cu workgroups"""
    groups = -(-half // (2 * K_TP))
    return -(-groups // min(groups, 2 * n_cu))


def hal_tags(req, n_cu=NOMINAL_CU):
    """(route, branch tags) of the request on a device of n_cu compute units"""
    route = hal_route(req, n_cu)
    half = 1 << (req.n_vars - 1)
    l2h = req.order == L2H
    tags = set()
    coef, eqs = coef_declines(req), eq_set_declines(req, is_wide(req))
    first_eq = bool(req.evs and req.evs[0].eq)
    truncated = any(m[0] == "trunc" and not _is_full(req, m) for m in req.mls)
    if route == "coef":
        tags.add("coef:domain-points" if req.n_points else "coef:degree3-at-1-inf")
        if first_eq and req.n_points and not is_wide(req):
            tags.add("eq_set:refused:domain-point")
    elif not l2h and coef == "multilinear not full" and req.n_points and coef_declines(req._replace(mls=[FULL] * len(req.mls))) is None:
        tags.add("coef:declined:truncated")
    elif l2h and req.n_points and req.n_vars >= 2 and coef_declines(req._replace(order=H2L)) is None:
        tags.add("coef:declined:l2h")
    if route == "eq_set":
        tags.add("eq_set:wide" if is_wide(req) else "eq_set:narrow")
    elif first_eq and eqs == "multilinear not full" and eq_set_declines(req._replace(mls=[FULL] * len(req.mls)), is_wide(req)) is None:
        tags.add("eq_set:declined:truncated")
    if route == "in_parts":
        parts = {hal_route(p, n_cu) for p in deal_parts(req)}
        if len(parts) >= 2:
            tags.add("in_parts:routes>=2:" + ("l2h" if l2h else "h2l"))
        if not _on(req, "BN_HAL_EQ_SET") and eq_set_declines(req._replace(env={}), True) is None:
            tags.add("in_parts:eq-set-off")
    if route in ("monomials", "rows_batched", "rows_per_point", "interpreter"):
        if any(m[0] == "transparent" for m in req.mls):
            tags.add("transparent:" + ("mono" if route == "monomials" else "rows" if route != "interpreter" else "interp"))
        jobs = plan_monomials(req, n_cu)
        if route == "monomials":
            mixed = not first_eq and any(e.eq for e in req.evs)
            if req.n_vars == 2:
                tags.add("mono:n_vars=2")
            for v, eq, at_inf in jobs:
                if not v and not eq:
                    tags.add("mono:const")
                elif l2h:
                    tags.add("strided:" + {(2, False): "(1,1)", (1, False): "(1,0)ones", (1, True): "(1,0)eq", (0, True): "(0,0)"}[(len(v), bool(eq))])
                elif not eq and len(v) == 1:
                    tags.add(("mono:xor-sum:at-inf" if at_inf else "mono:xor-sum:at-1-only") if half >= XOR_SUM_MIN_HALF else "mono:lone-on-ones")
                    if half == XOR_SUM_MIN_HALF >> 1:
                        tags.add("mono:lone-below-xor-sum")
                elif eq and mixed:
                    tags.add("mono:eq+%d" % len(v))
                elif len(v) == 3:
                    tags.add("mono:three-factor")
            if l2h:
                if not mfma_applies(n_cu, half >> 1):
                    tags.add("strided:at-threshold")
                if strided_groups_per_workgroup(half, n_cu) >= 2:
                    tags.add("strided:groups>=2")
        else:
            lo, hi = point_range(req)
            if jobs == "more than 15 jobs":
                tags.add("mono:declined:16-jobs")
            if jobs == "more than 12 terms":
                tags.add("mono:declined:13-terms")
            if jobs == "factors" and l2h:
                tags.add("mono:declined:l2h-eq-factors")
            if jobs == "Low-to-High below the matrix-core threshold" and mfma_applies(n_cu, 2 * half) and lo >= 1 and hi <= 3:
                tags.add("mono:declined:below-mfma")
        if route == "interpreter":
            if req.n_vars == 1:
                tags.add("interp:n_vars=1")
            elif half < ROWS_FLOOR and _on(req, "BN_CIRCUIT_MULTIPASS"):
                tags.add("interp:below-rows-floor:" + ("l2h" if l2h else "h2l"))
            if interp_points_per_thread(half, n_cu) >= 2:
                tags.add("interp:grid-stride")
        elif route in ("rows_batched", "rows_per_point"):
            launches, in_place = rows_plan(req)
            if route == "rows_batched" and half == ROWS_FLOOR and truncated and any(e.eq for e in req.evs) and req.n_points:
                tags.add("rows:floor:" + ("l2h" if l2h else "h2l"))
            if len(launches) >= 2:
                tags.add("rows:second-flush")
            if l2h and any(rows_blocks_per_workgroup(half, n, n_cu) >= 2 for n in launches):
                tags.add("rows:l2h-grid-stride")
            if route == "rows_per_point":
                tags.add("rows:per-point:l2h" if l2h else "rows:per-point:truncated" if truncated else "rows:per-point:in-place")
    return route, frozenset(tags)


# ---------------------------------------------------------------------------------------------- the cases
HalCase = namedtuple("HalCase", "id order n_vars mls evs n_points env route tags")
FULL = ("full",)
SFX = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0


def cut(by, suffix=SFX):
    """a multilinear that stores all but the last `by` evaluations (resolved against the case's n_vars)"""
    return ("cut", by, suffix)


def _c(cid, order, n_vars, mls, evs, n_points, route, *tags, **env):
    return HalCase(cid, order, n_vars, list(mls), [Ev(*e) for e in evs], n_points, dict(env), route, frozenset(tags))


# sixteen distinct monomials over six multilinears, eight to an evaluator; thirteen in one composition
_PAIRS = [(a, b) for a in range(6) for b in range(a + 1, 6)]
SIXTEEN_A, SIXTEEN_B = P(*_PAIRS[:8]), P(*(_PAIRS[8:] + [(0,)]))
THIRTEEN = P(*_PAIRS[:13])
SEVENTEEN_SUMMANDS = P(*([(0,), (1,)] * 8 + [(0,)]))   # 9 a + 8 b = a, as seventeen summands: sum_plan gives up
# nine evaluators over four multilinears: wider than one pass carries
_WIDE8 = [(P((i % 4, (i + 1) % 4), ((i + 2) % 4,)), P((i % 4, (i + 1) % 4)), 1, 3) for i in range(8)]

HAL_CASES = [
    # ---- the interpreter kernel
    _c("interp-n1", H2L, 1, [FULL, FULL], [(AB_PLUS_A, AB, 1, 2, False)], 0, "interpreter", "interp:n_vars=1"),
    _c("interp-n10-h2l", H2L, 10, [FULL, cut(3), ("trunc", 0, SFX)], [(AB_PLUS_C, AB, 0, 6, False), (ABC_PLUS_A, ABC, 1, 5, True)], 3,
       "interpreter", "interp:below-rows-floor:h2l"),
    _c("interp-n10-l2h", L2H, 10, [FULL, cut(3), ("trunc", 0, SFX)], [(AB_PLUS_C, AB, 0, 6, False), (ABC_PLUS_A, ABC, 1, 5, True)], 3,
       "interpreter", "interp:below-rows-floor:l2h"),
    _c("interp-grid-stride", L2H, ("interp", 2), [FULL, FULL], [(AB_PLUS_A, AB, 1, 4, False)], 1, "interpreter", "interp:grid-stride", "coef:declined:l2h",
       BN_CIRCUIT_MULTIPASS="0"),
    # ---- rows + compiled circuits, the points side by side
    _c("rows-n11-h2l", H2L, 11, [FULL, cut(5), FULL], [(AB_PLUS_C, AB, 0, 4, False), (ABC_PLUS_A, ABC, 1, 4, True)], 1, "rows_batched", "rows:floor:h2l"),
    _c("rows-n11-l2h", L2H, 11, [FULL, cut(5), FULL], [(AB_PLUS_C, AB, 0, 4, False), (ABC_PLUS_A, ABC, 1, 4, True)], 1, "rows_batched", "rows:floor:l2h"),
    _c("rows-25", H2L, 11, [FULL] * 5, [(P((0, 1), (2, 3), (4,)), P((0, 1), (2, 3)), 0, 5, False)], 2, "rows_batched", "rows:second-flush"),
    _c("rows-l2h-grid", L2H, ("rows", 2), [FULL, FULL], [(AB_PLUS_A, AB, 0, 4, False)], 1, "rows_batched", "rows:l2h-grid-stride"),
    _c("rows-l2h-ab-eq", L2H, ("mfma", 1), [FULL, FULL], [(AB, AB, 1, 3, True)], 0, "rows_batched", "mono:declined:l2h-eq-factors"),
    # ---- rows + compiled circuits, point by point
    _c("perpoint-in-place", H2L, 21, [FULL] * 3, [(ABC_PLUS_A, ABC, 1, 4, False)], 1, "rows_per_point", "rows:per-point:in-place", BN_HAL_COEF="0"),
    _c("perpoint-truncated", H2L, 21, [FULL, cut(5), FULL], [(ABC_PLUS_A, ABC, 1, 4, False)], 1, "rows_per_point", "rows:per-point:truncated",
       "coef:declined:truncated"),
    _c("perpoint-l2h", L2H, 21, [FULL] * 3, [(ABC_PLUS_A, ABC, 1, 4, False)], 1, "rows_per_point", "rows:per-point:l2h", "rows:l2h-grid-stride",
       "coef:declined:l2h"),
    # ---- one pass per monomial, High-to-Low
    _c("mono-n2", H2L, 2, [FULL, FULL], [(AB, AB, 1, 3, False)], 0, "monomials", "mono:n_vars=2"),
    _c("mono-const", H2L, 5, [FULL, FULL], [(P((0, 1), K1), AB, 1, 3, False)], 0, "monomials", "mono:const"),
    _c("mono-lone-n18", H2L, 18, [FULL] * 3, [(AB_PLUS_C, AB, 1, 3, False), (P((2,)), P((2,)), 1, 3, False)], 0, "monomials", "mono:lone-on-ones",
       "mono:lone-below-xor-sum"),
    _c("mono-lone-n19", H2L, 19, [FULL] * 4, [(AB_PLUS_C, AB, 1, 3, False), (P((3,)), P((3,)), 1, 3, False)], 0, "monomials", "mono:xor-sum:at-1-only",
       "mono:xor-sum:at-inf"),
    _c("mono-abc", H2L, 9, [FULL] * 3, [(ABC, ABC, 1, 3, False)], 0, "monomials", "mono:three-factor", BN_HAL_COEF="0"),
    _c("mono-mixed-eq", H2L, 9, [FULL] * 3, [(AB, AB, 1, 3, False), (P((0, 1), (2,), K1), AB, 1, 3, True)], 0, "monomials", "mono:eq+2", "mono:eq+1", "mono:eq+0"),
    _c("mono-16-jobs", H2L, 11, [FULL] * 6, [(SIXTEEN_A, SIXTEEN_A, 1, 3, False), (SIXTEEN_B, SIXTEEN_B, 1, 3, False)], 0, "rows_batched", "mono:declined:16-jobs"),
    _c("mono-13-terms", H2L, 11, [FULL] * 6, [(THIRTEEN, THIRTEEN, 1, 3, False)], 0, "rows_batched", "mono:declined:13-terms"),
    # ---- one pass per monomial, Low-to-High: the strided matrix-core launch
    _c("strided-mfma1", L2H, ("mfma", 1), [FULL, FULL], [(AB, AB, 1, 3, False), (LIN_A, LIN_A, 1, 3, False), (P((0,), K2), LIN_A, 1, 3, True)], 0, "monomials",
       "strided:(1,1)", "strided:(1,0)ones", "strided:(1,0)eq", "strided:(0,0)", "strided:at-threshold"),
    _c("strided-mfma0", L2H, ("mfma", 0), [FULL, FULL], [(AB, AB, 1, 3, False), (LIN_A, LIN_A, 1, 3, False), (P((0,), K2), LIN_A, 1, 3, True)], 0, "rows_batched",
       "mono:declined:below-mfma"),
    _c("strided-groups2", L2H, ("groups", 2), [FULL, FULL], [(AB_PLUS_A, AB, 1, 3, False)], 0, "monomials", "strided:(1,1)", "strided:(1,0)ones", "strided:groups>=2"),
    # ---- a constraint set's two launches
    _c("eqset-narrow", H2L, 9, [FULL] * 3, [(AB_PLUS_C, AB, 1, 3, True), (P((2,), K1), P((2,)), 1, 2, True)], 0, "eq_set", "eq_set:narrow"),
    _c("eqset-truncated", H2L, 11, [FULL, cut(5), FULL], [(AB_PLUS_C, AB, 1, 3, True)], 0, "rows_batched", "eq_set:declined:truncated"),
    _c("eqset-domain-point", H2L, 9, [FULL] * 3, [(AB_PLUS_C, AB, 1, 4, True)], 1, "coef", "coef:domain-points", "eq_set:refused:domain-point"),
    _c("eqset-wide", H2L, 8, [FULL] * 4, [e + (True,) for e in _WIDE8] + [(P((0, 3), K1), P((0, 3)), 1, 3, True)], 0, "eq_set", "eq_set:wide"),
    _c("eqset-wide-off", H2L, 8, [FULL] * 4, [e + (True,) for e in _WIDE8] + [(P((0, 3), K1), P((0, 3)), 1, 3, True)], 0, "in_parts", "in_parts:eq-set-off",
       BN_HAL_EQ_SET="0"),
    # ---- a wide request dealt out
    _c("parts-h2l", H2L, 8, [FULL] * 4, [e + (False,) for e in _WIDE8] + [(ABC_PLUS_A, ABC, 0, 3, False)], 0, "in_parts", "in_parts:routes>=2:h2l"),
    _c("parts-l2h", L2H, 11, [FULL] * 4, [e + (False,) for e in _WIDE8] + [(SEVENTEEN_SUMMANDS, LIN_A, 0, 3, False)], 0, "in_parts", "in_parts:routes>=2:l2h"),
    # ---- the coefficient form
    _c("coef-z", H2L, 9, [FULL] * 3, [(ABC_PLUS_A, ABC, 1, 5, False)], 2, "coef", "coef:domain-points"),
    _c("coef-1-inf", H2L, 9, [FULL] * 3, [(ABC_PLUS_A, ABC, 1, 3, False)], 0, "coef", "coef:degree3-at-1-inf"),
    _c("coef-truncated", H2L, 11, [FULL, FULL, cut(1)], [(ABC_PLUS_A, ABC, 1, 4, False)], 1, "rows_batched", "coef:declined:truncated"),
    _c("coef-l2h", L2H, 11, [FULL] * 3, [(ABC_PLUS_A, ABC, 1, 4, False)], 1, "rows_batched", "coef:declined:l2h"),
    # ---- Transparent multilinears, partially evaluated into scratch first
    _c("transparent-mono", H2L, 10, [("transparent", 5, 2), FULL, FULL], [(AB_PLUS_C, AB, 1, 3, False)], 0, "monomials", "transparent:mono", "mono:lone-on-ones"),
    _c("transparent-rows", L2H, 11, [FULL, ("transparent", 3, 3), FULL], [(AB_PLUS_C, AB, 0, 4, False)], 1, "rows_batched", "transparent:rows"),
]
HAL_BY_ID = {c.id: c for c in HAL_CASES}
assert len(HAL_BY_ID) == len(HAL_CASES)

# every branch that the cases are there for (tests/test_oracle_hal_cases.py: each is claimed by a case)
HAL_REQUIRED_TAGS = [
    "interp:n_vars=1", "interp:below-rows-floor:h2l", "interp:below-rows-floor:l2h", "interp:grid-stride",
    "rows:floor:h2l", "rows:floor:l2h", "rows:second-flush", "rows:l2h-grid-stride", "mono:declined:l2h-eq-factors",
    "rows:per-point:in-place", "rows:per-point:truncated", "rows:per-point:l2h",
    "mono:n_vars=2", "mono:const", "mono:lone-on-ones", "mono:lone-below-xor-sum", "mono:xor-sum:at-1-only", "mono:xor-sum:at-inf", "mono:three-factor",
    "mono:eq+0", "mono:eq+1", "mono:eq+2", "mono:declined:16-jobs", "mono:declined:13-terms",
    "strided:(1,1)", "strided:(1,0)ones", "strided:(1,0)eq", "strided:(0,0)", "strided:at-threshold", "mono:declined:below-mfma", "strided:groups>=2",
    "eq_set:narrow", "eq_set:declined:truncated", "eq_set:refused:domain-point", "eq_set:wide", "in_parts:eq-set-off",
    "in_parts:routes>=2:h2l", "in_parts:routes>=2:l2h",
    "coef:domain-points", "coef:degree3-at-1-inf", "coef:declined:truncated", "coef:declined:l2h",
    "transparent:mono", "transparent:rows",
]


def n_vars_of(c, n_cu=NOMINAL_CU):
    """n_vars of case `c` on a device of n_cu compute units (the launchers' own formulas)."""
    if isinstance(c.n_vars, int):
        return c.n_vars
    rule, k = c.n_vars
    if rule == "mfma":
        n = next(v for v in range(2, 40) if mfma_applies(n_cu, 1 << (v - 1)))
        assert not mfma_applies(n_cu, 1 << (n - 2))
        return n if k else n - 1
    if rule == "groups":
        n = next(v for v in range(2, 40) if strided_groups_per_workgroup(1 << (v - 1), n_cu) >= k)
        assert mfma_applies(n_cu, 1 << (n - 1))
        return n
    if rule == "interp":
        return next(v for v in range(2, 40) if interp_points_per_thread(1 << (v - 1), n_cu) >= k)
    assert rule == "rows"
    for v in range(11, 40):
        launches, _ = rows_plan(request(c._replace(n_vars=v)))
        if any(rows_blocks_per_workgroup(1 << (v - 1), n, n_cu) >= k for n in launches):
            return v
    raise AssertionError(c.id)


def request(c, n_cu=NOMINAL_CU):
    """The case as the request the predicates read: n_vars resolved, the cut multilinears with their stored lengths."""
    n_vars = n_vars_of(c, n_cu)
    mls = [("trunc", (1 << n_vars) - m[1], m[2]) if m[0] == "cut" else m for m in c.mls]
    return Req(c.order, n_vars, mls, c.evs, c.n_points, c.env)


def moved(d):
    return {k: v for k, v in d.items() if v}


def request_of(order, n_vars, mls, evaluators, n_points, env=None):
    """The request of a test that has its operands in the oracle's form: mls ('folded', array, suffix) | ('transparent', array, level,
    n_vars_ml); evaluators: dicts {steps, steps_inf, start, end, eq: a token of the indicator's DEVICE array, or None}."""
    specs = []
    for m in mls:
        if m[0] == "transparent":
            specs.append(("transparent", m[2], m[3] - n_vars))
        else:
            specs.append(FULL if m[1].shape[0] >= 1 << n_vars else ("trunc", m[1].shape[0], m[2]))
    evs = [Ev([tuple(s) for s in e["steps"]], [tuple(s) for s in e["steps_inf"]], e["start"], e["end"], e["eq"]) for e in evaluators]
    return Req(order, n_vars, specs, evs, n_points, dict(env or {}))


# ---------------------------------------------------------------------------------------------- inputs and references
_cache = {}


def inputs(oracle, c, n_cu=NOMINAL_CU):
    """The operands of a case, SplitMix64 streams of the case's own seeds: (multilinears in the oracle's form, tensor query or None, indicator or
    None, domain points, evaluators in the oracle's form)."""
    req = request(c, n_cu)
    seed = 0x4A1C0000 + 64 * (HAL_CASES.index(HAL_BY_ID[c.id]) if c.id in HAL_BY_ID else 1000 + zlib.crc32(c.id.encode()) % 1000)   # (a variant of a row: its own id)
    n = 1 << req.n_vars
    mls, query = [], None
    q_vars = {m[2] for m in req.mls if m[0] == "transparent"}
    assert len(q_vars) <= 1
    for j, m in enumerate(req.mls):
        if m[0] == "transparent":
            n_ml = req.n_vars + m[2]
            mls.append(("transparent", oracle.random_b128(seed + j, (1 << n_ml) >> (7 - m[1])), m[1], n_ml))
        else:
            length = n if m[0] == "full" else m[1]
            mls.append(("folded", np.ascontiguousarray(oracle.random_b128(seed + j, n)[:length]), 0 if m[0] == "full" else m[2]))
    if q_vars:
        q = q_vars.pop()
        query = oracle.arr(1 << q)
        query[0, 0] = 1
        oracle.tensor_expand(query, 0, oracle.random_scalars(seed + 40, q))
    eq = oracle.random_b128(seed + 41, max(1, n // 2)) if any(e.eq for e in req.evs) else None
    points = oracle.random_scalars(seed + 42, req.n_points) if req.n_points else []
    evs = [{"steps": e.steps, "steps_inf": e.steps_inf, "start": e.start, "end": e.end, "eq_ind": eq if e.eq else None} for e in req.evs]
    return mls, query, eq, points, evs


def reference(oracle, c, n_cu=NOMINAL_CU):
    """oracle.hal_round_evals of the case's inputs: computed once per process."""
    key = (c.id, n_cu)
    if key not in _cache:
        mls, query, _eq, points, evs = inputs(oracle, c, n_cu)
        rc, want = oracle.hal_round_evals(c.order, request(c, n_cu).n_vars, query, mls, evs, points)
        assert rc == 0
        _cache[key] = want
    return _cache[key]
