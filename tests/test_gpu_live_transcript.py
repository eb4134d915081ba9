"""The `_live` entry points (include/binius_amd_host.h, "Against a live transcript") on the device: every compiled prover driven by a
transcript whose samples depend on everything written so far (tests/transcript_ref.py), at the smallest shapes its array form's own
GPU test uses.  Per entry point:

  fixed point   the samples S the live run drew, fed to the ARRAY form on fresh copies of the inputs, give bit-equal outputs; the
                message bytes the transcript saw are the array outputs arranged in the documented writing order (truncated round
                polynomials, digests as raw bytes)
  oracle        the Python restatement the array form's test uses, fed S, gives the same outputs (hence the same bytes)
  schedule      the alternation of writes (with byte counts) and draws (with counts) equals a schedule computed here from the shapes
                alone, written from the reference lines the header cites -- never read back from the library
  verifier      bnh_fri_prove_live, bnh_piop_prove_committed_open_live: the restated verifiers read the recorded bytes, draw from a
                fresh challenger at their own points and accept; one flipped byte in any message segment makes them reject

and, on the batch sumcheck: a slow caller changes nothing; a callback that fails ends the call with BN_ERR_CALLBACK (or with the
Python exception it raised) and leaves the context usable."""
import numpy as np
import pytest

import transcript_ref as T

pytestmark = pytest.mark.gpu
M, D = T.MESSAGE, T.DECOMMITMENT


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, 1 << 22)
    yield ctx
    ctx.close()


def challenger(**kw):
    from binius_amd._host import Transcript

    return T.make_challenger(Transcript)(**kw)


def live_then_array(schedule, run, messages, decommitment=None):
    """run(roles) -> outputs, on fresh copies of the inputs: once under the challenger (roles: zeros of the right lengths, which the
    _live form does not read), once through the array form with the samples the challenger served.  Checks the schedule, the fixed
    point and the bytes; returns (challenger, roles, outputs)."""
    ch = challenger()
    with ch.proving():
        live = run(T.zero_roles(schedule))
    assert T.merged(ch.log) == T.merged(schedule), "the alternation of writes and draws is not the schedule"
    roles = T.roles_of(schedule, ch.drawn)
    array = run(roles) if not ch.drawn_bits else run(roles, ch.drawn_bits)
    assert same(live, array), "the _live form and the array form fed its samples differ"
    assert bytes(ch.written[M]) == messages(array), "the message bytes are not the array outputs in writing order"
    if decommitment is not None:
        assert bytes(ch.written[D]) == decommitment(array)
    return ch, roles, array


def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a if not str(k).endswith("_ms"))
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def flat(rows):
    return [x for row in rows for x in row]


def batch_run_schedule(provers, coeffs_per_round=2, role="ch"):
    """front_loaded::BatchProver::run (front_loaded.rs:122-197) over provers [(n_vars, m)] ascending: per round the evaluations of the
    provers whose n_vars is the round (m scalars each), the truncated round polynomial, one sample; then the last provers' evaluations"""
    sched, rounds = [], max([v for v, _ in provers] + [0])
    for r in range(rounds):
        sched += [("w", M, 16 * m) for v, m in provers if v == r]
        sched += [("w", M, 16 * coeffs_per_round), ("s", role, 1)]
    return sched + [("w", M, 16 * m) for v, m in provers if v == rounds]


def batch_run_messages(provers, round_proofs, final_evals, keep=2):
    """the same order over the array outputs: round_proofs[r][:keep], final_evals[p] of prover p = (n_vars, m)"""
    out, rounds = [], max([v for v, _ in provers] + [0])
    for r in range(rounds):
        out += [T.scalars(final_evals[p]) for p, (v, _) in enumerate(provers) if v == r]
        out.append(T.scalars(round_proofs[r][:keep]))
    out += [T.scalars(final_evals[p]) for p, (v, _) in enumerate(provers) if v == rounds]
    return b"".join(out)


# ---------------------------------------------------------------------------------------------- batch sumcheck
def batch_case(oracle, sizes, ks, seed):
    import test_gpu_group as G

    provers = G.batch_instance(oracle, sizes, ks, seed)
    shape = [(v, len(mls)) for v, mls, _, _ in provers]
    schedule = [("s", "bc", len(provers))] + batch_run_schedule(shape)

    def run_on(hal, roles):
        from binius_amd._host import BatchSumcheckPlan

        alloc = hal.dev_alloc()
        dev = [(v, [G.upload(hal, alloc, x) for x in mls], comps, sums) for v, mls, comps, sums in provers]
        plan = BatchSumcheckPlan(hal, dev, alloc.alloc(sum(len(mls) << v for v, mls, _, _ in provers) // 2 + 64), roles["bc"], roles["ch"])
        plan.run()
        return plan.round_proofs(), plan.final_evals()

    def oracle_items(roles):
        from oracle import piop_ref

        ref = [dict(n_vars=v, multilins=[x.copy() for x in mls], comps=comps, sums=sums) for v, mls, comps, sums in provers]
        return piop_ref.batch_sumcheck_prove(ref, roles["bc"], roles["ch"])

    return shape, schedule, run_on, oracle_items


def test_batch_sumcheck(oracle, hal):
    """three provers of 2, 3 and 5 variables (front_loaded.rs:51-59, 175-197)"""
    shape, schedule, run_on, oracle_items = batch_case(oracle, [2, 3, 5], [1, 2, 1], 0x11FE0000)
    assert T.merged(schedule)[:3] == [("s", 3), ("w", M, 32), ("s", 1)] and len([e for e in schedule if e[0] == "s"]) == 6
    ch, roles, (proofs, evals) = live_then_array(schedule, lambda roles: run_on(hal, roles), lambda out: batch_run_messages(shape, out[0], out[1]))
    items, want_evals = oracle_items(roles)
    assert evals == want_evals and proofs == [list(p) for k, p in items if k == "round_proof"]
    assert bytes(ch.written[M]) == b"".join(T.scalars(p) for _k, p in items), "the oracle's transcript, item by item"


def test_slow_caller_and_aborting_callbacks(oracle, hal):
    """One prover of 16 variables, so that rounds are armed ahead of the challenge: a sample that takes 20 ms in a middle round
    changes no byte; a sample that fails in a middle round ends the call with BN_ERR_CALLBACK, a Python exception in a callback comes
    out as that exception, and a complete proof on the same context afterwards is the oracle's."""
    from binius_amd import BnError
    from binius_amd._ffi import BN_ERR_CALLBACK
    from binius_amd._host import TranscriptAbort

    shape, schedule, run_on, oracle_items = batch_case(oracle, [16], [1], 0x11FE1000)
    before = hal.arm_counters()
    ch, roles, (proofs, evals) = live_then_array(schedule, lambda roles: run_on(hal, roles), lambda out: batch_run_messages(shape, out[0], out[1]))
    slow = challenger(slow_at=8)  # (call 0 draws the batch coefficient: call 8 is round 7's challenge)
    with slow.proving():
        assert run_on(hal, T.zero_roles(schedule)) == (proofs, evals)
    assert slow.drawn == ch.drawn and slow.written == ch.written and slow.sample_calls == 17
    after = hal.arm_counters()
    print("armed rounds over three proofs, one of them with a 20 ms sample: %r" % {k: after[k] - before[k] for k in ("hits", "cancels", "expired", "hosted", "two_round")})

    failing = challenger(fail_at=8, fail_with=TranscriptAbort())
    with pytest.raises(BnError) as e:
        with failing.proving():
            run_on(hal, T.zero_roles(schedule))
    assert e.value.code == BN_ERR_CALLBACK and e.value.kind == "Callback"
    assert failing.drawn == ch.drawn[:8] and bytes(failing.written[M]) == bytes(ch.written[M])[: 8 * 32], "the proof went on after the failed sample"
    raising = challenger(fail_at=8, fail_with=KeyError("the caller's own error"))
    with pytest.raises(KeyError, match="the caller's own error"):
        with raising.proving():
            run_on(hal, T.zero_roles(schedule))
    again = challenger()
    with again.proving():
        assert run_on(hal, T.zero_roles(schedule)) == (proofs, evals)
    assert again.written == ch.written
    items, want_evals = oracle_items(roles)
    assert evals == want_evals and bytes(again.written[M]) == b"".join(T.scalars(p) for _k, p in items)


# ---------------------------------------------------------------------------------------------- eq-ind sumcheck
def test_eqind_sumcheck(oracle, hal):
    """the keccak constraints over 4 variables (eq_ind.rs:378-644 as a front-loaded batch of one): what is written is the prover's
    polynomial times the batch coefficient without its last coefficient; the arrays keep the prover's own four coefficients"""
    from binius_amd._host import EqIndPlan
    from oracle import zerocheck_ref
    from test_gpu_hal_wide import keccak_constraints

    n_vars = 4
    n_mls, comps = keccak_constraints(3)
    mls = [oracle.random_b128(0x11FE2000 + j, 1 << n_vars) for j in range(n_mls)]
    stream = oracle.random_scalars(0x11FE2100, n_vars + len(comps))
    eqc, sums = stream[:n_vars], stream[n_vars:]
    schedule = [("s", "bc", 1)] + [e for _ in range(n_vars) for e in (("w", M, 16 * 3), ("s", "ch", 1))] + [("w", M, 16 * (n_mls + 1))]

    def run(roles):
        alloc = hal.dev_alloc()
        d = []
        for x in mls:
            d.append(alloc.alloc(x.shape[0]))
            hal.copy_h2d(x, d[-1])
        plan = EqIndPlan(hal, n_vars, d, comps, sums, eqc, alloc.alloc(64 + (1 << n_vars)), roles["bc"][0], roles["ch"])
        plan.run()
        return plan.round_coeffs(), plan.final_evals()

    ch = challenger()
    with ch.proving():
        live = run(T.zero_roles(schedule))
    assert T.merged(ch.log) == T.merged(schedule)
    roles = T.roles_of(schedule, ch.drawn)
    array = run(roles)
    assert live == array and all(len(rc) == 4 for rc in array[0])
    written = b"".join(T.scalars([oracle.mul(roles["bc"][0], c) for c in rc[:-1]]) for rc in array[0]) + T.scalars(array[1])
    assert bytes(ch.written[M]) == written
    want = zerocheck_ref.eqind_sumcheck_prove(mls, n_vars, comps, sums, eqc, roles["bc"][0], roles["ch"], None)
    assert [list(r) for r in want[0]] == [list(r) for r in array[0]] and list(want[1]) == list(array[1])


# ---------------------------------------------------------------------------------------------- univariate-skip zerocheck
def test_zerocheck_batch_tower(oracle, hal):
    """tables of 2, 5 and 6 variables with k = 3 (constraint_system/prove.rs:470; batch_zerocheck.rs:193-272): the first table is
    padded to k and finishes before round 0"""
    import zerocheck_skip_ref as R
    from binius_amd._host import ZerocheckBatchPlan
    from test_gpu_zerocheck_skip import CASES, device_tables

    k, _sat, make = CASES["tiny_bit_columns_at_3"]
    tables = make()
    n = [t["n_vars"] for t in tables]
    cols = [len(t["cols"]) for t in tables]
    deg = [max([2] + [c[2] for c in t["comps"]]) for t in tables]
    nr = [max(v, k) - k for v in n]
    rounds, D = max(nr), max(max(c[2] for c in t["comps"]) for t in tables) << k
    schedule = [("s", "zc", rounds), ("s", "bc", len(tables)), ("w", M, 16 * (D - (1 << k))), ("s", "uni", 1)]
    for r in range(rounds):
        schedule += [("w", M, 16 * (cols[p] + 1)) for p in range(len(tables)) if nr[p] == r]
        schedule += [("w", M, 16 * (max(deg[p] for p in range(len(tables)) if nr[p] > r) + 1)), ("s", "sc", 1)]
    schedule += [("w", M, 16 * (cols[p] + 1)) for p in range(len(tables)) if nr[p] == rounds]
    schedule += [("s", "rbc", 1)] + [e for _ in range(k) for e in (("w", M, 32), ("s", "rch", 1))] + [("w", M, 16 * (sum(cols) + 1))]

    def args(roles):
        return roles.get("zc", []), roles["bc"], roles["uni"][0], roles.get("sc", []), roles["rbc"][0], roles["rch"]

    def run(roles):
        alloc = hal.dev_alloc()
        d_tables = device_tables(hal, alloc, tables)
        return ZerocheckBatchPlan(hal, d_tables, k, *args(roles), alloc.alloc(ZerocheckBatchPlan.scratch_elems(d_tables, k, tower=True)), tower=True).run()

    def messages(out):
        parts = [T.scalars(out["message"])]
        for r in range(rounds):
            parts += [T.scalars(out["final_evals"][p]) for p in range(len(tables)) if nr[p] == r]
            parts.append(T.scalars(out["round_coeffs"][r][: max(deg[p] for p in range(len(tables)) if nr[p] > r) + 1]))
        parts += [T.scalars(out["final_evals"][p]) for p in range(len(tables)) if nr[p] == rounds]
        parts += [T.scalars(rc[:2]) for rc in out["reduction_round_coeffs"]]
        return b"".join(parts) + T.scalars(out["reduction_final_evals"])

    _ch, roles, out = live_then_array(schedule, run, messages)
    want = R.prove(tables, k, *args(roles))
    for key in ("message", "round_coeffs", "final_evals", "reduction_round_coeffs", "reduction_final_evals", "skipped_challenges", "unskipped_challenges",
                "concat_multilinear_evals"):
        assert out[key] == want[key], key


# ---------------------------------------------------------------------------------------------- GKR grand product
def gpa_schedule(n_vars):
    """gkr_gpa/prove.rs:67-126: step j -- the batch coefficient, j rounds of three coefficients and a challenge, the 2 * active layer
    evaluations and the indicator's, then the layer challenge"""
    sched = []
    for j in range(max(n_vars + [0])):
        active = len([n for n in n_vars if n > j])
        sched += [("s", "gpa_bc", 1)] + [e for r in range(j) for e in (("w", M, 48), ("s", ("gpa_sc", j), 1))]
        sched += [("w", M, 16 * (2 * active + 1)), ("s", "gpa_gc", 1)]
    return sched


def gpa_samples(roles, m):
    return roles.get("gpa_bc", []), [roles.get(("gpa_sc", j), []) for j in range(m)], roles.get("gpa_gc", [])


def gpa_messages(out):
    return b"".join(T.scalars(flat(out["round_proofs"][j])) + T.scalars(out["layer_evals"][j]) for j in range(len(out["layer_evals"])))


def test_gkr_gpa(oracle, hal):
    """trees of 0, 1 and 4 variables, one of them truncated"""
    import gkr_gpa_ref as R
    import test_gpu_gkr_gpa as G

    shapes = [(4, 11), (0, 1), (1, 2), (4, 16)]
    n_vars = [n for n, _ in shapes]
    inputs = [oracle.random_b128(0x11FE3000 + 17 * t, ln) for t, (_, ln) in enumerate(shapes)]
    schedule = gpa_schedule(n_vars)
    _ch, roles, out = live_then_array(schedule, lambda roles: G.run_prover(hal, shapes, inputs, *gpa_samples(roles, 4)), gpa_messages)
    bc, sc, gc = gpa_samples(roles, 4)
    G.assert_same_proof(out, R.gpa_prove(inputs, n_vars, bc, sc, gc))
    R.gpa_verify(n_vars, out["products"], out, bc, sc, gc)


# ---------------------------------------------------------------------------------------------- GKR exponentiation
def test_gkr_exp(oracle, hal):
    """the mixed batch of the array form's test (batch_prove.rs:101 = sumcheck::batch_prove, batch_sumcheck.rs:138-187): provers join
    in the round that equals their size and draw their coefficient there; the zero-variable prover draws its own after the rounds"""
    import gkr_exp_ref as R
    import test_gpu_gkr_exp as G

    claims = G.make_claims(oracle, G.MIXED, 0x11FE4000)
    k, max_w, max_n = len(claims), max(w for _, w, _ in G.MIXED), max(n for n, _, _ in G.MIXED)
    schedule, layers = [], []
    for L in range(max_w):
        # the provers still active, grouped by size (claims of one size share their point, and keep sharing it layer after layer); a
        # group is a sumcheck prover when one of its members has multilinears: (n_vars, composition degree, multilinears + 1)
        groups = []
        for n in sorted({n for n, w, _ in G.MIXED if w > L}, reverse=True):
            members = [(w, kind) for nn, w, kind in G.MIXED if nn == n and w > L]
            n_mls = [(2 if w - 1 == L else 3) if kind == "dynamic" else (0 if w - 1 == L else 2) for w, kind in members]
            if sum(n_mls):
                groups.append((n, max(4 if kind == "dynamic" and w - 1 > L else 2 for (w, kind), m in zip(members, n_mls) if m), sum(n_mls) + 1))
        layers.append(groups)
        rounds = groups[0][0] if groups else 0
        for r in range(rounds):
            schedule += [("s", ("bc", L), len([g for g in groups if g[0] == rounds - r]))]
            schedule += [("w", M, 16 * (max(d for n, d, _ in groups if n >= rounds - r) + 1)), ("s", ("ch", L), 1)]
        schedule += [("s", ("bc", L), len([g for g in groups if g[0] == 0 and rounds > 0 or rounds == 0]))]
        schedule += [("w", M, 16 * m) for _n, _d, m in groups]

    def samples(roles):
        pad = lambda v, n: list(v) + [0] * (n - len(v))  # noqa: E731 -- the array form reads [L * n_claims + g] and [L * max_n + r]
        return [pad(roles.get(("bc", L), []), k) for L in range(max_w)], [pad(roles.get(("ch", L), []), max_n) for L in range(max_w)]

    def messages(out):
        return b"".join(T.scalars(flat(out["round_proofs"][L])) + T.scalars(flat(out["multilinear_evals"][L])) for L in range(max_w))

    _ch, roles, out = live_then_array(schedule, lambda roles: G.run_prover(hal, claims, *samples(roles)), messages)
    coeffs, chals = samples(roles)
    G.assert_same_proof(out, R.exp_prove(claims, coeffs, chals))
    assert R.exp_verify(G.meta_of(claims), out, coeffs, chals) == out["layer_claims"]


# ---------------------------------------------------------------------------------------------- flush product check
def test_flush_prodcheck(oracle, hal):
    """the two-table system of the array form's test (constraint_system/prove.rs:309-425)"""
    import test_gpu_flush as G

    flushes, nonzero = G.two_table_system()
    nf, nz, n_channels = len(flushes), len(nonzero), 1 + max(fl["channel"] for fl in flushes)
    n_vars = [fl["n_vars"] for fl in flushes] + [z[3] for z in nonzero]
    # the MLE-checks: the flushes with selectors, grouped by size in order of first appearance (flushes of one size leave the
    # grand-product argument with one point); m: the distinct oracle ids of the group
    groups = []
    for fl in flushes:
        if fl["selectors"]:
            if fl["n_vars"] not in [g["n"] for g in groups]:
                groups.append({"n": fl["n_vars"], "ids": set(), "sel": 0})
            g = [g for g in groups if g["n"] == fl["n_vars"]][0]
            g["ids"] |= {i for i, _ in fl["selectors"]} | {e[1] for e in fl["entries"] if e[0] == "oracle"}
            g["sel"] = max(g["sel"], len(fl["selectors"]))
    schedule = [("w", M, 16 * nz), ("s", "mix", 1), ("s", "perm", n_channels), ("w", M, 16 * nf)] + gpa_schedule(n_vars)
    for i, g in enumerate(groups):
        per_round = max(2, g["sel"] + 1) + 1
        schedule += [("s", "rbc", 1)] + [e for _ in range(g["n"]) for e in (("w", M, 16 * per_round), ("s", ("rch", i), 1))] + [("w", M, 16 * (len(g["ids"]) + 1))]

    def samples(roles):
        bc, sc, gc = gpa_samples(roles, max(n_vars))
        return {"mixing_challenge": roles["mix"][0], "permutation_challenges": roles["perm"], "gpa_batch_coeffs": bc, "gpa_sumcheck_challenges": sc, "gpa_challenges": gc,
                "red_batch_coeffs": roles.get("rbc", []), "red_challenges": [roles.get(("rch", i), []) for i in range(len(groups))]}

    def messages(out):
        parts = [T.scalars(out["gpa"]["products"][nf:]), T.scalars(out["gpa"]["products"][:nf]), gpa_messages(out["gpa"])]
        parts += [T.scalars(flat(c["round_proofs"])) + T.scalars(c["final_evals"]) for c in out["checks"]]
        return b"".join(parts)

    _ch, roles, out = live_then_array(schedule, lambda roles: G.run_prover(hal, flushes, nonzero, samples(roles)), messages)
    G.assert_same_transcript(out, G.restated(flushes, nonzero, samples(roles)))


def test_flush_prodcheck_without_flushes_still_draws(hal):
    """No flush and no non-zero oracle: the reference still writes its empty product slices and draws the mixing challenge and the
    channel_count permutation challenges (constraint_system/prove.rs:318-330), so the live form draws them -- and launches nothing --
    or the caller's challenger would fall behind the verifier's.  The array form has nothing to keep in step and returns at once."""
    import ctypes as C

    from binius_amd._host import host_lib

    L = host_lib()
    n_channels = 3
    ch = challenger()
    fn = L.bnh_flush_prodcheck_prove_live
    assert len(fn.argtypes) == 36
    args = [None if t is not C.c_uint32 and t is not C.c_uint64 else 0 for t in fn.argtypes]
    n_checks, n_linear = C.c_uint32(7), C.c_uint32(7)
    args[0], args[18], args[21], args[28], args[33] = hal._h, n_channels, ch.table(), C.pointer(n_checks), C.pointer(n_linear)
    assert fn(*args) == 0, L.bnh_last_error().decode()
    assert (n_checks.value, n_linear.value) == (0, 0)
    assert T.merged(ch.log) == T.merged([("w", M, 0), ("s", "mix", 1), ("s", "perm", n_channels), ("w", M, 0)]) == [("s", 1 + n_channels)]
    want = T.Hasher()
    assert ch.drawn == [want.sample() for _ in range(1 + n_channels)] and not ch.written[M] and not ch.written[D]
    array = L.bnh_flush_prodcheck_prove
    args = [None if t is not C.c_uint32 and t is not C.c_uint64 else 0 for t in array.argtypes]
    args[0] = hal._h
    assert array(*args) == 0


# ---------------------------------------------------------------------------------------------- evalcheck
def test_evalcheck_bivariate_lc(oracle, hal):
    """two provers of 3 and 6 variables: projections, linear combinations, a shift indicator and a tower basis (subclaims.rs:549-586)"""
    import adversarial as A
    import evalcheck_lincomb_ref as L
    import evalcheck_ref as R
    from binius_amd._host import EvalcheckPlan
    from test_gpu_evalcheck_lincomb import random_column

    pool = oracle.random_scalars(0x11FE5000, 36)
    state = [random_column(0x11FE5100 + t, 0, 16) for t in range(10)]
    c64 = [random_column(0x11FE5200 + t, 6, 10) for t in range(2)]
    c = [[(state[5 * y + x], 0, 1) for y in range(2)] for x in range(2)]
    packed, comps_p = [("basis", 6, 0)], []
    for x in range(2):
        comps_p.append((len(packed), 0))
        packed.append(("lincomb", c[x], 0, 16, 16, 10))
    comps_p.append((len(packed), 0))
    packed.append(("proj", state[7], 0, 16, 16, 10))
    right, comps_r = [("shift", 3, 1, R.LOGICAL_RIGHT, 26, 3)], []
    for col in c64:
        comps_r.append((len(right), 0))
        right.append(("proj", col, 6, 10, 29, 7))
    provers = [(3, right, comps_r, None), (6, packed, comps_p, None)]
    tables = L.resolve(provers, pool)
    provers = [(b, mls, comps, R.claim_sums(tabs, comps)) for (b, mls, comps, _), tabs in zip(provers, tables)]
    shape = [(b, len(mls)) for b, mls, _, _ in provers]
    schedule = [("s", "bc", len(provers))] + batch_run_schedule(shape)

    def run(roles):
        alloc = hal.dev_alloc()
        placed = {}

        def put(col):
            if id(col) not in placed:
                placed[id(col)] = A.place(hal, alloc, col, 1 + 2 * len(placed))[0]
            return placed[id(col)]

        dev = []
        for b, mls, comps, sums in provers:
            dmls = [("proj", put(ml[1])) + tuple(ml[2:]) if ml[0] == "proj" else
                    ("lincomb", [(put(col), level, coeff) for col, level, coeff in ml[1]]) + tuple(ml[2:]) if ml[0] == "lincomb" else ml for ml in mls]
            dev.append((b, dmls, comps, sums))
        plan = EvalcheckPlan(hal, dev, pool, alloc.alloc(EvalcheckPlan.scratch_elems(dev)), roles["bc"], roles["ch"])
        plan.run()
        return plan.round_proofs(), plan.final_evals()

    _ch, roles, (proofs, evals) = live_then_array(schedule, run, lambda out: batch_run_messages(shape, out[0], out[1]))
    want_proofs, want_evals = L.prove(provers, pool, roles["bc"], roles["ch"], tables=tables)
    assert proofs == want_proofs and evals == want_evals
    assert L.verify(provers, pool, roles["bc"], roles["ch"], proofs, evals)


# ---------------------------------------------------------------------------------------------- ring switch
def test_ring_switch(oracle, hal):
    """seven claims over four tower levels (ring_switch/prove.rs:68-104): the mixed tensor elements go out between the two draws"""
    import ring_switch_ref as R
    from binius_amd._host import RingSwitchPlan

    case = R.seven_claim_case()
    kappas = [kp for _off, kp in case["prefixes"]]
    n_claims = len(case["claims"])
    max_kappa = max(case["suffixes"][cl[1]][2] for cl in case["claims"])
    schedule = [("s", "mix", (n_claims - 1).bit_length()), ("w", M, 16 * sum(1 << kp for kp in kappas)), ("s", "row", max_kappa), ("w", M, 16 * n_claims)]
    assert len(case["mixing"]) == 3 and len(case["row"]) == max_kappa

    def run(roles):
        alloc = hal.dev_alloc()
        cols = []
        for arr, level, n_vars in case["columns"]:
            cols.append((alloc.alloc(arr.shape[0]), level, n_vars))
            hal.copy_h2d(arr, cols[-1][0])
        scratch = alloc.alloc(RingSwitchPlan.scratch_elems(case["suffixes"], case["claims"]))
        plan = RingSwitchPlan(hal, cols, case["pool"], case["suffixes"], kappas, case["claims"], scratch, roles["mix"], roles["row"])
        plan.run()
        return {"mixed": plan.mixed_tensor_elems(), "row_batched_evals": plan.row_batched_evals(), "transparents": [hal.copy_d2h(t) for t in plan.transparents()]}

    _ch, roles, out = live_then_array(schedule, run, lambda out: T.scalars(flat(out["mixed"])) + T.scalars(out["row_batched_evals"]))
    want = R.prove(dict(case, mixing=roles["mix"], row=roles["row"]))
    assert out["mixed"] == want["mixed"] and out["row_batched_evals"] == want["row_batched_evals"]
    assert all(np.array_equal(a, b) for a, b in zip(out["transparents"], want["transparents"]))


# ---------------------------------------------------------------------------------------------- FRI
def fri_schedule(p, role="ch"):
    """per fold round a challenge, then the round's commitment when the folder commits in it (fri/prove.rs:307-432); finish_proof
    (:483-507): the terminate codeword (decommitment), the indices, the layers and the openings (decommitment)"""
    commit_rounds, at = set(), 0
    for arity in p.fold_arities:
        at += arity
        commit_rounds.add(at)
    rounds = [[("s", role, 1)] + ([("w", M, 32)] if r + 1 in commit_rounds else []) for r in range(p.n_fold_rounds())]
    tail = [("w", D, 16 * p.terminate_len()), ("b", p.n_test_queries), ("w", D, 16 * (p.layout()[2] - p.terminate_len()))]
    return rounds, tail


def flipped(data, at):
    out = bytearray(data)
    out[at] ^= 0x10
    return bytes(out)


def segment_starts(schedule):
    """the offset of every MESSAGE write segment in the concatenated message bytes"""
    out, at = [], 0
    for e in T.merged([x for x in schedule if x[0] != "w" or x[1] == M]):
        if e[0] == "w":
            out.append(at)
            at += e[2]
    return out


def test_fri_prove(oracle, hal):
    """log_dim 6, log_inv_rate 1, batch 2, arities (3, 2, 1), three queries: the verifier of tests/fri_verify_ref.py on the recorded bytes"""
    import fri_verify_ref as fv
    from binius_amd._host import FRIParams, FriProvePlan

    p = fv.SHAPES[0][0]
    message = fv.case(oracle, p)[0]
    rounds, tail = fri_schedule(p)
    schedule = [("w", M, 32)] + flat(rounds) + tail

    def run(roles, idx=None):
        alloc = hal.dev_alloc()
        d_msg = alloc.alloc(message.shape[0])
        hal.copy_h2d(message, d_msg)
        plan = FriProvePlan(hal, FRIParams(p.log_dim, p.log_inv_rate, p.log_batch_size, list(p.fold_arities), p.n_test_queries), d_msg,
                            alloc.alloc(4 << (p.log_dim + p.log_batch_size + p.log_inv_rate)), roles["ch"], idx if idx is not None else [0] * p.n_test_queries)
        plan.run()
        return {"roots": plan.roots.copy(), "advice": np.array(plan.advice)}

    ch, roles, out = live_then_array(schedule, run, lambda out: out["roots"].tobytes(), lambda out: out["advice"].tobytes())
    pr = fv.prove(oracle, p, message, roles["ch"], ch.drawn_bits)
    assert [bytes(r) for r in out["roots"]] == pr.commitments and np.array_equal(out["advice"], pr.advice)

    def verifier(msg, dec):
        drawn, idx = T.replay(schedule, msg, bits=p.index_bits())
        roots = [msg[i : i + 32] for i in range(0, len(msg), 32)]
        return fv.verify(oracle, p, roots[0], roots[1:], drawn["ch"], idx, np.frombuffer(dec, dtype=np.uint64).reshape(-1, 2))

    msg, dec = bytes(ch.written[M]), bytes(ch.written[D])
    verifier(msg, dec)
    for at in segment_starts(schedule):
        with pytest.raises(fv.FriVerifyError):
            verifier(flipped(msg, at + 5), dec)


def test_fri_prove_with_a_short_advice_buffer_writes_nothing(oracle, hal):
    """An advice buffer one element short is rejected before the transcript has seen a byte or served a sample."""
    import fri_verify_ref as fv
    from binius_amd import BnError
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION
    from binius_amd._host import FRIParams, FriProvePlan

    p = fv.SHAPES[0][0]
    message = fv.case(oracle, p)[0]
    alloc = hal.dev_alloc()
    d_msg = alloc.alloc(message.shape[0])
    hal.copy_h2d(message, d_msg)
    plan = FriProvePlan(hal, FRIParams(p.log_dim, p.log_inv_rate, p.log_batch_size, list(p.fold_arities), p.n_test_queries), d_msg,
                        alloc.alloc(4 << (p.log_dim + p.log_batch_size + p.log_inv_rate)), [0] * p.n_fold_rounds(), [0] * p.n_test_queries, max_advice_elems=p.layout()[2] - 1)
    ch = challenger()
    with pytest.raises(BnError) as e:
        ch.prove(plan)
    assert e.value.code == BN_ERR_INPUT_VALIDATION and ch.log == []


# ---------------------------------------------------------------------------------------------- the PIOP
def test_piop_prove_committed_open(oracle):
    """committed multilinears of 6, 6, 8 and 9 variables (piop/prove.rs:306-395 ending in FRIFolder::finish_proof): piop::verify
    restated (tests/piop_verify.py, tests/fri_verify_ref.py) on the recorded bytes"""
    import binius_amd
    import fri_verify_ref as fv
    from binius_amd._host import FRIParams, PiopCommit, PiopCommittedOpenPlan, piop_commit_elems
    from oracle import piop_ref
    from piop_verify import make_instance, optimal_params, piecewise, verify_transcript

    n_varss = [6, 6, 8, 9]
    meta = piop_ref.CommitMeta.with_vars(n_varss)
    op = optimal_params(meta.total_vars, 1)
    p = fv.Params(op.log_dim, op.log_inv_rate, op.log_batch_size, tuple(op.fold_arities), op.n_test_queries)
    hp = FRIParams(p.log_dim, p.log_inv_rate, p.log_batch_size, list(p.fold_arities), p.n_test_queries)
    committed, transparents, claims = make_instance(oracle, n_varss, 1, 0x11FE6000)
    t_sizes = [t.shape[0].bit_length() - 1 for t in transparents]
    sizes = sorted(set(n_varss))
    # one prover per size: its committed multilinears, then its transparents
    provers = [(v, n_varss.count(v) + t_sizes.count(v)) for v in sizes]
    rounds, tail = fri_schedule(p)
    schedule, kinds = [("s", "bc", len(sizes))], []  # kinds: what every MESSAGE write of the schedule is, in order

    def writes(kind, n_bytes):
        schedule.append(("w", M, n_bytes))
        kinds.append((kind, n_bytes))

    for r in range(meta.total_vars):
        for v, m in provers:
            if v == r:
                writes("multilinear_evals", 16 * m)
        writes("round_proof", 32 if [v for v, _ in provers if v > r] else 0)  # (no prover left: the batched polynomial has no coefficient)
        schedule.append(rounds[r][0])
        if len(rounds[r]) > 1:
            writes("fri_commitment", 32)
    for v, m in provers:
        if v == meta.total_vars:
            writes("multilinear_evals", 16 * m)
    schedule += tail
    code_elems, tree_elems = piop_commit_elems(hp)
    ml_elems = sum(x.shape[0] for x in committed) + sum(x.shape[0] for x in transparents)

    with binius_amd.Context(0, code_elems + tree_elems + 2 * ml_elems + 4 * code_elems + (1 << 16)) as hal:
        alloc = hal.dev_alloc()

        def up(x):
            d = alloc.alloc(x.shape[0])
            hal.copy_h2d(x, d)
            return d

        d_c = [(v, up(x)) for v, x in zip(n_varss, committed)]
        d_t = [(v, up(x)) for v, x in zip(t_sizes, transparents)]
        codeword, tree = alloc.alloc(code_elems), alloc.alloc(tree_elems)
        scratch = alloc.alloc(3 * code_elems + ml_elems + (1 << 14))
        commit = PiopCommit(hal, d_c, hp, codeword, tree)
        commit.run()

        def run(roles, idx=None):
            plan = PiopCommittedOpenPlan(hal, d_c, d_t, claims, hp, codeword, tree, scratch, roles["bc"], roles["ch"], idx if idx is not None else [0] * p.n_test_queries)
            plan.run()
            return {"items": plan.transcript(), "advice": np.array(plan.advice)}

        def messages(out):
            assert out["items"][-1][0] == "fri_terminate" and fv.ints(out["advice"][: p.terminate_len()]) == out["items"][-1][1]
            return b"".join(pl if kind == "fri_commitment" else T.scalars(pl) for kind, pl in out["items"][:-1])

        ch, roles, out = live_then_array(schedule, run, messages, lambda out: out["advice"].tobytes())
        commitment = commit.commitment

    _c, items, _evals, terminate = piop_ref.piop_prove(committed, transparents, claims, op, roles["bc"], roles["ch"])
    assert out["items"] == items and fv.ints(out["advice"][: p.terminate_len()]) == list(terminate)

    def verifier(msg, dec):
        """piop::verify from the bytes: the items are cut out of the message by the schedule, the samples come from a fresh challenger"""
        drawn, idx = T.replay(schedule, msg, bits=p.index_bits())
        got, at = [], 0
        for kind, n_bytes in kinds:
            chunk, at = msg[at : at + n_bytes], at + n_bytes
            got.append((kind, chunk if kind == "fri_commitment" else fv.ints(np.frombuffer(chunk, dtype=np.uint64).reshape(-1, 2))))
        advice = np.frombuffer(dec, dtype=np.uint64).reshape(-1, 2)
        got.append(("fri_terminate", fv.ints(advice[: p.terminate_len()])))
        verify_transcript(oracle, piop_ref, n_varss, committed, transparents, claims, op, drawn["bc"], drawn["ch"], got)
        final = fv.verify(oracle, p, commitment, [pl for kind, pl in got if kind == "fri_commitment"], drawn["ch"], idx, advice)
        piece_evals = []
        for v, payload in zip(sizes, [pl for kind, pl in got if kind == "multilinear_evals"]):
            piece_evals += payload[: meta.n_multilins_by_vars[v]]
        piece_evals.reverse()
        assert final == piecewise(oracle, drawn["ch"], meta.n_multilins_by_vars, piece_evals)

    msg, dec = bytes(ch.written[M]), bytes(ch.written[D])
    verifier(msg, dec)
    for at in segment_starts(schedule):
        with pytest.raises((AssertionError, fv.FriVerifyError)):
            verifier(flipped(msg, at + 5), dec)
