"""GPU parity of the GKR exponentiation argument: bn_exp_circuit_layers and bn_bits_to_b128 (binius_amd/csrc/kernels_expcircuit.hip +
abi_expcircuit.cpp; reference: gkr_exp/witness.rs:31-110, 139-156, 258-284) against tests/gkr_exp_ref.py exp_layers, and
bnh_gkr_exp_prove (binius_amd/host/gkr_exp.hpp; reference: gkr_exp/batch_prove.rs:46-315) against exp_prove and the verifier checker of
the same file (pinned by tests/test_gkr_exp_oracle.py).  Everything is bit-exact and nothing is compared with the device's own output.
One context per module."""
import functools

import numpy as np
import pytest

import adversarial as A
import gkr_exp_ref as R

pytestmark = pytest.mark.gpu

ARENA_ELEMS = 1 << 24
FULL_ELEM = 0x0123456789ABCDEFFEDCBA9876543210


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, ARENA_ELEMS)
    yield ctx
    ctx.close()


def rand_bits(seed, n):
    import oracle

    return (oracle.splitmix_words(seed, n) & np.uint64(1)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def random_witness(seed, n_vars, width, kind):
    """(bits, base, layers) of SplitMix64 data; computed once per shape."""
    import oracle

    bits = [rand_bits(seed + 31 * k, 1 << n_vars) for k in range(width)]
    base = oracle.random_scalars(seed + 5, 1)[0] if kind == "static" else oracle.random_b128(seed + 6, 1 << n_vars)
    return bits, base, R.exp_layers(bits, base, kind)


def run_layers(hal, witnesses, framed=True):
    """witnesses: [(n_vars, bits, base, expected layers)].  One call of the op for all of them.  framed: every input and arena sits
    between canary frames at a 16-byte base that is not otherwise aligned; frames and inputs must be unchanged, every layer equal."""
    alloc = hal.dev_alloc()
    n_vars, cols, bases, arenas, checks, lead = [], [], [], [], [], 1

    def unchanged(s, arr):
        assert np.array_equal(hal.copy_d2h(s), arr), "an input was modified"

    def put(arr):
        nonlocal lead
        if framed:
            s, chk = A.place(hal, alloc, arr, lead)
            lead += 2
            checks.append(chk)
            return s
        s = alloc.alloc(arr.shape[0])
        hal.copy_h2d(arr, s)
        checks.append(functools.partial(unchanged, s, arr))
        return s

    for n, bits, base, _ in witnesses:
        n_vars.append(n)
        cols.append([put(R.pack_bits(b)) for b in bits])
        bases.append(base if isinstance(base, int) else put(base))
        if framed:
            s, chk = A.place(hal, alloc, len(bits) << n, lead)
            lead += 2
            checks.append(functools.partial(chk, body=False))
        else:
            s = alloc.alloc(len(bits) << n)
        arenas.append(s)
    hal.exp_circuit_layers(n_vars, cols, bases, arenas)
    for t, (n, bits, _, layers) in enumerate(witnesses):
        got = hal.copy_d2h(arenas[t])
        for k in range(len(bits)):
            assert np.array_equal(got[k << n : (k + 1) << n], layers[k]), "witness %d (n_vars %d, width %d): layer %d differs" % (t, n, len(bits), k)
    for chk in checks:
        chk()


@pytest.mark.parametrize("kind", ["static", "dynamic"])
@pytest.mark.parametrize("width", [1, 2, 3])
@pytest.mark.parametrize("n_vars", [0, 1, 4, 6, 7, 8, 10])
def test_single_witness(hal, n_vars, width, kind):
    bits, base, layers = random_witness(0xF1000 + 97 * n_vars + width, n_vars, width, kind)
    run_layers(hal, [(n_vars, bits, base, layers)])


@pytest.mark.parametrize("kind", ["static", "dynamic"])
@pytest.mark.parametrize("width", [32, 64, 128])
def test_wide_exponents(hal, width, kind):
    bits, base, layers = random_witness(0xF2000 + width, 8, width, kind)
    run_layers(hal, [(8, bits, base, layers)])


def mixed_batch(count):
    ws = []
    for t in range(count):
        n, kind = (5 * t + 3) % 13, ("static", "dynamic")[t & 1]
        width = [1, 2, 64, 7, 33, 3][t % 6] if n <= 9 else [1, 5, 2][t % 3]
        bits, base, layers = random_witness(0xF3000 + t, n, width, kind)
        ws.append((n, bits, base, layers))
    return ws


def test_mixed_batch_in_one_call_and_its_launch_count(hal):
    ws = mixed_batch(26)
    assert {w[0] for w in ws} == set(range(13)) and max(len(w[1]) for w in ws) == 64 and min(len(w[1]) for w in ws) == 1
    before = hal.exp_counters()
    run_layers(hal, ws, framed=False)
    mid = hal.exp_counters()
    assert mid["calls"] - before["calls"] == 1
    many = mid["launches"] - before["launches"]
    # the same largest width with a tenth of the witnesses: the same number of launches
    few_ws = [w for w in ws if len(w[1]) == 64][:1] + ws[:2]
    run_layers(hal, few_ws, framed=False)
    few = hal.exp_counters()["launches"] - mid["launches"]
    assert many == few, "the launch count depends on the number of witnesses (%d for 26, %d for 3)" % (many, few)
    assert 1 <= many <= 64 + 2


def test_layers_at_2_20(hal):
    """4682 units of 224 rows each for n_cu x 8 wave slots: the grid-stride path."""
    ws = []
    for kind in ("static", "dynamic"):
        bits, base, layers = random_witness(0xF4000, 20, 3, kind)
        ws.append((20, bits, base, layers))
    run_layers(hal, ws, framed=False)


@pytest.mark.parametrize("kind", ["zero", "ones", "sparse", "dense", "sub3", "sub5"])
def test_adversarial_base_columns(hal, kind):
    n, w = 9, 4
    if kind == "ones":
        base = np.zeros((1 << n, 2), dtype=np.uint64)
        base[:, 0] = 1
    else:
        base = A.operands(kind, 0xF5000, 1 << n)
    bits = [rand_bits(0xF5100 + k, 1 << n) for k in range(w)]
    run_layers(hal, [(n, bits, base, R.exp_layers(bits, base, "dynamic"))])


@pytest.mark.parametrize("base", [0, 1])
def test_static_bases_zero_and_one(hal, base):
    n, w = 9, 4
    bits = [rand_bits(0xF6000 + k, 1 << n) for k in range(w)]
    run_layers(hal, [(n, bits, base, R.exp_layers(bits, base, "static"))])


@pytest.mark.parametrize("pattern", ["zeros", "ones", "first", "last"])
def test_adversarial_exponent_columns(hal, pattern):
    import oracle

    n, w = 9, 3
    col = np.zeros(1 << n, dtype=np.uint8)
    if pattern == "ones":
        col[:] = 1
    elif pattern == "first":
        col[0] = 1
    elif pattern == "last":
        col[-1] = 1
    bits = [col.copy() for _ in range(w)]
    dyn = oracle.random_b128(0xF7000, 1 << n)
    run_layers(hal, [(n, bits, FULL_ELEM, R.exp_layers(bits, FULL_ELEM, "static")), (n, bits, dyn, R.exp_layers(bits, dyn, "dynamic"))])


def test_bits_to_b128(hal):
    alloc = hal.dev_alloc()
    logs = [0, 3, 7, 8, 13]
    srcs, dsts, want = [], [], []
    for t, n in enumerate(logs):
        bits = rand_bits(0xF8000 + t, 1 << n)
        s, chk_s = A.place(hal, alloc, R.pack_bits(bits), 1 + 2 * t)
        d, chk_d = A.place(hal, alloc, 1 << n, 2 * t)
        srcs.append(s), dsts.append(d)
        expect = np.zeros((1 << n, 2), dtype=np.uint64)
        expect[:, 0] = bits
        want.append((chk_s, chk_d, expect))
    before = hal.exp_counters()["bits_launches"]
    hal.bits_to_b128(logs, srcs, dsts)
    assert hal.exp_counters()["bits_launches"] - before == 1
    for chk_s, chk_d, expect in want:
        chk_s()
        chk_d(expect=expect)


def test_validation_errors_launch_nothing_and_leave_the_context_usable(hal):
    from binius_amd._ffi import BnError, DevSlice

    alloc = hal.dev_alloc()
    col, base = alloc.alloc(2), alloc.alloc(256)
    arena, check_arena = A.place(hal, alloc, 2 << 8, 3)
    before = hal.exp_counters()

    def rejected(*args, **kw):
        with pytest.raises(BnError) as e:
            hal.exp_circuit_layers(*args, **kw)
        assert e.value.kind == "InputValidation"

    rejected([8], [[]], [5], [DevSlice(arena.ptr, 0)])  # width 0
    rejected([8], [[col] * 129], [5], [DevSlice(arena.ptr, 129 << 8)])  # width 129
    rejected([29], [[col, col]], [5], [DevSlice(arena.ptr, 2 << 29)])  # n_vars 29
    rejected([8], [[col, col]], [5], [arena], kinds=[2])  # unknown kind
    rejected([8], [[col, None]], [5], [arena])  # a NULL bit column
    rejected([8], [[col, col]], [None], [arena], kinds=[1])  # a NULL base column
    rejected([8], [[col, col]], [5], [None])  # a NULL arena
    rejected([8], [[col, col]], [base], [DevSlice(base.ptr + 16 * 255, 2 << 8)])  # the arena overlaps the base column
    rejected([8], [[col, DevSlice(arena.ptr + 16 * 100, 2)]], [5], [arena])  # the arena overlaps a bit column
    assert hal.exp_counters() == before, "a rejected call launched something"
    check_arena(None)
    with pytest.raises(BnError) as e:
        hal.bits_to_b128([3], [None], [arena.slice(0, 8)])
    assert e.value.kind == "InputValidation"
    bits, b, layers = random_witness(0xF1000 + 97 * 7 + 2, 7, 2, "dynamic")
    run_layers(hal, [(7, bits, b, layers)])


# ---------------------------------------------------------------------------------------------- the prover
def make_claims(oracle, shapes, seed, points=None):
    """shapes: [(n_vars, width, kind)], sorted by n_vars descending.  A claim is its result layer's evaluation at a point: one random
    point per n_vars (claims of equal n_vars share it), or points[t]."""
    claims, by_n = [], {}
    for t, (n, w, kind) in enumerate(shapes):
        bits = [rand_bits(seed + 131 * t + k, 1 << n) for k in range(w)]
        base = oracle.random_scalars(seed + 7 * t + 1, 1)[0] if kind == "static" else oracle.random_b128(seed + 7 * t + 2, 1 << n)
        pt = points[t] if points is not None else by_n.setdefault(n, oracle.random_scalars(seed + 1000 + n, max(1, n))[:n])
        layers = R.exp_layers(bits, base, kind)
        claims.append({"n_vars": n, "kind": kind, "base": base, "bits": bits, "point": pt, "eval": oracle.mle_evaluate(layers[-1], n, pt)})
    return claims


def samples(oracle, claims, seed):
    max_w, max_n, k = max(len(c["bits"]) for c in claims), max(c["n_vars"] for c in claims), len(claims)
    flat_c, flat_z = oracle.random_scalars(seed, max_w * k), oracle.random_scalars(seed + 1, max(1, max_w * max_n))
    return [flat_c[L * k : (L + 1) * k] for L in range(max_w)], [flat_z[L * max_n : (L + 1) * max_n] for L in range(max_w)]


def meta_of(claims):
    return [{"n_vars": c["n_vars"], "width": len(c["bits"]), "kind": c["kind"], "base": c["base"] if c["kind"] == "static" else None,
             "point": c["point"], "eval": c["eval"]} for c in claims]


def run_prover(hal, claims, coeffs, chals, scratch_elems=None, n_witnesses=None):
    """The device prover over freshly uploaded witnesses; returns its output in exp_prove's shape.  The inputs must come back unchanged."""
    from binius_amd._host import GkrExpPlan

    alloc = hal.dev_alloc()
    cols, bases, arenas, kept = [], [], [], []

    def put(arr):
        s = alloc.alloc(arr.shape[0])
        hal.copy_h2d(arr, s)
        kept.append((s, arr))
        return s

    for c in claims:
        cols.append([put(R.pack_bits(b)) for b in c["bits"]])
        bases.append(c["base"] if c["kind"] == "static" else put(c["base"]))
        arenas.append(alloc.alloc(len(c["bits"]) << c["n_vars"]))
    n_vars = [c["n_vars"] for c in claims]
    need = GkrExpPlan.scratch_elems(n_vars, [c["kind"] == "dynamic" for c in claims])
    scratch = alloc.alloc(need if scratch_elems is None else scratch_elems)
    plan = GkrExpPlan(hal, n_vars, cols, bases, arenas, [c["point"] for c in claims], [c["eval"] for c in claims], scratch, coeffs, chals, n_witnesses=n_witnesses)
    plan.run()
    for s, arr in kept:
        assert np.array_equal(hal.copy_d2h(s), arr), "the prover wrote to an input"
    return plan.output()


def assert_same_proof(got, want):
    for key in ("round_proofs", "multilinear_evals", "layer_claims"):
        assert [[list(x) if key != "layer_claims" else (list(x[0]), x[1]) for x in layer] for layer in got[key]] == \
               [[list(x) if key != "layer_claims" else (list(x[0]), x[1]) for x in layer] for layer in want[key]], "%s differ from the CPU restatement" % key


MIXED = [(5, 3, "dynamic"), (5, 1, "static"), (3, 4, "static"), (0, 2, "dynamic")]


def test_prover_mixed_batch_vs_restatement(oracle, hal):
    claims = make_claims(oracle, MIXED, 0xFA000)
    coeffs, chals = samples(oracle, claims, 0xFA100)
    want = R.exp_prove(claims, coeffs, chals)
    got = run_prover(hal, claims, coeffs, chals)
    assert_same_proof(got, want)
    assert R.exp_verify(meta_of(claims), got, coeffs, chals) == got["layer_claims"]


def test_prover_two_groups_in_layer_0(oracle, hal):
    n = 4
    pts = [oracle.random_scalars(0xFB000, n), oracle.random_scalars(0xFB001, n)]
    claims = make_claims(oracle, [(n, 3, "static"), (n, 3, "dynamic")], 0xFB010, points=pts)
    coeffs, chals = samples(oracle, claims, 0xFB020)
    want = R.exp_prove(claims, coeffs, chals)
    assert [len(e) for e in want["multilinear_evals"]] == [2, 1, 1]
    got = run_prover(hal, claims, coeffs, chals)
    assert_same_proof(got, want)
    assert R.exp_verify(meta_of(claims), got, coeffs, chals) == got["layer_claims"]


def test_prover_static_only_batch_with_a_layer_without_sumcheck(oracle, hal):
    claims = make_claims(oracle, [(6, 2, "static"), (6, 2, "static"), (2, 1, "static")], 0xFC000)
    coeffs, chals = samples(oracle, claims, 0xFC100)
    want = R.exp_prove(claims, coeffs, chals)
    assert want["round_proofs"][1] == [] and want["multilinear_evals"][1] == []
    got = run_prover(hal, claims, coeffs, chals)
    assert_same_proof(got, want)
    assert R.exp_verify(meta_of(claims), got, coeffs, chals) == got["layer_claims"]


def test_prover_at_2_16_passes_the_verifier(oracle, hal):
    """No CPU prover at this size: the verifier's equations, and every LayerClaim against mle_evaluate of its column."""
    n, w = 16, 8
    claims = make_claims(oracle, [(n, w, "static"), (n, w, "dynamic")], 0xFD000)
    coeffs, chals = samples(oracle, claims, 0xFD100)
    got = run_prover(hal, claims, coeffs, chals)
    layer_claims = R.exp_verify(meta_of(claims), got, coeffs, chals)
    assert layer_claims == got["layer_claims"]
    for L, lc in enumerate(layer_claims):
        (p0, e0), (p1, e1), (p2, e2) = lc
        assert e0 == oracle.mle_evaluate(R.bits_to_b128(claims[0]["bits"][w - 1 - L]), n, p0), "layer %d: static bit claim" % L
        assert e1 == oracle.mle_evaluate(R.bits_to_b128(claims[1]["bits"][L]), n, p1), "layer %d: dynamic bit claim" % L
        assert e2 == oracle.mle_evaluate(claims[1]["base"], n, p2), "layer %d: base claim" % L


def test_prover_validation_errors(oracle, hal):
    from binius_amd._ffi import BnError

    claims = make_claims(oracle, [(3, 2, "static"), (4, 2, "dynamic")], 0xFE000)  # unsorted
    coeffs, chals = samples(oracle, claims, 0xFE100)
    with pytest.raises(BnError) as e:
        run_prover(hal, claims, coeffs, chals)
    assert e.value.kind == "InputValidation" and "ClaimsOutOfOrder" in str(e.value)
    claims = claims[::-1]
    with pytest.raises(BnError) as e:
        run_prover(hal, claims, coeffs, chals, n_witnesses=1)
    assert e.value.kind == "InputValidation" and "MismatchedWitnessClaimLength" in str(e.value)
    with pytest.raises(BnError) as e:
        run_prover(hal, claims, coeffs, chals, scratch_elems=8)
    assert e.value.kind == "InputValidation"
    want = R.exp_prove(claims, coeffs, chals)
    assert_same_proof(run_prover(hal, claims, coeffs, chals), want)
