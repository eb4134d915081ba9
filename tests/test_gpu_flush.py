"""GPU parity of the flush witnesses: bn_flush_witness_batch (binius_amd/csrc/kernels_flush.hip + abi_flush.cpp; reference:
make_masked_flush_witnesses and count_zero_suffixes, constraint_system/prove.rs:671-902) against tests/flush_ref.py (pinned by
tests/test_flush_oracle.py), and bnh_flush_prodcheck_prove (binius_amd/host/flush.hpp; reference: constraint_system/prove.rs:276-428,
1017-1117) against flush_prodcheck_prove and the verifier's equations of the same file.  Everything is bit-exact and nothing is compared
with the device's own output.  For the op, in every case the output is pre-filled with the canary, and the tail beyond the prefix
length, the inputs and the returned prefix lengths are checked.  One context per module."""
import functools

import numpy as np
import pytest

import adversarial as A
import flush_ref as R

pytestmark = pytest.mark.gpu

ARENA_ELEMS = 1 << 24
CANARY_ROW = np.array([A.CANARY & A.M64, A.CANARY >> 64], dtype=np.uint64)


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, ARENA_ELEMS)
    yield ctx
    ctx.close()


def rand_bits(seed, n):
    import oracle

    return (oracle.splitmix_words(seed, n) & np.uint64(1)).astype(np.uint8)


def scalar(seed):
    import oracle

    return oracle.random_scalars(seed, 1)[0]


def run_flushes(hal, flushes, framed=True, alloc=None):
    """flushes: [(n_vars, selectors, columns, const_term)] in flush_ref's conventions.  One call of the op for all of them.  Every
    output is pre-filled with the canary: rows below the prefix must equal the restatement, rows at and beyond it must still hold
    the canary; the inputs must be unchanged and the returned prefix lengths equal.  framed: every array sits between canary frames
    at a 16-byte base that is not otherwise aligned.  Returns (prefix lengths, output slices, expected witnesses)."""
    alloc = hal.dev_alloc() if alloc is None else alloc
    checks, lead = [], 1

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

    n_vars, sels, cols, consts, outs, frames, want = [], [], [], [], [], [], []
    for n, selectors, columns, const_term in flushes:
        n_vars.append(n)
        sels.append([put(R.pack_bits(s)) for s in selectors])
        cols.append([(put(R.pack_column(v, level)), level, coeff) for v, level, coeff in columns])
        consts.append(const_term)
        if framed:
            s, chk = A.place(hal, alloc, 1 << n, lead)
            lead += 2
            frames.append(functools.partial(chk, body=False))
        else:
            s = alloc.alloc(1 << n)
            hal.fill(s, A.CANARY)
        outs.append(s)
        want.append(R.flush_witness(n, selectors, columns, const_term))
    got_lens = hal.flush_witness_batch(n_vars, sels, cols, consts, outs)
    for t, (prefix, witness) in enumerate(want):
        what = "flush %d (n_vars %d, %d selectors, levels %s)" % (t, n_vars[t], len(sels[t]), [c[1] for c in cols[t]])
        assert got_lens[t] == prefix, "%s: prefix length %d, expected %d" % (what, got_lens[t], prefix)
        got = hal.copy_d2h(outs[t])
        bad = np.flatnonzero((got[:prefix] != witness[:prefix]).any(axis=1))
        assert bad.size == 0, "%s: %d rows differ, the first at %d" % (what, bad.size, bad[0])
        assert (got[prefix:] == CANARY_ROW).all(), "%s: the tail beyond the prefix was written" % what
    for chk in checks + frames:
        chk()
    return got_lens, outs, want


@functools.lru_cache(maxsize=None)
def column(seed, n_vars, level):
    return R.random_column(seed, 1 << n_vars, level)


@pytest.mark.parametrize("level", R.LEVELS)
@pytest.mark.parametrize("n_vars", [0, 1, 3, 6, 7, 8, 10, 13, 16])
def test_one_column_no_selector(hal, n_vars, level):
    col = column(0xA1000 + 16 * n_vars + level, n_vars, level)
    run_flushes(hal, [(n_vars, [], [(col, level, scalar(0xA1100 + level))], scalar(0xA1200 + n_vars))])


def test_mixed_levels_with_constants_between_the_columns(hal):
    """B1 + B8 + B32 + B128 columns with constant entries between them: the columns' coefficients skip mixing powers."""
    n = 12
    alpha, r = scalar(0xA2000), scalar(0xA2001)
    entries = [("oracle",), ("const", 0x1234), ("oracle",), ("oracle",), ("const", scalar(0xA2002)), ("const", 7), ("oracle",)]
    const_term, coeffs = R.mixing_terms(entries, alpha, r)
    import oracle

    assert coeffs[0] == 1 and coeffs[1] == oracle.mul(alpha, alpha) and coeffs[3] == oracle.mul(oracle.mul(coeffs[2], alpha), oracle.mul(alpha, alpha))
    levels = [0, 3, 5, 7]
    cols = [(column(0xA2100 + l, n, l), l, c) for l, c in zip(levels, coeffs)]
    run_flushes(hal, [(n, [rand_bits(0xA2200, 1 << n)], cols, const_term)])


@pytest.mark.parametrize("level", [3, 5, 7])
def test_first_coefficient_one_and_not_one(hal, level):
    """The shortcut for a coefficient ONE (no table: the value itself) and the table path against the same restatement, which
    knows no shortcut: ONE as the first and as the last coefficient of a flush (equal expected data), alone, and the same column
    under a coefficient that is not ONE."""
    n = 9
    x, y, c = column(0xA3000 + level, n, level), column(0xA3100 + level, n, level), scalar(0xA3200)
    const_term = scalar(0xA3300)
    _, outs, want = run_flushes(hal, [(n, [], [(x, level, 1), (y, level, c)], const_term), (n, [], [(y, level, c), (x, level, 1)], const_term),
                                      (n, [], [(x, level, 1)], 0), (n, [], [(x, level, c)], 0)])
    assert np.array_equal(want[0][1], want[1][1])
    assert np.array_equal(hal.copy_d2h(outs[0]), hal.copy_d2h(outs[1])), "the result depends on the position of the coefficient ONE"
    assert np.array_equal(want[2][1], R.embed(x, level)), "coefficient ONE, no constant: the witness is the embedded column"


def selector_with_last_bit(n_vars, last, seed):
    s = rand_bits(seed, 1 << n_vars)
    s[last + 1 :] = 0
    s[last] = 1
    return s


@pytest.mark.parametrize("n_vars", [8, 12])
@pytest.mark.parametrize("where", ["row0", "row127", "row128", "last", "three_fifths"])
def test_selector_cut(hal, n_vars, where):
    rows = 1 << n_vars
    last = {"row0": 0, "row127": 127, "row128": 128, "last": rows - 1, "three_fifths": (3 * rows // 5) | 1}[where]
    sel = selector_with_last_bit(n_vars, last, 0xA4000 + n_vars)
    assert R.selector_prefix(sel, n_vars) == min(rows, 128 * (last // 128 + 1))
    cols = [(column(0xA4100, n_vars, 5), 5, scalar(0xA4200)), (column(0xA4101, n_vars, 3), 3, scalar(0xA4201))]
    run_flushes(hal, [(n_vars, [sel], cols, scalar(0xA4300))])


@pytest.mark.parametrize("n_vars", [3, 7, 11])
def test_selectors_none_one_three_all_ones_all_zeros(hal, n_vars):
    rows = 1 << n_vars
    ones, zeros = np.ones(rows, dtype=np.uint8), np.zeros(rows, dtype=np.uint8)
    a, b = rand_bits(0xA5000 + n_vars, rows), rand_bits(0xA5001 + n_vars, rows)
    # one selector on where another is off inside the prefix: the row is ONE
    b[0], a[0] = 0, 1
    cols = [(column(0xA5100, n_vars, 4), 4, scalar(0xA5200)), (column(0xA5101, n_vars, 0), 0, scalar(0xA5201))]
    ct = scalar(0xA5300)
    lens, _, want = run_flushes(hal, [(n_vars, [], cols, ct), (n_vars, [a], cols, ct), (n_vars, [a, b, ones], cols, ct), (n_vars, [ones], cols, ct),
                                      (n_vars, [zeros], cols, ct), (n_vars, [ones, zeros, a], cols, ct)])
    assert lens[4] == 0 and lens[5] == 0 and lens[0] == rows and lens[3] == rows
    assert tuple(want[2][1][0]) == (1, 0), "row 0: a selector is off, the witness is ONE"


def test_selectors_of_different_prefixes(hal):
    """The prefix is the minimum over the selectors: the short one cuts the long one."""
    n = 11
    long_sel, short_sel = selector_with_last_bit(n, 1500, 0xA6000), selector_with_last_bit(n, 700, 0xA6001)
    cols = [(column(0xA6100, n, 6), 6, scalar(0xA6200))]
    lens, _, _ = run_flushes(hal, [(n, [long_sel, short_sel], cols, 5), (n, [short_sel, long_sel], cols, 5)])
    assert lens == [768, 768]


def test_64_wide_columns_go_multipass(hal):
    n = 10
    base = [column(0xA7000 + j, n, 7) for j in range(4)]
    cols = [(base[j % 4], 7, scalar(0xA7100 + j)) for j in range(64)]
    before = hal.flush_counters()
    run_flushes(hal, [(n, [rand_bits(0xA7200, 1 << n)], cols, scalar(0xA7300))], framed=False)
    after = hal.flush_counters()
    assert after["multipass"] - before["multipass"] == 1 and after["flushes"] - before["flushes"] == 1
    # 33 B64 columns: 528 tables, three passes, the last one a single column
    cols = [(column(0xA7400 + (j % 3), n, 6), 6, scalar(0xA7500 + j)) for j in range(33)]
    run_flushes(hal, [(n, [], cols, 0)], framed=False)
    assert hal.flush_counters()["multipass"] - after["multipass"] == 1


def mixed_batch(count):
    fl = []
    for t in range(count):
        n = (7 * t + 2) % 16
        n_sel = t % 4
        levels = [R.LEVELS[(t + j) % 6] for j in range(1 + t % 5)]
        sels = [rand_bits(0xA8000 + 16 * t + s, 1 << n) for s in range(n_sel)]
        if n_sel and t % 3 == 0:
            sels[0] = selector_with_last_bit(n, ((3 << n) // 5) | 1 if n else 0, 0xA8800 + t)
        cols = [(column(0xA9000 + 8 * t + j, n, l), l, 1 if (j == 0 and t % 2) else scalar(0xA9800 + 8 * t + j)) for j, l in enumerate(levels)]
        fl.append((n, sels, cols, scalar(0xAA000 + t)))
    return fl


def test_batch_of_40_mixed_flushes_and_two_large_ones_in_one_call(hal):
    fl = mixed_batch(40)
    assert {f[0] for f in fl} == set(range(16))
    for n, seed in ((17, 0xAB000), (18, 0xAB100)):
        sel = selector_with_last_bit(n, ((3 << n) // 5) | 1, seed)
        fl.append((n, [sel], [(column(seed + 1, n, 5), 5, scalar(seed + 2)), (column(seed + 3, n, 3), 3, scalar(seed + 4))], scalar(seed + 5)))
    before = hal.flush_counters()
    run_flushes(hal, fl, framed=False)
    mid = hal.flush_counters()
    assert mid["calls"] - before["calls"] == 1 and mid["flushes"] - before["flushes"] == 42
    run_flushes(hal, [fl[1]], framed=False)
    one = hal.flush_counters()["launches"] - mid["launches"]
    assert len(fl[1][1]) >= 1 and mid["launches"] - before["launches"] == one == 2, "the launch count depends on the batch"
    run_flushes(hal, [fl[0]], framed=False)  # (no selector: no pre-pass)
    assert hal.flush_counters()["launches"] - mid["launches"] == one + 1


@pytest.mark.parametrize("coeff_kind", ["zero", "sub3", "sub5", "sparse", "dense"])
@pytest.mark.parametrize("col_kind", ["zero", "sub3", "sub5", "sparse", "dense"])
def test_adversarial_b128_columns_and_coefficients(hal, col_kind, coeff_kind):
    import oracle

    n = 9
    col = A.operands(col_kind, 0xAC000, 1 << n)
    coeffs = oracle.arr_to_ints(A.operands(coeff_kind, 0xAC100, 2))
    run_flushes(hal, [(n, [rand_bits(0xAC200, 1 << n)], [(col, 7, coeffs[0]), (column(0xAC300, n, 5), 5, coeffs[1])], coeffs[0])])


def test_validation_errors_launch_nothing_and_leave_the_context_usable(hal):
    from binius_amd._ffi import BnError, DevSlice

    alloc = hal.dev_alloc()
    col, sel = alloc.alloc(256), alloc.alloc(2)
    out, check_out = A.place(hal, alloc, 1 << 8, 3)
    before = hal.flush_counters()

    def rejected(*args):
        with pytest.raises(BnError) as e:
            hal.flush_witness_batch(*args)
        assert e.value.kind == "InputValidation"

    rejected([8], [[]], [[]], [0], [out])  # zero columns: EmptyFlushOracles
    rejected([8], [[]], [[(col, 1, 3)]], [0], [out])  # level 1
    rejected([8], [[]], [[(col, 2, 3)]], [0], [out])  # level 2
    rejected([29], [[]], [[(col, 0, 3)]], [0], [DevSlice(out.ptr, 1 << 29)])  # n_vars 29
    rejected([8], [[sel] * 9], [[(col, 5, 3)]], [0], [out])  # nine selectors
    rejected([8], [[sel]], [[(col, 5, 3)] * 65], [0], [out])  # 65 columns
    rejected([8], [[None]], [[(col, 5, 3)]], [0], [out])  # a NULL selector
    rejected([8], [[]], [[(None, 5, 3)]], [0], [out])  # a NULL column
    rejected([8], [[]], [[(col, 5, 3)]], [0], [None])  # a NULL output
    rejected([8], [[]], [[(col, 7, 3)]], [0], [DevSlice(col.ptr + 16 * 255, 1 << 8)])  # the output overlaps its column
    rejected([8, 8], [[], []], [[(col, 7, 3)], [(out, 7, 3)]], [0, 0], [out, alloc.alloc(256)])  # ... or a column of another flush
    rejected([8, 8], [[], []], [[(col, 7, 3)], [(col, 7, 3)]], [0, 0], [out, DevSlice(out.ptr + 16, 256)])  # ... or another output
    assert hal.flush_counters() == before, "a rejected call launched something"
    check_out(None)
    assert hal.flush_witness_batch([], [], [], [], []) == []  # n_flushes = 0 is a no-op
    assert hal.flush_counters() == before
    run_flushes(hal, [(8, [rand_bits(0xAD000, 256)], [(column(0xAD100, 8, 5), 5, scalar(0xAD200))], 9)])


@pytest.mark.parametrize("n_vars", [5, 11, 14])
def test_the_witness_and_its_prefix_feed_the_product_tree(hal, n_vars):
    """Composition with the next op: the output and prefix_lens_out as bn_product_tree_layers' input and input_lens give the
    restatement's grand product (the unwritten tail, still canary, must count as ONE)."""
    rows = 1 << n_vars
    sel = selector_with_last_bit(n_vars, ((3 * rows) // 5) | 1, 0xAE000 + n_vars)
    cols = [(column(0xAE100 + n_vars, n_vars, 5), 5, 1), (column(0xAE200 + n_vars, n_vars, 3), 3, scalar(0xAE300))]
    from binius_amd._ffi import DevSlice

    alloc = hal.dev_alloc()
    lens, outs, want = run_flushes(hal, [(n_vars, [sel], cols, scalar(0xAE400))], framed=False, alloc=alloc)

    products = hal.product_tree_layers([n_vars], [DevSlice(outs[0].ptr, lens[0]) if lens[0] else None], [alloc.alloc(rows)])
    assert products[0] == R.product(want[0][1])


# ---------------------------------------------------------------------------------------------- the prover
def samples(oracle, flushes, nonzero, seed):
    m = max([fl["n_vars"] for fl in flushes] + [z[3] for z in nonzero] + [0])
    groups = R.flush_groups(flushes)
    S = oracle.random_scalars
    return {"mixing_challenge": S(seed, 1)[0], "permutation_challenges": S(seed + 1, 1 + max([fl["channel"] for fl in flushes] + [0])),
            "gpa_batch_coeffs": S(seed + 2, max(1, m))[:m], "gpa_sumcheck_challenges": [S(seed + 100 + j, max(1, j))[:j] for j in range(m)],
            "gpa_challenges": S(seed + 3, max(1, m))[:m], "red_batch_coeffs": S(seed + 4, max(1, len(groups)))[: len(groups)],
            "red_challenges": [S(seed + 200 + g, max(1, n))[:n] for g, (n, _, _) in enumerate(groups)]}


def run_prover(hal, flushes, nonzero, smp, scratch_elems=None):
    """The device prover over freshly uploaded columns (one upload per oracle id); returns its output in flush_prodcheck_prove's shape.
    The inputs must come back unchanged."""
    from binius_amd._host import FlushProdcheckPlan

    alloc = hal.dev_alloc()
    by_id, kept = {}, []

    def put(oid, arr):
        if oid not in by_id:
            s = alloc.alloc(arr.shape[0])
            hal.copy_h2d(arr, s)
            kept.append((s, arr))
            by_id[oid] = s
        return by_id[oid]

    d_flushes = [{"channel": fl["channel"], "n_vars": fl["n_vars"], "selectors": [(i, put(i, R.pack_bits(b))) for i, b in fl["selectors"]],
                  "entries": [(("oracle", e[1], put(e[1], R.pack_column(e[2], e[3])), e[3]) if e[0] == "oracle" else e) for e in fl["entries"]]} for fl in flushes]
    d_nonzero = [(i, put(i, R.pack_column(v, level)), level, n) for i, v, level, n in nonzero]
    need = FlushProdcheckPlan.scratch_elems(d_flushes, d_nonzero)
    scratch = alloc.alloc(need if scratch_elems is None else scratch_elems)
    plan = FlushProdcheckPlan(hal, d_flushes, d_nonzero, smp["mixing_challenge"], smp["permutation_challenges"], scratch, smp["gpa_batch_coeffs"],
                              smp["gpa_sumcheck_challenges"], smp["gpa_challenges"], smp["red_batch_coeffs"], smp["red_challenges"])
    try:
        plan.run()
    finally:
        for s, arr in kept:
            assert np.array_equal(hal.copy_d2h(s), arr), "the prover wrote to an input"
    return plan.output()


def restated(flushes, nonzero, smp):
    return R.flush_prodcheck_prove(flushes, nonzero, smp["mixing_challenge"], smp["permutation_challenges"], smp["gpa_batch_coeffs"], smp["gpa_sumcheck_challenges"],
                                   smp["gpa_challenges"], smp["red_batch_coeffs"], smp["red_challenges"])


def assert_same_transcript(got, want):
    assert got["prefix_lens"] == want["prefix_lens"]
    for key in ("products", "final_evals", "final_points", "layer_evals"):
        assert [list(x) if isinstance(x, (list, tuple)) else x for x in got["gpa"][key]] == [list(x) if isinstance(x, (list, tuple)) else x for x in want["gpa"][key]], \
            "grand-product argument: %s differ from the CPU restatement" % key
    assert [[list(r) for r in step] for step in got["gpa"]["round_proofs"]] == [[list(r) for r in step] for step in want["gpa"]["round_proofs"]]
    assert got["linear_flushes"] == want["linear_flushes"]
    assert len(got["checks"]) == len(want["checks"])
    for g, (a, b) in enumerate(zip(got["checks"], want["checks"])):
        assert a["n_vars"] == b["n_vars"] and a["ids"] == b["ids"], "MLE-check %d: its multilinears differ" % g
        assert [list(r) for r in a["round_proofs"]] == [list(r) for r in b["round_proofs"]], "MLE-check %d: round proofs differ from the CPU restatement" % g
        assert list(a["final_evals"]) == list(b["final_evals"]), "MLE-check %d: final evaluations differ from the CPU restatement" % g


def nonzero_column(seed, n_vars, level):
    col = R.random_column(seed, 1 << n_vars, level).copy()
    if level == 7:
        col[(col[:, 0] == 0) & (col[:, 1] == 0), 0] = 1
    else:
        col[col == 0] = 1
    return col


def two_table_system():
    """Two tables (2^9 and 2^12 rows, plus a 2^4 one on the side) flushing to three channels, with and without selectors, one
    constant entry, oracle ids out of order and shared between flushes; two non-zero oracles."""
    a32, a8, a1 = column(0xB0001, 12, 5), column(0xB0002, 12, 3), column(0xB0003, 12, 0)
    b64, b128 = column(0xB0004, 9, 6), column(0xB0005, 9, 7)
    c16 = column(0xB0006, 4, 4)
    sa, sa2 = selector_with_last_bit(12, ((3 << 12) // 5) | 1, 0xB0010), rand_bits(0xB0011, 1 << 12)
    sb, sc = rand_bits(0xB0012, 1 << 9), rand_bits(0xB0013, 1 << 4)
    flushes = [
        {"channel": 0, "n_vars": 12, "selectors": [(40, sa)], "entries": [("oracle", 7, a32, 5), ("const", 0xABCD), ("oracle", 3, a8, 3)]},
        {"channel": 0, "n_vars": 9, "selectors": [], "entries": [("oracle", 12, b64, 6), ("oracle", 11, b128, 7)]},
        {"channel": 1, "n_vars": 12, "selectors": [(40, sa), (41, sa2)], "entries": [("oracle", 3, a8, 3), ("oracle", 5, a1, 0), ("oracle", 7, a32, 5)]},
        {"channel": 1, "n_vars": 9, "selectors": [(42, sb)], "entries": [("oracle", 11, b128, 7), ("oracle", 12, b64, 6)]},
        {"channel": 2, "n_vars": 4, "selectors": [(43, sc)], "entries": [("oracle", 20, c16, 4)]},
        {"channel": 2, "n_vars": 12, "selectors": [], "entries": [("oracle", 5, a1, 0), ("oracle", 7, a32, 5)]},
    ]
    nonzero = [(30, nonzero_column(0xB0020, 12, 3), 3, 12), (31, nonzero_column(0xB0021, 2, 5), 5, 2)]
    return flushes, nonzero


def test_prover_two_tables_three_channels_vs_restatement(oracle, hal):
    flushes, nonzero = two_table_system()
    smp = samples(oracle, flushes, nonzero, 0xB1000)
    want = restated(flushes, nonzero, smp)
    assert [c["n_vars"] for c in want["checks"]] == [12, 9, 4] and want["linear_flushes"] == [1, 5] and want["prefix_lens"][0] < 1 << 12
    assert len(want["checks"][0]["round_proofs"][0]) == 4 and len(want["checks"][1]["round_proofs"][0]) == 3
    assert_same_transcript(run_prover(hal, flushes, nonzero, smp), want)


def test_prover_two_composite_flushes_sharing_a_column(oracle, hal):
    """Equal size, one point: ONE MLE-check with two compositions over the de-duplicated union of their oracles."""
    n = 8
    shared, x, y = column(0xB2001, n, 5), column(0xB2002, n, 3), column(0xB2003, n, 7)
    s0, s1 = rand_bits(0xB2010, 1 << n), rand_bits(0xB2011, 1 << n)
    flushes = [{"channel": 0, "n_vars": n, "selectors": [(9, s0)], "entries": [("oracle", 4, shared, 5), ("oracle", 8, x, 3)]},
               {"channel": 1, "n_vars": n, "selectors": [(2, s1)], "entries": [("oracle", 6, y, 7), ("const", 5), ("oracle", 4, shared, 5)]}]
    smp = samples(oracle, flushes, [], 0xB2100)
    want = restated(flushes, [], smp)
    assert len(want["checks"]) == 1 and want["checks"][0]["ids"] == [2, 4, 6, 8, 9]
    got = run_prover(hal, flushes, [], smp)
    assert_same_transcript(got, want)
    # the new claims against independent evaluations of the inner columns
    cols = {2: R.embed(s1.astype(np.uint64), 0), 9: R.embed(s0.astype(np.uint64), 0), 4: R.embed(shared, 5), 8: R.embed(x, 3), 6: y}
    for oid, point, ev in R.new_claims(got, smp["red_challenges"]):
        assert ev == oracle.mle_evaluate(np.ascontiguousarray(cols[oid]), n, point), "claim on oracle %d" % oid


def test_prover_flush_only_and_nonzero_only(oracle, hal):
    flushes, nonzero = two_table_system()
    for fl, nz in ((flushes[3:5], []), ([], nonzero), (flushes[1:2], [])):
        smp = samples(oracle, fl, nz, 0xB3000)
        assert_same_transcript(run_prover(hal, fl, nz, smp), restated(fl, nz, smp))


def test_prover_reduces_flushes_of_zero_variables(oracle, hal):
    """Two composite flushes of a single row share the MLE-check over zero variables -- no rounds, the final evaluations are the
    columns' single elements -- next to one of three variables; the second one's selector is zero, so its witness is empty."""
    flushes = [{"channel": 0, "n_vars": 0, "selectors": [(5, np.array([1], dtype=np.uint8))], "entries": [("oracle", 1, column(0xB5001, 0, 5), 5), ("const", 0x1234)]},
               {"channel": 1, "n_vars": 0, "selectors": [(2, np.array([0], dtype=np.uint8))], "entries": [("oracle", 6, column(0xB5002, 0, 3), 3)]},
               {"channel": 0, "n_vars": 3, "selectors": [(9, selector_with_last_bit(3, 7, 0xB5010))], "entries": [("oracle", 4, column(0xB5003, 3, 7), 7)]}]
    smp = samples(oracle, flushes, [], 0xB5100)
    want = restated(flushes, [], smp)
    assert want["prefix_lens"] == [1, 0, 8] and want["linear_flushes"] == []
    assert [(c["n_vars"], len(c["round_proofs"])) for c in want["checks"]] == [(0, 0), (3, 3)]
    assert want["checks"][0]["ids"] == [1, 2, 5, 6] and len(want["checks"][0]["final_evals"]) == 5
    assert_same_transcript(run_prover(hal, flushes, [], smp), want)


def test_prover_reports_a_zero_nonzero_product_and_the_context_stays_usable(oracle, hal):
    from binius_amd._ffi import BnError

    flushes, nonzero = two_table_system()
    zeroed = nonzero[0][1].copy()
    zeroed[1234] = 0
    bad = [(30, zeroed, 3, 12), nonzero[1]]
    smp = samples(oracle, flushes, bad, 0xB4000)
    with pytest.raises(R.ZerosError):
        restated(flushes, bad, smp)
    before = hal.flush_counters()
    with pytest.raises(BnError) as e:
        run_prover(hal, flushes, bad, smp)
    assert "Zeros" in str(e.value)
    assert hal.flush_counters() == before, "work ran after the zeros error"
    with pytest.raises(BnError) as e:
        run_prover(hal, flushes, nonzero, smp, scratch_elems=64)
    assert e.value.kind == "InputValidation"
    eight = dict(flushes[0], selectors=[(40 + i, flushes[0]["selectors"][0][1]) for i in range(8)])
    with pytest.raises(BnError) as e:
        run_prover(hal, [eight], [], samples(oracle, [eight], [], 0xB4100))
    assert e.value.kind == "InputValidation"
    fl = flushes[3:5]
    smp = samples(oracle, fl, [], 0xB4200)
    assert_same_transcript(run_prover(hal, fl, [], smp), restated(fl, [], smp))


def test_prover_at_2_16_passes_the_verifiers_equations(oracle, hal):
    """No CPU prover at this size: the products against the restated witnesses, the grand-product verifier, the MLE-check verifier's
    equations, and every new claim against mle_evaluate of its column."""
    import gkr_gpa_ref as G

    n = 16
    c32, c8 = column(0xB5001, n, 5), column(0xB5002, n, 3)
    sel = selector_with_last_bit(n, ((3 << n) // 5) | 1, 0xB5010)
    nzc = nonzero_column(0xB5020, n, 4)
    flushes = [{"channel": 0, "n_vars": n, "selectors": [(3, sel)], "entries": [("oracle", 1, c32, 5), ("oracle", 2, c8, 3), ("const", 77)]},
               {"channel": 1, "n_vars": n, "selectors": [], "entries": [("oracle", 2, c8, 3), ("oracle", 1, c32, 5)]}]
    nonzero = [(9, nzc, 4, n)]
    smp = samples(oracle, flushes, nonzero, 0xB5100)
    got = run_prover(hal, flushes, nonzero, smp)
    terms = [R.mixing_terms(fl["entries"], smp["mixing_challenge"], smp["permutation_challenges"][fl["channel"]]) for fl in flushes]
    wits = []
    for fl, (ct, cf) in zip(flushes, terms):
        cols = [(e[2], e[3], c) for e, c in zip([e for e in fl["entries"] if e[0] == "oracle"], cf)]
        wits.append(R.flush_witness(n, [s[1] for s in fl["selectors"]], cols, ct))
    assert got["prefix_lens"] == [w[0] for w in wits]
    assert got["gpa"]["products"] == [R.product(w[1]) for w in wits] + [R.product(np.ascontiguousarray(R.embed(nzc, 4)))]
    points, evals = G.gpa_verify([n, n, n], got["gpa"]["products"], got["gpa"], smp["gpa_batch_coeffs"], smp["gpa_sumcheck_challenges"], smp["gpa_challenges"])
    assert points == got["gpa"]["final_points"] and evals == got["gpa"]["final_evals"]
    assert got["linear_flushes"] == [1] and len(got["checks"]) == 1
    R.mlecheck_verify(flushes, terms, got["checks"][0], [0], points[0], [evals[0]], smp["red_batch_coeffs"][0], smp["red_challenges"][0])
    cols = {1: R.embed(c32, 5), 2: R.embed(c8, 3), 3: R.embed(sel.astype(np.uint64), 0)}
    for oid, point, ev in R.new_claims(got, smp["red_challenges"]):
        assert ev == oracle.mle_evaluate(np.ascontiguousarray(cols[oid]), n, point), "claim on oracle %d" % oid
