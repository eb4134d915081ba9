"""The witness plan (binius_amd/host/witness.hpp, bnh_witness_derive) against tests/derive_ref.py: a keccak-shaped chain of virtual
columns over small B1 columns, a B128 combination through the existing lincomb op, what the plan rejects, and u32_add's cin derived on
the device and handed to the zerocheck prover in place of an uploaded one."""
import numpy as np
import pytest

import derive_ref as D
import zerocheck_skip_ref as R
from test_zerocheck_skip_oracle import samples, u32_add_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    with binius_amd.Context(0, 1 << 20) as h:
        yield h


def upload(hal, alloc, values, level):
    packed = D.pack(values, level)
    d = alloc.alloc(packed.shape[0])
    hal.copy_h2d(packed, d)
    return d


def run_plan(hal, alloc, columns):
    from binius_amd._host import WitnessPlan

    scratch = alloc.alloc(max(1, WitnessPlan.scratch_elems(columns)))
    plan = WitnessPlan(hal, columns, scratch.slice(0, WitnessPlan.scratch_elems(columns)))  # (exactly what the formula says: not an element more)
    return plan, plan.run()


def test_keccak_shaped_chain(hal):
    rng = np.random.default_rng(0x3E77)
    n = 12  # 2^12 bits: 32 elements a column
    state = [D.random_values(rng, 0, n) for _ in range(5)]
    other = D.random_values(rng, 0, n)
    byte = np.array([0xB7], dtype=np.uint8)
    word = D.random_values(rng, 0, 5)  # 32 bits: below one element
    alloc = hal.dev_alloc()
    d_state = [upload(hal, alloc, v, 0) for v in state]
    d_other, d_byte, d_word = upload(hal, alloc, other, 0), upload(hal, alloc, byte, 3), upload(hal, alloc, word, 0)
    columns = [("given", d, 0, n) for d in d_state] + [
        ("given", d_other, 0, n),                                # 5
        ("lincomb", [(i, 1) for i in range(5)], 0, n),           # 6: c[x], wave 1
        ("shifted", 6, 6, 1, "circular_left"),                   # 7: its rotation in 64-bit blocks, wave 2
        ("lincomb", [(7, 1), (5, 1)], 0, n),                     # 8: wave 3
        ("packed", 0, 3),                                        # 9: an alias
        ("given", d_byte, 3, 0),                                 # 10: an 8-bit constant
        ("repeating", 10, 9),                                    # 11: repeated to 2^9 bytes, wave 1
        ("zero_padded", 5, 2, 3, 2),                             # 12: wave 1
        ("given", d_word, 0, 5),                                 # 13
        ("shifted", 13, 5, 1, "logical_left"),                   # 14: below one element: host work, no launch
        ("repeating", 10, 2),                                    # 15: four bytes: host work
        ("lincomb", [(13, 1), (14, 1)], 1, 5),                   # 16: an XOR below one element behind a host column: wave 2, host work
    ]
    c_x = D.xor_combination(state, 0, 0, n)
    rot = D.shifted(c_x, 6, 1, D.CIRCULAR_LEFT)
    shifted_word = D.shifted(word, 5, 1, D.LOGICAL_LEFT)
    want = {6: (c_x, 0), 7: (rot, 0), 8: (rot ^ other, 0), 9: (np.packbits(state[0], bitorder="little"), 3), 11: (D.repeating(byte, 9), 3),
            12: (D.zero_padded(other, 2, 3, 2), 0), 14: (shifted_word, 0), 15: (D.repeating(byte, 2), 3), 16: (word ^ shifted_word ^ 1, 0)}
    before = hal.derive_counters()
    for _ in range(2):  # resident inputs, run twice: the same values
        plan, got = run_plan(hal, alloc, columns)
        assert plan.n_waves == 3 and plan.n_launches == 3  # one launch per wave; aliases and host columns make none
        for i, (values, level) in want.items():
            d, got_level, got_n_vars = got[i]
            assert got_level == level and 1 << got_n_vars == len(values), i
            assert np.array_equal(hal.copy_d2h(d), D.pack(values, level)), "column %d differs from the restatement" % i
        assert got[9][0].ptr == d_state[0].ptr and got[9][1:] == (3, n - 3)
        for i, c in enumerate(columns):
            if c[0] == "given":
                assert got[i][0].ptr == c[1].ptr and got[i][1:] == (c[2], c[3])
    after = hal.derive_counters()
    assert after["calls"] - before["calls"] == 6 and after["launches"] - before["launches"] == 6
    assert after["jobs"] - before["jobs"] == 2 * 5  # columns 6, 7, 8, 11, 12
    for d, v in zip(d_state + [d_other], state + [other]):
        assert np.array_equal(hal.copy_d2h(d), D.pack(v, 0)), "an input was modified"


def test_b128_combination_goes_through_the_lincomb_op(hal, oracle):
    n = 5
    x, y = oracle.random_b128(0xD301, 1 << n), oracle.random_b128(0xD302, 1 << n)
    c1, c2, offset = oracle.random_scalars(0xD303, 3)
    bits = D.random_values(np.random.default_rng(5), 0, 12)
    alloc = hal.dev_alloc()
    d_x, d_y, d_bits = alloc.alloc(1 << n), alloc.alloc(1 << n), upload(hal, alloc, bits, 0)
    hal.copy_h2d(x, d_x)
    hal.copy_h2d(y, d_y)
    columns = [("given", d_x, 7, n), ("given", d_y, 7, n), ("given", d_bits, 0, 12),
               ("lincomb", [(0, c1), (1, c2)], offset, n),   # 3: random coefficients: the lincomb op
               ("lincomb", [(0, 1), (1, 1)], offset, n),     # 4: all ONE at the terms' level: the XOR form
               ("shifted", 2, 12, 100, "logical_right")]     # 5: beside them in the same wave
    ints = lambda a: [int(r[0]) | (int(r[1]) << 64) for r in a]  # noqa: E731
    xi, yi = ints(x), ints(y)
    want3 = [offset ^ oracle.mul(c1, a) ^ oracle.mul(c2, b) for a, b in zip(xi, yi)]
    want4 = [offset ^ a ^ b for a, b in zip(xi, yi)]
    pel, dv = hal.partial_eval_lincomb_counters(), hal.derive_counters()
    plan, got = run_plan(hal, alloc, columns)
    pel2, dv2 = hal.partial_eval_lincomb_counters(), hal.derive_counters()
    assert pel2["calls"] - pel["calls"] == 1 and pel2["jobs"] - pel["jobs"] == 1
    assert dv2["calls"] - dv["calls"] == 1 and dv2["jobs"] - dv["jobs"] == 2
    assert plan.n_waves == 1 and plan.n_launches == 2
    assert [g[1:] for g in got[3:]] == [(7, n), (7, n), (0, 12)]
    assert ints(hal.copy_d2h(got[3][0])) == want3
    assert ints(hal.copy_d2h(got[4][0])) == want4
    assert np.array_equal(hal.copy_d2h(got[5][0]), D.pack(D.shifted(bits, 12, 100, D.LOGICAL_RIGHT), 0))


def test_what_the_plan_rejects(hal):
    from binius_amd._ffi import BnError
    from binius_amd._host import WitnessPlan

    alloc = hal.dev_alloc()
    words = D.random_values(np.random.default_rng(6), 5, 5)
    d = upload(hal, alloc, words, 5)
    scratch = alloc.alloc(64)
    before = hal.derive_counters(), hal.partial_eval_lincomb_counters()
    bad = {
        "a B32 combination with a non-unit coefficient": [("given", d, 5, 5), ("lincomb", [(0, 3)], 0, 5)],
        "unit coefficients over terms of a lower level than the offset's": [("given", d, 5, 5), ("lincomb", [(0, 1)], 1 << 40, 5)],
        "an inner index that is not smaller": [("given", d, 5, 5), ("shifted", 1, 2, 1, 0)],
        "a term with another n_vars": [("given", d, 5, 5), ("lincomb", [(0, 1)], 0, 4)],
        "a shift offset of a whole block": [("given", d, 5, 5), ("shifted", 0, 2, 4, 0)],
        "packed above the tower": [("given", d, 5, 5), ("packed", 0, 3)],
        "an unknown kind": [("given", d, 5, 5), (6, 0, 0)],
    }
    for name, columns in bad.items():
        with pytest.raises(BnError) as e:
            WitnessPlan(hal, columns, scratch).run()
        assert e.value.kind == "InputValidation", name
    ok = [("given", d, 5, 5), ("lincomb", [(0, 1)], 0xFFFFFFFF, 5)]
    with pytest.raises(BnError) as e:  # one element short of the formula
        WitnessPlan(hal, ok, scratch.slice(0, WitnessPlan.scratch_elems(ok) - 1)).run()
    assert e.value.kind == "InputValidation"
    assert (hal.derive_counters(), hal.partial_eval_lincomb_counters()) == before  # everything is checked before the first device call


def test_derived_cin_is_a_drop_in_for_an_uploaded_one(hal, oracle):
    """u32_add: cin = cout << 1 inside 32-bit blocks, built by the plan from the uploaded cout; the zerocheck prover's outputs equal the
    restatement's proof computed with the host-made cin."""
    from binius_amd._host import ZerocheckBatchPlan

    k = 6
    table = u32_add_table(4, 0xADD)
    (xin, _), (yin, _), (cin, _), (cout, _), (zout, _) = table["cols"]
    assert np.array_equal(D.shifted(cout, 5, 1, D.LOGICAL_LEFT), cin)  # the gadget's identity, on the host's columns
    args = samples(oracle, 0x7700, [table], k)
    want = R.prove([table], k, *args)
    alloc = hal.dev_alloc()
    n = table["n_vars"]
    d_x, d_y, d_cout, d_z = (upload(hal, alloc, v, 0) for v in (xin, yin, cout, zout))
    plan, got = run_plan(hal, alloc, [("given", d_cout, 0, n), ("shifted", 0, 5, 1, "logical_left")])
    d_cin = got[1][0]
    assert got[1][1:] == (0, n) and np.array_equal(hal.copy_d2h(d_cin), D.pack(cin, 0))
    d_tables = [(n, [(d_x, 0), (d_y, 0), (d_cin, 0), (d_cout, 0), (d_z, 0)], table["comps"])]
    scratch = alloc.alloc(ZerocheckBatchPlan.scratch_elems(d_tables, k))
    proof = ZerocheckBatchPlan(hal, d_tables, k, *args, scratch).run()
    for key in ("message", "round_coeffs", "final_evals", "reduction_round_coeffs", "reduction_final_evals", "skipped_challenges", "unskipped_challenges",
                "concat_multilinear_evals"):
        assert proof[key] == want[key], "%s differs" % key
