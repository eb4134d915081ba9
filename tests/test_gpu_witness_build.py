"""The build plan (witness_build of binius_amd/host/witness.hpp, bnh_witness_build, WitnessBuild) against tests/generate_ref.py and
tests/derive_ref.py composed the same way: a chain through every new kind, the old kinds through the new entry point, what is still
rejected, and a step-down selector made on the device in place of an uploaded one."""
import numpy as np
import pytest

import derive_ref as D
import generate_ref as G

pytestmark = pytest.mark.gpu

B64_GENERATOR = 0x070F870DCD9C1D88  # tests/golden/field_kats.json, multiplicative_generators["64"]


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    with binius_amd.Context(0, 1 << 20) as h:
        yield h


def upload(hal, alloc, values, level):
    packed = G.pack(values, level)
    d = alloc.alloc(packed.shape[0])
    hal.copy_h2d(packed, d)
    return d


def run_plan(hal, alloc, columns, cls=None):
    from binius_amd._host import WitnessBuild

    cls = cls or WitnessBuild
    n = cls.scratch_elems(columns)
    scratch = alloc.alloc(max(1, n))
    plan = cls(hal, columns, scratch.slice(0, n))  # (exactly what the formula says: not an element more)
    return plan, plan.run()


def counters(hal):
    return hal.derive_counters(), hal.generate_counters(), hal.partial_eval_lincomb_counters()


def test_chain_through_every_kind(hal):
    rng = np.random.default_rng(0xB11D)
    n = 14  # 2^14 bits: 128 elements; 32 values a row, 2^9 rows
    words = G.random_values(rng, 0, n)
    alloc = hal.dev_alloc()
    d_words = upload(hal, alloc, words, 0)
    columns = [
        ("given", d_words, 0, n),                   # 0
        ("shifted", 0, 5, 3, "logical_right"),      # 1: wave 1, derive
        ("projected_bits", 1, 0, 5, 9),             # 2: bit 9 of every 32-bit word of 1: 2^9 bits, wave 2, generate
        ("repeating", 2, 3),                        # 3: wave 3, derive
        ("step_down", n, 10000),                    # 4: wave 0, generate
        ("incrementing", 5, 9),                     # 5: B32, wave 0
        ("constant", 3, 6, 0xC3),                   # 6: wave 0
        ("zero_padded", 6, 2, 3, 1),                # 7: wave 1, derive
        ("powers", 6, 6, B64_GENERATOR),            # 8: B64, wave 0
        ("select_row", 3, 5),                       # 9: 8 bits: host work in wave 0, no launch
        ("projected_bits", 2, 3, 4, 6),             # 10: 2^5 bits from the 2^9 of column 2: host work in wave 3
        ("projected_bits", 0, 9, 2, 2),             # 11: whole elements of a given column: wave 1, generate
        ("step_up", 7, 1),                          # 12: wave 0
    ]
    shifted = D.shifted(words, 5, 3, D.LOGICAL_RIGHT)
    bit9 = G.projected_bits(shifted, 0, 5, 9)
    const = G.constant(0xC3, 3, 6)
    want = {1: (shifted, 0), 2: (bit9, 0), 3: (D.repeating(bit9, 12), 0), 4: (G.step_down(n, 10000), 0), 5: (G.incrementing(5, 9), 5), 6: (const, 3),
            7: (D.zero_padded(const, 2, 3, 1), 3), 8: (G.powers(B64_GENERATOR, 6, 6), 6), 9: (G.select_row(3, 5), 0), 10: (G.projected_bits(bit9, 3, 4, 6), 0),
            11: (G.projected_bits(words, 9, 2, 2), 0), 12: (G.step_up(7, 1), 0)}
    # the rules: a generated column without an inner is wave 0, a projection one more than its inner, the derived kinds as before
    waves = {0: 0, 1: 1, 2: 2, 3: 3, 4: 0, 5: 0, 6: 0, 7: 1, 8: 0, 9: 0, 10: 3, 11: 1, 12: 0}
    on_host = {9, 10}
    generated, derived = {2, 4, 5, 6, 8, 9, 10, 11, 12} - on_host, {1, 3, 7}
    n_launches = len({waves[i] for i in generated}) + len({waves[i] for i in derived})  # one call of each op per wave that has its columns
    assert n_launches == 3 + 2
    before = counters(hal)
    for _ in range(2):  # resident inputs, run twice: the same values
        plan, got = run_plan(hal, alloc, columns)
        assert plan.n_waves == max(waves.values()) == 3 and plan.n_launches == n_launches
        for i, (vals, level) in want.items():
            d, got_level, got_n_vars = got[i]
            assert got_level == level and 1 << got_n_vars == len(vals), i
            body = hal.copy_d2h(d)
            if len(vals) << level < 128:  # below one element: the values, in the low bits of the element
                mask = (1 << (len(vals) << level)) - 1
                assert (int(body[0][0]) | (int(body[0][1]) << 64)) & mask == int(G.pack(vals, level)[0][0]) & mask, "column %d differs from the restatement" % i
            else:
                assert np.array_equal(body, G.pack(vals, level)), "column %d differs from the restatement" % i
        assert got[0][0].ptr == d_words.ptr
    after = counters(hal)
    assert after[0]["calls"] - before[0]["calls"] == 2 * 2 and after[0]["jobs"] - before[0]["jobs"] == 2 * len(derived)
    assert after[1]["calls"] - before[1]["calls"] == 2 * 3 and after[1]["launches"] - before[1]["launches"] == 2 * 3
    assert after[1]["jobs"] - before[1]["jobs"] == 2 * len(generated)
    assert np.array_equal(hal.copy_d2h(d_words), G.pack(words, 0)), "an input was modified"


def test_old_kinds_give_the_bytes_of_the_derive_plan(hal):
    from binius_amd._host import WitnessPlan

    rng = np.random.default_rng(0x01D)
    n = 12
    state = [D.random_values(rng, 0, n) for _ in range(3)]
    byte = np.array([0xB7], dtype=np.uint8)
    alloc = hal.dev_alloc()
    d_state = [upload(hal, alloc, v, 0) for v in state]
    d_byte = upload(hal, alloc, byte, 3)
    columns = [("given", d, 0, n) for d in d_state] + [
        ("lincomb", [(0, 1), (1, 1), (2, 1)], 0, n),   # 3
        ("shifted", 3, 6, 1, "circular_left"),         # 4
        ("packed", 4, 3),                              # 5
        ("given", d_byte, 3, 0),                       # 6
        ("repeating", 6, 9),                           # 7
        ("zero_padded", 1, 2, 3, 2),                   # 8
        ("repeating", 6, 2),                           # 9: host work
    ]
    old_plan, old = run_plan(hal, alloc, columns, WitnessPlan)
    new_plan, new = run_plan(hal, alloc, columns)
    assert (new_plan.n_waves, new_plan.n_launches) == (old_plan.n_waves, old_plan.n_launches) == (2, 2)
    assert type(new_plan).scratch_elems(columns) == WitnessPlan.scratch_elems(columns)
    for i, ((d_old, *shape_old), (d_new, *shape_new)) in enumerate(zip(old, new)):
        assert shape_old == shape_new, i
        assert np.array_equal(hal.copy_d2h(d_old), hal.copy_d2h(d_new)), "column %d: the build plan's bytes differ from the derive plan's" % i
    assert np.array_equal(hal.copy_d2h(new[4][0]), D.pack(D.shifted(D.xor_combination(state, 0, 0, n), 6, 1, D.CIRCULAR_LEFT), 0))


def test_what_is_still_rejected(hal):
    from binius_amd._ffi import BnError
    from binius_amd._host import WitnessBuild, WitnessPlan

    alloc = hal.dev_alloc()
    d = upload(hal, alloc, G.random_values(np.random.default_rng(6), 0, 12), 0)
    scratch = alloc.alloc(64)
    before = counters(hal)
    with pytest.raises(BnError) as e:  # bnh_witness_derive: kind 6 is an unknown kind, as before
        WitnessPlan(hal, [("given", d, 0, 12), (6, 0, 0, 5)], scratch).run()
    assert e.value.kind == "InputValidation" and "unknown column kind" in str(e.value)
    bad = {
        "an unknown kind": [("given", d, 0, 12), (13, 0, 0, 0)],
        "a projection's inner index that is not smaller": [("given", d, 0, 12), ("projected_bits", 1, 0, 5, 0)],
        "query_bits = 2^query_size": [("given", d, 0, 12), ("projected_bits", 0, 0, 5, 32)],
        "start_index + query_size above the inner's n_vars": [("given", d, 0, 12), ("projected_bits", 0, 8, 5, 0)],
        "query_size zero": [("given", d, 0, 12), ("projected_bits", 0, 0, 0, 0)],
        "a selected row of 2^n_vars": [("select_row", 12, 1 << 12)],
        "a step index above 2^n_vars": [("step_down", 12, (1 << 12) + 1)],
        "a constant above its level": [("constant", 3, 9, 0x100)],
        "a base above its level": [("powers", 4, 9, 0x10000)],
        "powers at level 0": [("powers", 0, 9, 1)],
        "an incrementing column above 2^level variables": [("incrementing", 3, 9)],
        "level 2": [("constant", 2, 9, 1)],
        "a bad column behind good ones": [("step_down", 12, 7), ("given", d, 0, 12), ("projected_bits", 1, 0, 5, 3), ("select_row", 12, 1 << 12)],
    }
    for name, columns in bad.items():
        with pytest.raises(BnError) as e:
            WitnessBuild(hal, columns, scratch).run()
        assert e.value.kind == "InputValidation", name
    ok = [("given", d, 0, 12), ("projected_bits", 0, 0, 5, 3), ("step_down", 12, 77)]
    assert WitnessBuild.scratch_elems(ok) == 1 + 32
    with pytest.raises(BnError) as e:  # one element short of the formula
        WitnessBuild(hal, ok, scratch.slice(0, WitnessBuild.scratch_elems(ok) - 1)).run()
    assert e.value.kind == "InputValidation"
    assert counters(hal) == before  # everything is checked before the first device call


def test_a_step_down_selector_made_by_the_plan_equals_an_uploaded_one(hal):
    """The selector of a table of 3000 rows among 2^12: made on the device, it has the bytes of the one a caller fills and uploads."""
    alloc = hal.dev_alloc()
    rows, n = 3000, 12
    d_uploaded = upload(hal, alloc, G.step_down(n, rows), 0)
    gen = hal.generate_counters()
    plan, got = run_plan(hal, alloc, [("step_down", n, rows)])
    assert plan.n_waves == 0 and plan.n_launches == 1 and got[0][1:] == (0, n)
    assert hal.generate_counters()["jobs"] - gen["jobs"] == 1
    assert got[0][0].len == d_uploaded.len and np.array_equal(hal.copy_d2h(got[0][0]), hal.copy_d2h(d_uploaded))
    # and as an operand: the inner product with a column of ones counts the rows (B1 x B128 subfield inner product)
    ones = np.zeros((1 << n, 2), dtype=np.uint64)
    ones[:, 0] = 1
    d_ones = alloc.alloc(1 << n)
    hal.copy_h2d(ones, d_ones)
    assert hal.inner_product(got[0][0], 0, d_ones) == hal.inner_product(d_uploaded, 0, d_ones) == rows % 2
