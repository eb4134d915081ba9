"""The compute plan (witness_compute of binius_amd/host/witness.hpp, bnh_witness_compute, WitnessCompute) on a table shaped like m3's
mul gadget (m3/src/gadgets/mul.rs:466-489) at 2^8 rows, against tests/compose_tower_ref.py and tests/derive_ref.py composed the same way:
B1 bit columns given, 32 composite columns a + s (a + b), pack_fp of them into B32, a shifted column of a computed column (two waves),
a computed column below one element.  Waves and launches against hand counts; what the build plan and the compute plan reject."""
import numpy as np
import pytest

import compose_tower_ref as T
import derive_ref as D
import univariate_skip_base_ref as U

pytestmark = pytest.mark.gpu

N_VARS = 8
SELECT = [("var", 0), ("var", 1), ("var", 2), ("add", 0, 1), ("mul", 2, 3), ("add", 0, 4)]  # a + s (a + b)
SMALL = [("var", 0), ("var", 1), ("mul", 0, 1), ("add", 2, 0)]  # t0 t1 + t0


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    with binius_amd.Context(0, 1 << 18) as h:
        yield h


def upload(hal, alloc, values, level):
    packed = T.pack(values, level)
    d = alloc.alloc(packed.shape[0])
    hal.copy_h2d(packed, d)
    return d


@pytest.fixture(scope="module")
def table():
    """the given columns' values and every derived column's, from the restatement: computed once"""
    rng = np.random.default_rng(0x3A11)
    a = [T.random_values(rng, 0, 1 << N_VARS) for _ in range(32)]
    b = [T.random_values(rng, 0, 1 << N_VARS) for _ in range(32)]
    s = T.random_values(rng, 0, 1 << N_VARS)
    t = [T.random_values(rng, 0, 16) for _ in range(2)]
    sel = [T.evaluate(SELECT, [(a[k], 0), (b[k], 0), (s, 0)], 0) for k in range(32)]
    packed = T.evaluate(T.pack_steps(32), [(c, 0) for c in sel], 5)
    assert U.to_ints(packed) == [sum(int(sel[k][r]) << k for k in range(32)) for r in range(1 << N_VARS)]
    return {"a": a, "b": b, "s": s, "t": t, "sel": sel, "packed": packed, "shifted": D.shifted(sel[0], 5, 3, D.LOGICAL_LEFT), "small": T.evaluate(SMALL, [(t[0], 0), (t[1], 0)], 0)}


def columns_of(hal, alloc, table):
    given = table["a"] + table["b"] + [table["s"]]
    cols = [("given", upload(hal, alloc, v, 0), 0, N_VARS) for v in given]                      # 0 .. 31: a, 32 .. 63: b, 64: s
    cols += [("computed", SELECT, [k, 32 + k, 64], N_VARS, 0) for k in range(32)]                 # 65 .. 96: wave 1, one call each
    cols.append(("lincomb", [(65 + k, 1 << k) for k in range(32)], 0, N_VARS))                     # 97: pack_fp at B32, wave 2
    cols.append(("shifted", 65, 5, 3, "logical_left"))                                            # 98: of a computed column, wave 2
    cols += [("given", upload(hal, alloc, v, 0), 0, 4) for v in table["t"]]                       # 99, 100: 16 bits each
    cols.append(("computed", SMALL, [99, 100], 4, 0))                                             # 101: below one element: host work, wave 1
    return cols


def test_mul_shaped_table(hal, table):
    from binius_amd._host import WitnessCompute

    alloc = hal.dev_alloc()
    cols = columns_of(hal, alloc, table)
    want = {65 + k: (table["sel"][k], 0) for k in range(32)}
    want.update({97: (table["packed"], 5), 98: (table["shifted"], 0), 101: (table["small"], 0)})
    n_scratch = WitnessCompute.scratch_elems(cols)
    assert n_scratch == 32 * 2 + (1 << N_VARS) * 32 // 128 + 2 + 1  # the composites, the packed column, the shifted one, one element of host work
    scratch = alloc.alloc(n_scratch)
    for _ in range(2):  # resident inputs, run twice: the same values
        before = hal.compute_composite_counters(), hal.derive_counters()
        plan = WitnessCompute(hal, cols, scratch)
        got = plan.run()
        # waves: the composites 1, what reads them 2; launches: 32 composites + pack_fp (bn_compute_composite each) + one derive call
        assert plan.n_waves == 2 and plan.n_launches == 32 + 1 + 1
        after = hal.compute_composite_counters(), hal.derive_counters()
        assert {k: after[0][k] - before[0][k] for k in after[0]} == {"calls": 33, "launches": 33, "bitwise": 32, "values": 1}
        assert after[1]["calls"] - before[1]["calls"] == 1
        for i, (vals, level) in want.items():
            d, got_level, got_n_vars = got[i]
            assert got_level == level and 1 << got_n_vars == len(vals), i
            body = hal.copy_d2h(d)
            if len(vals) << level < 128:  # below one element: the values, in the low bits of the element
                mask = (1 << (len(vals) << level)) - 1
                assert (int(body[0][0]) | (int(body[0][1]) << 64)) & mask == int(T.pack(vals, level)[0][0]) & mask, "column %d differs from the restatement" % i
            else:
                assert np.array_equal(body, T.pack(vals, level)), "column %d differs from the restatement" % i
        for i, v in enumerate(table["a"] + table["b"] + [table["s"]]):
            assert got[i][0].ptr == cols[i][1].ptr and np.array_equal(hal.copy_d2h(cols[i][1]), T.pack(v, 0)), "an input was modified"


def test_the_build_plan_rejects_the_same_plan(hal, table):
    import binius_amd._ffi as F
    from binius_amd._host import WitnessBuild

    alloc = hal.dev_alloc()
    cols = columns_of(hal, alloc, table)
    scratch = alloc.alloc(1 << 10)
    before = hal.compute_composite_counters()
    raw = [(13, i - 65 if i < 101 else 32, c[3], c[4]) if c[0] == "computed" else c for i, c in enumerate(cols)]  # (kind 13 as the header encodes it)
    assert WitnessBuild.scratch_elems(raw) == 0
    with pytest.raises(F.BnError) as e:
        WitnessBuild(hal, raw, scratch).run()
    assert e.value.kind == "InputValidation"
    # ... and pack_fp alone: a subfield combination outside the XOR form
    pack_only = cols[:32] + [("lincomb", [(k, 1 << k) for k in range(32)], 0, N_VARS)]
    assert WitnessBuild.scratch_elems(pack_only) == 0
    with pytest.raises(F.BnError) as e:
        WitnessBuild(hal, pack_only, scratch).run()
    assert e.value.kind == "InputValidation"
    assert hal.compute_composite_counters() == before


def test_a_combination_of_level_two_is_rejected(hal, table):
    import binius_amd._ffi as F
    from binius_amd._host import WitnessCompute

    alloc = hal.dev_alloc()
    d = upload(hal, alloc, table["s"], 0)
    cols = [("given", d, 0, N_VARS), ("lincomb", [(0, 4)], 0, N_VARS)]  # 4 lies in B4 \\ B2: the column would have tower level 2
    assert WitnessCompute.scratch_elems(cols) == 0
    before = hal.compute_composite_counters()
    with pytest.raises(F.BnError) as e:
        WitnessCompute(hal, cols, alloc.alloc(16)).run()
    assert e.value.kind == "InputValidation"
    assert hal.compute_composite_counters() == before
    # the same coefficient over a B8 column is a B8 combination: taken
    v = T.random_values(np.random.default_rng(7), 3, 1 << N_VARS)
    cols = [("given", upload(hal, alloc, v, 3), 3, N_VARS), ("lincomb", [(0, 4)], 9, N_VARS)]
    plan = WitnessCompute(hal, cols, alloc.alloc(WitnessCompute.scratch_elems(cols)))
    got = plan.run()
    assert (plan.n_waves, plan.n_launches) == (1, 1) and got[1][1:] == (3, N_VARS)
    steps = [("var", 0), ("const", 4), ("mul", 0, 1), ("const", 9), ("add", 2, 3)]
    assert np.array_equal(hal.copy_d2h(got[1][0]), T.evaluate_packed(steps, [(v, 3)], 3))
