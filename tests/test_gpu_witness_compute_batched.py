"""The batched compute plan (witness_compute_batched of binius_amd/host/witness.hpp, bnh_witness_compute_batched, WitnessComputeBatched):
the mul-shaped table of tests/test_gpu_witness_compute.py at 2^8 rows, with the expression columns of a wave in ONE launch
(bn_expr_compile_tower_batch) instead of one bn_compute_composite each.  Against tests/compose_tower_ref.py and tests/derive_ref.py
composed the same way, never against the per-column plan's output.  Waves, launches and both counter sets against hand counts; a second
table whose one wave mixes expressions of 2, 6 and 12 live slots at levels 0, 3 and 5; what the compute plan rejects."""
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
    rng = np.random.default_rng(0x3A12)
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
    cols += [("computed", SELECT, [k, 32 + k, 64], N_VARS, 0) for k in range(32)]                 # 65 .. 96: wave 1, ONE batch
    cols.append(("lincomb", [(65 + k, 1 << k) for k in range(32)], 0, N_VARS))                     # 97: pack_fp at B32, wave 2: a batch of one job
    cols.append(("shifted", 65, 5, 3, "logical_left"))                                            # 98: of a computed column, wave 2
    cols += [("given", upload(hal, alloc, v, 0), 0, 4) for v in table["t"]]                       # 99, 100: 16 bits each
    cols.append(("computed", SMALL, [99, 100], 4, 0))                                             # 101: below one element: host work, wave 1
    return cols


def compare(hal, got, i, vals, level):
    d, got_level, got_n_vars = got[i]
    assert got_level == level and 1 << got_n_vars == len(vals), i
    body = hal.copy_d2h(d)
    if len(vals) << level < 128:  # below one element: the values, in the low bits of the element
        mask = (1 << (len(vals) << level)) - 1
        assert (int(body[0][0]) | (int(body[0][1]) << 64)) & mask == int(T.pack(vals, level)[0][0]) & mask, "column %d differs from the restatement" % i
    else:
        assert np.array_equal(body, T.pack(vals, level)), "column %d differs from the restatement" % i


def test_mul_shaped_table(hal, table):
    from binius_amd._host import WitnessCompute, WitnessComputeBatched

    alloc = hal.dev_alloc()
    cols = columns_of(hal, alloc, table)
    want = {65 + k: (table["sel"][k], 0) for k in range(32)}
    want.update({97: (table["packed"], 5), 98: (table["shifted"], 0), 101: (table["small"], 0)})
    n_scratch = WitnessComputeBatched.scratch_elems(cols)
    assert n_scratch == WitnessCompute.scratch_elems(cols) == 32 * 2 + (1 << N_VARS) * 32 // 128 + 2 + 1
    scratch = alloc.alloc(n_scratch)
    for _ in range(2):  # resident inputs, run twice: the same values
        hal.fill(scratch, 0x5A)
        before = hal.compute_composite_batch_counters(), hal.compute_composite_counters(), hal.derive_counters()
        plan = WitnessComputeBatched(hal, cols, scratch)
        got = plan.run()
        # waves: the composites 1, what reads them 2; launches: the batch of wave 1, the batch of wave 2, one derive call
        assert plan.n_waves == 2 and plan.n_launches == 3
        after = hal.compute_composite_batch_counters(), hal.compute_composite_counters(), hal.derive_counters()
        assert {k: after[0][k] - before[0][k] for k in after[0]} == {"calls": 2, "launches": 2, "jobs": 33, "programs": 2}
        assert after[1] == before[1], "the batched plan moved the old tower counters"
        assert after[2]["calls"] - before[2]["calls"] == 1
        for i, (vals, level) in want.items():
            compare(hal, got, i, vals, level)
        for i, v in enumerate(table["a"] + table["b"] + [table["s"]]):
            assert got[i][0].ptr == cols[i][1].ptr and np.array_equal(hal.copy_d2h(cols[i][1]), T.pack(v, 0)), "an input was modified"


def products_then_sum(k):
    """k products of input pairs, all before the first sum: k + 1 live slots"""
    steps = [("var", i) for i in range(2 * k)] + [("mul", 2 * i, 2 * i + 1) for i in range(k)]
    steps.append(("add", 2 * k, 2 * k + 1))
    for i in range(2, k):
        steps.append(("add", len(steps) - 1, 2 * k + i))
    return steps


def test_one_wave_of_mixed_classes_and_levels(hal):
    """a 2-slot expression at B1, a 6-slot one at B8 over B1 and B8 columns, a 12-slot one at B32 over B1 and B32 columns: one wave, one
    launch whose LDS is the 12-slot job's"""
    from binius_amd._host import WitnessComputeBatched

    n_vars = 9
    rng = np.random.default_rng(0x3A13)
    alloc = hal.dev_alloc()
    levels = [0] * 3 + [0, 3] * 5 + [0, 5] * 11
    vals = [T.random_values(rng, lv, 1 << n_vars) for lv in levels]
    cols = [("given", upload(hal, alloc, v, lv), lv, n_vars) for v, lv in zip(vals, levels)]
    exprs = [(SELECT, [0, 1, 2], 0), (products_then_sum(5), list(range(3, 13)), 3), (products_then_sum(11), list(range(13, 35)), 5)]
    cols += [("computed", steps, ins, n_vars, lv) for steps, ins, lv in exprs]
    cols.append(("computed", SELECT, [2, 1, 0], n_vars, 0))  # the first program again, over other rows
    scratch = alloc.alloc(WitnessComputeBatched.scratch_elems(cols))
    before = hal.compute_composite_batch_counters(), hal.compute_composite_counters()
    plan = WitnessComputeBatched(hal, cols, scratch)
    got = plan.run()
    assert (plan.n_waves, plan.n_launches) == (1, 1)
    after = hal.compute_composite_batch_counters()
    assert {k: after[k] - before[0][k] for k in after} == {"calls": 1, "launches": 1, "jobs": 4, "programs": 3}
    assert hal.compute_composite_counters() == before[1]
    for i, (steps, ins, lv) in enumerate(exprs + [(SELECT, [2, 1, 0], 0)]):
        compare(hal, got, 35 + i, T.evaluate(steps, [(vals[v], levels[v]) for v in ins], lv), lv)


def test_the_batched_plan_rejects_what_the_compute_plan_rejects(hal, table):
    import binius_amd._ffi as F
    from binius_amd._host import WitnessComputeBatched

    alloc = hal.dev_alloc()
    d = upload(hal, alloc, table["s"], 0)
    g0 = ("given", d, 0, N_VARS)
    seventeen = [("var", i) for i in range(34)] + [("mul", 2 * i, 2 * i + 1) for i in range(17)]
    acc = 34
    for i in range(1, 17):
        seventeen.append(("add", acc, 34 + i))
        acc = len(seventeen) - 1
    rejected = {
        "a combination of level two": [g0, ("lincomb", [(0, 4)], 0, N_VARS)],
        "an offset of level one": [g0, ("lincomb", [(0, 1)], 2, N_VARS)],
        "an input that is not an earlier column": [g0, ("computed", SELECT, [0, 0, 1], N_VARS, 0)],
        "an input of another n_vars": [g0, ("given", d, 0, N_VARS - 1), ("computed", SELECT, [0, 0, 1], N_VARS, 0)],
        "a variable without an input": [g0, ("computed", SELECT, [0, 0], N_VARS, 0)],
        "a step above the column's level": [g0, ("computed", [("var", 0), ("const", 2), ("mul", 0, 1)], [0], N_VARS, 0)],
        "level 2": [g0, ("computed", [("var", 0)], [0], N_VARS, 2)],
        "an input above the column's level": [("given", d, 3, N_VARS - 3), ("computed", [("var", 0)], [0], N_VARS - 3, 0)],
        "no steps": [g0, ("computed", [], [0], N_VARS, 0)],
        "an operand that is not an earlier step": [g0, ("computed", [("var", 0), ("add", 0, 1)], [0], N_VARS, 0)],
        "17 live slots": [g0, ("computed", seventeen, [0] * 34, N_VARS, 0)],
    }
    scratch = alloc.alloc(64)
    before = hal.compute_composite_batch_counters(), hal.compute_composite_counters(), hal.derive_counters()
    for name, cols in rejected.items():
        assert WitnessComputeBatched.scratch_elems(cols) == 0, name
        with pytest.raises(F.BnError) as e:
            WitnessComputeBatched(hal, cols, scratch).run()
        assert e.value.kind == "InputValidation", name
    assert (hal.compute_composite_batch_counters(), hal.compute_composite_counters(), hal.derive_counters()) == before
    # the same coefficient over a B8 column is a B8 combination: taken, as a batch of one job
    v = T.random_values(np.random.default_rng(7), 3, 1 << N_VARS)
    cols = [("given", upload(hal, alloc, v, 3), 3, N_VARS), ("lincomb", [(0, 4)], 9, N_VARS)]
    plan = WitnessComputeBatched(hal, cols, alloc.alloc(WitnessComputeBatched.scratch_elems(cols)))
    got = plan.run()
    assert (plan.n_waves, plan.n_launches) == (1, 1) and got[1][1:] == (3, N_VARS)
    steps = [("var", 0), ("const", 4), ("mul", 0, 1), ("const", 9), ("add", 2, 3)]
    assert np.array_equal(hal.copy_d2h(got[1][0]), T.evaluate_packed(steps, [(v, 3)], 3))
