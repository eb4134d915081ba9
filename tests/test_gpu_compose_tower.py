"""bn_compute_composite with a tower-typed expression (bn_expr_compile_tower; csrc/compose_tower.hpp, kernels_compose_tower.hip) against
tests/compose_tower_ref.py, bit for bit -- never against the device's own output.  Every input and the output sit at an odd 16-byte base
between canary frames (tests/adversarial.py); inputs must be unchanged after the call; every call runs twice from resident inputs, and
every accepted call moves the counters by exactly one launch.  Shapes are the smallest at which a path can go wrong: one output element
(an input of a lower level is then below one element), one workgroup's share of output elements, and more than one workgroup."""
import ctypes as C

import numpy as np
import pytest

import adversarial as A
import compose_tower_ref as T

pytestmark = pytest.mark.gpu

ARENA = 6 << 20  # elements
UNIT_ELEMS = 1024  # output elements of one workgroup (kComposeUnitElems)
LEVELS = T.LEVELS
PAIRS = [(lo, hi) for hi in LEVELS for lo in LEVELS if lo <= hi]
# the multiplicative generators of the tower's fields (binary_field.rs:740-747)
GENERATOR = {0: 1, 3: 0x2D, 4: 0xE2DE, 5: 0x03E21CEA, 6: 0x070F870DCD9C1D88, 7: 0x2E895399AF449ACE499596F6E5FCCAFA}


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    with binius_amd.Context(0, ARENA) as h:
        yield h


def elems(level, n_values):
    return max(1, (n_values << level) >> 7)


def ones(level):
    return (1 << (1 << level)) - 1


def data(kind, level, n, seed):
    if kind == "zero":
        return T.constant(0, level, n)
    if kind == "ones":
        return T.constant(ones(level), level, n)
    if kind == "generator":
        return T.constant(GENERATOR[level], level, n)
    return T.random_values(np.random.default_rng([0xC7, level, n, seed]), level, n)


def run_case(hal, steps, cols, out_level, n_values, n_rows_extra=0):
    """Place, compile, compute twice; the output against the restatement, the inputs against what was uploaded, frames included, and
    the counters: one call, one launch, bitwise at level 0 and per value above."""
    alloc = hal.dev_alloc()
    placed, lead = [], 1
    for v, lv in cols:
        assert len(v) == n_values
        placed.append(A.place(hal, alloc, T.pack(v, lv), lead))
        lead = (lead + 2) % 16
    out, check_out = A.place(hal, alloc, elems(out_level, n_values), lead)
    want = T.evaluate_packed(steps, cols, out_level)
    assert want.shape[0] == elems(out_level, n_values)
    expr = hal.expr_compile_tower(steps, [lv for _, lv in cols], out_level)
    assert expr.n_vars() == len(cols)
    try:
        for _ in range(2):
            before = hal.compute_composite_counters()
            hal.compute_composite_tower([s for s, _ in placed] + [placed[0][0]] * n_rows_extra, out, expr, n_values)
            after = hal.compute_composite_counters()
            moved = {k: after[k] - before[k] for k in after}
            assert moved == {"calls": 1, "launches": 1, "bitwise": int(out_level == 0), "values": int(out_level != 0)}, moved
            check_out(want)
            for _, check in placed:
                check()
    finally:
        hal._exprs.remove(expr)
        expr.free()


# ---- 1. x * c + d for every pair of levels: one output element, a workgroup's share, two shares, four
@pytest.mark.parametrize("lo,hi", PAIRS)
@pytest.mark.parametrize("out_elems", [1, UNIT_ELEMS, 2 * UNIT_ELEMS, 4 * UNIT_ELEMS])
def test_affine_every_level_pair(hal, lo, hi, out_elems):
    n = (out_elems << 7) >> hi
    rng = np.random.default_rng([0xAF, lo, hi])
    c, d = (int.from_bytes(rng.bytes(16), "little") & ones(hi) for _ in range(2))
    c |= 1 << ((1 << hi) - 1)  # (the constants are of the output's level, not below)
    d |= 1 << ((1 << hi) - 1)
    steps = [("var", 0), ("const", c), ("mul", 0, 1), ("const", d), ("add", 2, 3)]
    run_case(hal, steps, [(data("random", lo, n, 1), lo)], hi, n)


# ---- 2. products of two inputs: every level, extreme data, the narrow operand on either side
@pytest.mark.parametrize("lo,hi", PAIRS)
def test_products_of_two_inputs(hal, lo, hi):
    n = (8 << 7) >> hi  # eight output elements
    steps = [("var", 0), ("var", 1), ("mul", 0, 1)]
    for kind in ("random", "zero", "ones", "generator"):
        a = data(kind, lo, n, 2)
        b = data("random" if kind in ("zero", "generator") else kind, hi, n, 3)
        run_case(hal, steps, [(a, lo), (b, hi)], hi, n)
        if lo != hi or kind == "generator":
            run_case(hal, steps, [(b, hi), (a, lo)], hi, n)


# ---- 3. powers
@pytest.mark.parametrize("level", [3, 6])
@pytest.mark.parametrize("exponent", [0, 1, 2, 3, 254, (1 << 64) - 1])
def test_powers(hal, level, exponent):
    n = (4 << 7) >> level
    for kind in ("random", "zero", "ones"):
        run_case(hal, [("var", 0), ("pow", 0, exponent)], [(data(kind, level, n, 4), level)], level, n)


@pytest.mark.parametrize("exponent", [0, 5])
def test_powers_at_b1(hal, exponent):
    run_case(hal, [("var", 0), ("pow", 0, exponent)], [(data("random", 0, 1 << 11, 5), 0)], 0, 1 << 11)


# ---- 4. constants of level 1 and 2, roots that hold no slot, a repeated variable, an unused input, dead steps
SMALL = {
    "const_levels_1_2": ([("var", 0), ("const", 2), ("mul", 0, 1), ("const", 9), ("mul", 2, 3), ("const", 1), ("add", 4, 5)], [3], 3),
    "root_var_upcast_b8_to_b32": ([("var", 0)], [3], 5),
    "root_const": ([("var", 0), ("const", 0xABCD)], [3], 4),
    "repeated_variable": ([("var", 0), ("mul", 0, 0), ("add", 1, 1), ("add", 2, 0), ("mul", 3, 3)], [3], 3),
    "unused_input": ([("var", 1), ("const", 3), ("mul", 0, 1)], [5, 3, 0], 3),
    "dead_steps": ([("var", 0), ("var", 1), ("mul", 0, 1), ("pow", 2, 77), ("add", 0, 1)], [3, 3], 3),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_circuits(hal, name):
    steps, levels, out_level = SMALL[name]
    n = 1 << 9
    run_case(hal, steps, [(data("random", lv, n, 6 + i), lv) for i, lv in enumerate(levels)], out_level, n)


def test_more_rows_than_inputs(hal):
    steps, levels, out_level = SMALL["dead_steps"]
    n = 1 << 9
    run_case(hal, steps, [(data("random", lv, n, 6 + i), lv) for i, lv in enumerate(levels)], out_level, n, n_rows_extra=2)


# ---- 5. gadget shapes at 2^10 rows
GADGETS = {
    "pack_fp_b32": (T.pack_steps(32), [0] * 32, 5),
    "pack_fp_b64": (T.pack_steps(64), [0] * 64, 6),
    "pack_b8": (T.pack_steps(8), [0] * 8, 3),
    "b1_select": ([("var", 0), ("var", 1), ("var", 2), ("add", 0, 1), ("mul", 2, 3), ("add", 0, 4)], [0, 0, 0], 0),  # a + s (a + b)
    "plus_one_b32": ([("var", 0), ("const", 1), ("add", 0, 1)], [5], 5),
    "five_term_sum_b1": ([("var", i) for i in range(5)] + [("add", 0, 1), ("add", 5, 2), ("add", 6, 3), ("add", 7, 4)], [0] * 5, 0),
}


@pytest.mark.parametrize("name", sorted(GADGETS))
def test_gadget_shapes(hal, name):
    steps, levels, out_level = GADGETS[name]
    n = 1 << 10
    assert name != "pack_fp_b32" or len(steps) == 127
    run_case(hal, steps, [(data("random", lv, n, 20 + i), lv) for i, lv in enumerate(levels)], out_level, n)


# ---- 6. slots
def balanced_sum_of_products(n_products):
    steps = [("var", i) for i in range(2 * n_products)]

    def build(lo, hi):
        if hi - lo == 1:
            steps.append(("mul", 2 * lo, 2 * lo + 1))
        else:
            a, b = build(lo, (lo + hi) // 2), build((lo + hi) // 2, hi)
            steps.append(("add", a, b))
        return len(steps) - 1

    build(0, n_products)
    return steps


def products_then_sum(n_products):
    """every product before the first sum: n_products values are alive at once"""
    steps = [("var", i) for i in range(2 * n_products)] + [("mul", 2 * i, 2 * i + 1) for i in range(n_products)]
    acc = 2 * n_products
    for i in range(1, n_products):
        steps.append(("add", acc, 2 * n_products + i))
        acc = len(steps) - 1
    return steps


def test_balanced_sum_of_32_products(hal):
    n = 1 << 7
    run_case(hal, balanced_sum_of_products(32), [(data("random", 4, n, 40 + i), 4) for i in range(64)], 4, n)


def test_sixteen_live_slots_run_and_seventeen_are_rejected(hal):
    import binius_amd._ffi as F

    n = 1 << 7
    run_case(hal, products_then_sum(15), [(data("random", 4, n, 40 + i), 4) for i in range(30)], 4, n)  # 15 products + the running sum
    with pytest.raises(F.BnError) as e:
        hal.expr_compile_tower(products_then_sum(17), [4] * 34, 4)
    assert e.value.kind == "InputValidation"


def test_left_deep_pack_into_b128(hal):
    steps = T.pack_steps(128)
    assert len(steps) == 511
    n = 1 << 7
    run_case(hal, steps, [(data("random", 0, n, 60 + i), 0) for i in range(128)], 7, n)


# ---- 7. seeded random DAGs over mixed levels
def random_dag(seed):
    rng = np.random.default_rng([0xDA6, seed])
    out_level = LEVELS[rng.integers(0, 6)]
    levels = [int(rng.choice([lv for lv in LEVELS if lv <= out_level])) for _ in range(rng.integers(1, 5))]
    steps = []
    for s in range(int(rng.integers(1, 25))):
        k = int(rng.integers(0, 2)) if s < 2 else int(rng.integers(0, 7))
        if k == 0:
            steps.append(("var", int(rng.integers(0, len(levels)))))
        elif k == 1:
            steps.append(("const", int.from_bytes(rng.bytes(16), "little") & ones(int(rng.integers(0, out_level + 1)))))
        elif k <= 3:
            steps.append(("add", int(rng.integers(0, s)), int(rng.integers(0, s))))
        elif k <= 5:
            steps.append(("mul", int(rng.integers(0, s)), int(rng.integers(0, s))))
        else:
            steps.append(("pow", int(rng.integers(0, s)), int(rng.integers(0, 9)) if rng.integers(0, 5) else int(rng.integers(0, 1 << 63)) * 2 + 1))
    return steps, levels, out_level


@pytest.mark.parametrize("seed", range(40))
def test_random_dags(hal, seed):
    steps, levels, out_level = random_dag(seed)
    n = 1 << 10
    run_case(hal, steps, [(data("random", lv, n, 80 + i), lv) for i, lv in enumerate(levels)], out_level, n)


# ---- 8. the invalid tables
INVALID_EXPR = {
    "no_steps": ([], [3], 3),
    "too_many_steps": ([("var", 0)] * 1025, [3], 3),
    "too_many_inputs": ([("var", 0)], [0] * 257, 3),
    "operand_not_earlier": ([("var", 0), ("add", 0, 1)], [3], 3),
    "pow_base_not_earlier": ([("var", 0), ("pow", 1, 2)], [3], 3),
    "var_index": ([("var", 1)], [3], 3),
    "input_level_1": ([("var", 0)], [1], 3),
    "input_level_2": ([("var", 0)], [2], 3),
    "input_level_8": ([("var", 0)], [8], 7),
    "output_level_1": ([("const", 1)], [0], 1),
    "output_level_2": ([("const", 1)], [0], 2),
    "output_level_8": ([("var", 0)], [3], 8),
    "input_above_output": ([("var", 0)], [5], 3),
    "constant_above_output": ([("var", 0), ("const", 256), ("add", 0, 1)], [3], 3),
    "too_many_live_slots": (products_then_sum(17), [4] * 34, 4),
}


@pytest.mark.parametrize("case", sorted(INVALID_EXPR))
def test_invalid_expressions_are_rejected(hal, case):
    import binius_amd._ffi as F

    steps, levels, out_level = INVALID_EXPR[case]
    n_exprs = len(hal._exprs)
    with pytest.raises(F.BnError) as e:
        hal.expr_compile_tower(steps, levels, out_level)
    assert e.value.kind == "InputValidation", case
    assert len(hal._exprs) == n_exprs


def test_unknown_kind_and_null_arguments_are_rejected(hal):
    import binius_amd._ffi as F

    L = F.lib()
    st = F.make_steps([("var", 0), ("var", 0)])
    st[1].kind = 9
    lv = (C.c_uint32 * 1)(3)
    h = C.c_void_p()
    assert L.bn_expr_compile_tower(hal._h, st, 2, lv, 1, 3, C.byref(h)) == F.BN_ERR_INPUT_VALIDATION and not h.value
    assert L.bn_expr_compile_tower(hal._h, None, 2, lv, 1, 3, C.byref(h)) == F.BN_ERR_INPUT_VALIDATION and not h.value
    assert L.bn_expr_compile_tower(hal._h, st, 1, None, 1, 3, C.byref(h)) == F.BN_ERR_INPUT_VALIDATION and not h.value
    assert L.bn_expr_compile_tower(hal._h, st, 1, lv, 1, 3, None) == F.BN_ERR_INPUT_VALIDATION
    assert L.bn_expr_compile_tower(None, st, 1, lv, 1, 3, C.byref(h)) == F.BN_ERR_INPUT_VALIDATION and not h.value


@pytest.fixture()
def valid_call(hal):
    """a + b at B8 over 2^9 values, computed once: (expr, [input slices], out slice, check_out, want, n)"""
    n = 1 << 9
    steps = [("var", 0), ("var", 1), ("add", 0, 1)]
    cols = [(data("random", 3, n, 90), 3), (data("random", 3, n, 91), 3)]
    alloc = hal.dev_alloc()
    ins = [A.place(hal, alloc, T.pack(v, lv), 1 + 2 * i)[0] for i, (v, lv) in enumerate(cols)]
    out, check_out = A.place(hal, alloc, elems(3, n), 7)
    expr = hal.expr_compile_tower(steps, [3, 3], 3)
    hal.compute_composite_tower(ins, out, expr, n)
    want = T.evaluate_packed(steps, cols, 3)
    check_out(want)
    yield expr, ins, out, check_out, want, n
    hal._exprs.remove(expr)
    expr.free()


def _raw(hal, rows, n_rows, row_len, out_ptr, out_len, expr):
    import binius_amd._ffi as F

    arr = (C.c_void_p * max(1, len(rows)))(*rows) if rows is not None else None
    return F.lib().bn_compute_composite(hal._h, arr, n_rows, row_len, out_ptr, out_len, expr.handle)


INVALID_CALL = {
    "lengths_differ": lambda ins, out, n: (ins, 2, n, out, n // 2),
    "not_a_power_of_two": lambda ins, out, n: (ins, 2, n - 1, out, n - 1),
    "output_below_one_element": lambda ins, out, n: (ins, 2, 8, out, 8),
    "zero_values": lambda ins, out, n: (ins, 2, 0, out, 0),
    "fewer_rows_than_inputs": lambda ins, out, n: (ins[:1], 1, n, out, n),
    "null_rows": lambda ins, out, n: (None, 2, n, out, n),
    "null_row": lambda ins, out, n: ([ins[0], None], 2, n, out, n),
    "null_output": lambda ins, out, n: (ins, 2, n, None, n),
    "misaligned_row": lambda ins, out, n: ([ins[0], ins[1] + 8], 2, n, out, n),
    "misaligned_output": lambda ins, out, n: (ins, 2, n, out + 4, n),
    "output_is_a_row": lambda ins, out, n: ([ins[0], out], 2, n, out, n),
    "output_overlaps_a_row": lambda ins, out, n: ([ins[0], out + 16 * (n // 16 - 1)], 2, n, out, n),
}


@pytest.mark.parametrize("case", sorted(INVALID_CALL))
def test_invalid_calls_are_rejected(hal, valid_call, case):
    import binius_amd._ffi as F

    expr, ins, out, check_out, want, n = valid_call
    rows, n_rows, row_len, out_ptr, out_len = INVALID_CALL[case]([s.ptr for s in ins], out.ptr, n)
    before = hal.compute_composite_counters()
    assert _raw(hal, rows, n_rows, row_len, out_ptr, out_len, expr) == F.BN_ERR_INPUT_VALIDATION, case
    assert hal.compute_composite_counters() == before
    check_out(want)  # nothing was launched: the output still holds the valid call's values, the frames are intact


def test_other_consumers_reject_a_tower_expression(hal, valid_call):
    import binius_amd._ffi as F

    expr, ins, out, check_out, want, n = valid_call
    alloc = hal.dev_alloc()
    a = alloc.alloc(1 << 6)
    hal.fill(a, 1)
    before = hal.compute_composite_counters()

    def kernel(ke, log_chunks, bufs):
        acc = ke.decl_value(0)
        ke.sum_composition_evals([bufs[0].to_ref(), bufs[0].to_ref()], expr, 1, acc)
        return [acc]

    with pytest.raises(F.BnError) as e:
        hal.accumulate_kernels(kernel, [("chunked", a, 0)])
    assert e.value.kind == "InputValidation"
    plain = hal.compile_expr([("var", 0), ("var", 1), ("mul", 0, 1)])
    for comp, inf in ((expr, plain), (plain, expr)):
        with pytest.raises(F.BnError) as e:
            hal.hal_round_evals(1, 6, None, [("folded", a, 0), ("folded", a, 0)],
                                [{"composition": comp, "composition_at_infinity": inf, "start": 1, "end": 3, "eq_ind": None}], [])
        assert e.value.kind == "InputValidation"
    assert hal.compute_composite_counters() == before


# ---- 9. the plain B128 route is untouched and counts nowhere
def test_plain_expressions_do_not_move_the_counters(hal):
    import oracle

    n = 1 << 8
    alloc = hal.dev_alloc()
    rows = [oracle.random_b128(0xCC00 + i, n) for i in range(3)]
    d = []
    for r in rows:
        s = alloc.alloc(n)
        hal.copy_h2d(r, s)
        d.append(s)
    out = alloc.alloc(n)
    steps = [("var", 0), ("var", 1), ("var", 2), ("add", 0, 1), ("mul", 2, 3), ("add", 0, 4)]
    expr = hal.compile_expr(steps)
    before = hal.compute_composite_counters()
    hal.compute_composite(d, out, expr)
    assert hal.compute_composite_counters() == before
    want = np.zeros((n, 2), dtype=np.uint64)
    assert oracle.compute_composite(rows, want, steps) == 0
    assert np.array_equal(hal.copy_d2h(out), want)
