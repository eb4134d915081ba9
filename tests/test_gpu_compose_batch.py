"""bn_compute_composite with a BATCH of tower-typed expressions (bn_expr_compile_tower_batch; csrc/compose_batch.hpp,
k_compose_tower_batch of kernels_compose_tower.hip) against tests/compose_tower_ref.py, bit for bit -- never against the device's own
output.  Every row and the output arena sit at an odd 16-byte base between canary frames (tests/adversarial.py); the arena is filled
with the canary too, so the elements before, between and after the jobs' outputs must still hold it after the call.  Inputs must be
unchanged; every accepted call moves the batch counters by one call and one launch and the old tower counters not at all; a rejected
call moves neither and writes nothing.  Sizes are the smallest at which a path can go wrong: one output element, exactly one unit
(1024 output elements, one workgroup) and two units, mixed in one table and not in ascending order."""
import ctypes as C

import numpy as np
import pytest

import adversarial as A
import compose_tower_ref as T

pytestmark = pytest.mark.gpu

ARENA = 8 << 20  # elements
UNIT_ELEMS = 1024  # output elements of one workgroup (kComposeUnitElems)
SELECT = [("var", 0), ("var", 1), ("var", 2), ("add", 0, 1), ("mul", 2, 3), ("add", 0, 4)]  # a + s (a + b), mul.rs:466-489
CANARY = np.array([A.CANARY & A.M64, A.CANARY >> 64], dtype=np.uint64)


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    with binius_amd.Context(0, ARENA) as h:
        yield h


def elems(level, n_values):
    return max(1, (n_values << level) >> 7)


def products_then_sum(k):
    """k independent products of input pairs, every one before the first sum: k + 1 slots are live at the first sum (k = 1: the
    product plus its first input)"""
    steps = [("var", i) for i in range(2 * k)] + [("mul", 2 * i, 2 * i + 1) for i in range(k)]
    steps.append(("add", 2 * k, 0 if k == 1 else 2 * k + 1))
    for i in range(2, k):
        steps.append(("add", len(steps) - 1, 2 * k + i))
    return steps


class Batch:
    """Rows placed one by one, jobs laid out in one canary-filled arena with gaps of 1, 2, 3 elements before and between them.
    members: [(steps, input levels, out level)]; add_rows([(values, level), ...]) -> first_row; add_job(member, first_row, n_values)."""

    def __init__(self, hal, members, arena_elems, lead=5):
        self.hal, self.members, self.alloc = hal, members, hal.dev_alloc()
        self.rows, self.cols, self.checks, self.jobs, self.want_jobs = [], [], [], [], []
        self.arena, self.check_arena = A.place(hal, self.alloc, arena_elems, lead)
        self.want = np.tile(CANARY, (arena_elems, 1))
        self.top = 1
        self.exprs = [hal.expr_compile_tower(*m) for m in members]
        self.batch = None

    def add_rows(self, cols):
        first = len(self.rows)
        for v, lv in cols:
            s, check = A.place(self.hal, self.alloc, T.pack(v, lv), 1 + 2 * (len(self.rows) % 8))
            self.rows.append(s)
            self.cols.append((v, lv))
            self.checks.append(check)
        return first

    def add_job(self, member, first_row, n_values, want=None):
        steps, levels, out_level = self.members[member]
        n = elems(out_level, n_values)
        off = self.top
        self.top += n + 1 + len(self.jobs) % 3
        assert self.top <= self.arena.len
        if want is None:
            want = T.evaluate_packed(steps, self.cols[first_row : first_row + len(levels)], out_level)
        assert want.shape[0] == n
        self.want[off : off + n] = want
        self.jobs.append((member, first_row, n_values.bit_length() - 1, off))
        return off

    def compile(self):
        self.batch = self.hal.expr_compile_tower_batch(self.exprs, self.jobs)
        for e in self.exprs:  # the batch holds copies: the members go at once
            self.hal._exprs.remove(e)
            e.free()
        self.exprs = []
        return self.batch

    def run(self, programs, times=2):
        if self.batch is None:
            self.compile()
        assert self.batch.n_vars() == max(f + len(self.members[m][1]) for m, f, _, _ in self.jobs)
        for _ in range(times):
            before, old = self.hal.compute_composite_batch_counters(), self.hal.compute_composite_counters()
            self.hal.compute_composite_tower_batch(self.rows, self.arena, self.batch)
            after = self.hal.compute_composite_batch_counters()
            assert {k: after[k] - before[k] for k in after} == {"calls": 1, "launches": 1, "jobs": len(self.jobs), "programs": programs}
            assert self.hal.compute_composite_counters() == old, "a batch call moved the old tower counters"
            self.check()

    def check(self):
        self.check_arena(self.want)
        for check in self.checks:
            check()

    def close(self):
        for e in self.exprs + ([self.batch] if self.batch is not None else []):
            self.hal._exprs.remove(e)
            e.free()
        self.exprs, self.batch = [], None


def rnd_cols(seed, levels, n):
    rng = np.random.default_rng([0xCB, seed, n])
    return [(T.random_values(rng, lv, n), lv) for lv in levels]


# ---- 1. classes Q = 4 / 2 / 1, output levels 0 / 3 / 5 / 7 over inputs of lower levels, one element / one unit / two units
def test_mixed_batch(hal):
    members = [
        (SELECT, [0, 0, 0], 0),                                # 2 slots, Q = 4, bitwise
        (products_then_sum(4), [0, 3] * 4, 3),                 # 5 slots, Q = 2, spread 0 -> 3
        (products_then_sum(8), [0, 5] * 8, 5),                 # 9 slots, Q = 1, spread 0 -> 5
        (products_then_sum(1), [3, 7], 7),                     # 2 slots, Q = 4, spread 3 -> 7
        (products_then_sum(15), [3, 0] * 15, 3),               # 16 slots, Q = 1: the launch's LDS is 64 KiB
    ]
    sizes = [(1, 2 * UNIT_ELEMS), (0, 1), (2, UNIT_ELEMS), (3, 1), (0, 2 * UNIT_ELEMS), (4, 1), (3, UNIT_ELEMS), (1, 1), (2, 1), (0, UNIT_ELEMS), (3, 2 * UNIT_ELEMS),
             (4, UNIT_ELEMS)]
    b = Batch(hal, members, sum(n + 3 for _, n in sizes) + 2)
    try:
        for j, (m, out_elems) in enumerate(sizes):
            n_values = (out_elems << 7) >> members[m][2]
            b.add_job(m, b.add_rows(rnd_cols(j, members[m][1], n_values)), n_values)
        b.run(programs=5)
    finally:
        b.close()


# ---- 2. 33 jobs, one program: the mul shape at 2^8 and 2^13 bits; members compiled twice from the same steps collapse
@pytest.mark.parametrize("n_vars", [8, 13])
def test_shared_program(hal, n_vars):
    n = 1 << n_vars
    b = Batch(hal, [(SELECT, [0, 0, 0], 0), (list(SELECT), [0, 0, 0], 0)], 33 * (elems(0, n) + 3) + 2)
    try:
        for j in range(33):
            b.add_job(j % 2, b.add_rows(rnd_cols(100 + j, [0, 0, 0], n)), n)
        b.run(programs=1)
    finally:
        b.close()


# ---- 3. a row read by three jobs; a job whose input lies in the arena, written by an earlier call
def test_rows_reused_and_rows_inside_the_arena(hal):
    n = 1 << 11
    product = ([("var", 0), ("var", 1), ("mul", 0, 1)], [3, 3], 3)
    first = Batch(hal, [(SELECT, [0, 0, 0], 0), product], 4096, lead=3)
    try:
        r = first.add_rows(rnd_cols(1, [0, 0, 0, 0], n) + rnd_cols(2, [3, 3, 3], n))
        first.add_job(0, r, n)          # rows 0 1 2
        first.add_job(0, r + 1, n)      # rows 1 2 3: rows 1 and 2 are read by ...
        first.add_job(0, r, n)          # ... three jobs
        x_off = first.add_job(1, r + 4, n)  # x = rows 4 * 5 at B8
        first.add_job(1, r + 5, n)      # rows 5 6
        first.run(programs=2)
        # a second call on the SAME arena: its job reads x where the first call wrote it and writes behind everything
        x_vals = T.evaluate(product[0], first.cols[r + 4 : r + 6], 3)
        x = first.arena.slice(x_off, x_off + elems(3, n))
        again = hal.expr_compile_tower(*product)
        y_off = first.top + 2
        batch = hal.expr_compile_tower_batch([again], [(0, len(first.rows) - 1, n.bit_length() - 1, y_off)])  # rows: [.., row 6, x]
        try:
            before = hal.compute_composite_batch_counters()
            hal.compute_composite_tower_batch(first.rows + [x], first.arena, batch)
            after = hal.compute_composite_batch_counters()
            assert {k: after[k] - before[k] for k in after} == {"calls": 1, "launches": 1, "jobs": 1, "programs": 1}
            first.want[y_off : y_off + elems(3, n)] = T.evaluate_packed(product[0], [first.cols[r + 6], (x_vals, 3)], 3)
            first.check()
        finally:
            for e in (again, batch):
                hal._exprs.remove(e)
                e.free()
    finally:
        first.close()


# ---- 4. pack_fp into B32 from 32 B1 columns at 2^8 values, beside a B32 x B32 product and a POW
def test_pack_fp_beside_a_product_and_a_power(hal):
    n = 1 << 8
    members = [(T.pack_steps(32), [0] * 32, 5), ([("var", 0), ("var", 1), ("mul", 0, 1)], [5, 5], 5), ([("var", 0), ("pow", 0, 0xFFFFFFFE)], [5], 5)]
    b = Batch(hal, members, 3 * (elems(5, n) + 3) + 2)
    try:
        for m, (_, levels, _) in enumerate(members):
            b.add_job(m, b.add_rows(rnd_cols(200 + m, levels, n)), n)
        b.run(programs=3)
    finally:
        b.close()


# ---- 5. what the call rejects: nothing launched, nothing written, no counter moved
@pytest.fixture()
def valid_batch(hal):
    """two jobs: select over 2^10 bits (8 elements, rows 0 1 2), a B32 product over 2^3 values (2 elements, rows 3 4); run once"""
    b = Batch(hal, [(SELECT, [0, 0, 0], 0), ([("var", 0), ("var", 1), ("mul", 0, 1)], [5, 5], 5)], 64)
    b.add_job(0, b.add_rows(rnd_cols(300, [0, 0, 0], 1 << 10)), 1 << 10)
    b.add_job(1, b.add_rows(rnd_cols(301, [5, 5], 1 << 3)), 1 << 3)
    b.run(programs=2, times=1)
    yield b
    b.close()


def _raw(hal, rows, n_rows, row_len, out_ptr, out_len, expr):
    import binius_amd._ffi as F

    arr = (C.c_void_p * max(1, len(rows)))(*rows) if rows is not None else None
    return F.lib().bn_compute_composite(hal._h, arr, n_rows, row_len, out_ptr, out_len, expr.handle)


def _swap(rows, i, value):
    return rows[:i] + [value] + rows[i + 1 :]


# (rows, arena pointer, arena elements, job offsets) -> (rows, n_rows, row_len, out pointer, out_len)
INVALID_CALL = {
    "output_overlaps_a_row_of_its_job": lambda r, out, n, off: (_swap(r, 1, out + 16 * (off[0] + 7)), 5, n, out, n),
    "output_overlaps_a_row_of_another_job": lambda r, out, n, off: (_swap(r, 4, out + 16 * off[0]), 5, n, out, n),
    "a_rows_tail_overlaps_an_output": lambda r, out, n, off: (_swap(r, 0, out + 16 * (off[1] - 7)), 5, n, out, n),
    "range_leaves_the_arena": lambda r, out, n, off: (r, 5, off[1] + 1, out, off[1] + 1),
    "offset_leaves_the_arena": lambda r, out, n, off: (r, 5, off[0], out, off[0]),
    "n_rows_too_small": lambda r, out, n, off: (r[:4], 4, n, out, n),
    "row_len_differs_from_out_len": lambda r, out, n, off: (r, 5, n // 2, out, n),
    "row_len_is_the_number_of_values": lambda r, out, n, off: (r, 5, 1 << 10, out, n),
    "misaligned_row": lambda r, out, n, off: (_swap(r, 2, r[2] + 8), 5, n, out, n),
    "null_row": lambda r, out, n, off: (_swap(r, 3, None), 5, n, out, n),
    "null_rows": lambda r, out, n, off: (None, 5, n, out, n),
    "null_arena": lambda r, out, n, off: (r, 5, n, None, n),
    "misaligned_arena": lambda r, out, n, off: (r, 5, n, out + 4, n),
}


@pytest.mark.parametrize("case", sorted(INVALID_CALL))
def test_invalid_calls_are_rejected(hal, valid_batch, case):
    import binius_amd._ffi as F

    b = valid_batch
    rows, n_rows, row_len, out_ptr, out_len = INVALID_CALL[case]([s.ptr for s in b.rows], b.arena.ptr, b.arena.len, [j[3] for j in b.jobs])
    hal.fill(b.arena, A.CANARY)  # the fill pattern: a rejected call leaves it
    b.want[:] = CANARY
    before = hal.compute_composite_batch_counters(), hal.compute_composite_counters()
    assert _raw(hal, rows, n_rows, row_len, out_ptr, out_len, b.batch) == F.BN_ERR_INPUT_VALIDATION, case
    assert (hal.compute_composite_batch_counters(), hal.compute_composite_counters()) == before
    b.check()


def test_a_batch_is_rejected_by_the_other_consumers(hal, valid_batch):
    import binius_amd._ffi as F

    b = valid_batch
    a = b.alloc.alloc(1 << 6)
    hal.fill(a, 1)
    hal.fill(b.arena, A.CANARY)
    b.want[:] = CANARY
    before = hal.compute_composite_batch_counters(), hal.compute_composite_counters()

    def kernel(ke, log_chunks, bufs):
        acc = ke.decl_value(0)
        ke.sum_composition_evals([bufs[0].to_ref(), bufs[0].to_ref()], b.batch, 1, acc)
        return [acc]

    with pytest.raises(F.BnError) as e:
        hal.accumulate_kernels(kernel, [("chunked", a, 0)])
    assert e.value.kind == "InputValidation"
    plain = hal.compile_expr([("var", 0), ("var", 1), ("mul", 0, 1)])
    for comp, inf in ((b.batch, plain), (plain, b.batch)):
        with pytest.raises(F.BnError) as e:
            hal.hal_round_evals(1, 6, None, [("folded", a, 0), ("folded", a, 0)],
                                [{"composition": comp, "composition_at_infinity": inf, "start": 1, "end": 3, "eq_ind": None}], [])
        assert e.value.kind == "InputValidation"
    assert (hal.compute_composite_batch_counters(), hal.compute_composite_counters()) == before
    b.check()


# ---- 6. what the compiler of a batch rejects, through the library (the plan's own cases run on the CPU: tests/cpp/compose_batch_check.cpp)
def test_invalid_batches_are_rejected(hal):
    import binius_amd._ffi as F

    sel = hal.expr_compile_tower(SELECT, [0, 0, 0], 0)
    b32 = hal.expr_compile_tower([("var", 0), ("var", 1), ("mul", 0, 1)], [5, 5], 5)
    plain = hal.compile_expr([("var", 0), ("var", 1), ("mul", 0, 1)])
    good = hal.expr_compile_tower_batch([sel, b32], [(0, 0, 10, 0), (1, 3, 3, 8)])
    assert good.n_vars() == 5
    nested = [good]
    cases = {
        "no_jobs": ([sel], []),
        "too_many_jobs": ([sel], [(0, 0, 7, j) for j in range(F.BN_COMPOSE_BATCH_MAX_JOBS + 1)]),
        "expr_index": ([sel, b32], [(2, 0, 10, 0)]),
        "plain_member": ([sel, plain], [(0, 0, 10, 0)]),
        "batch_as_member": (nested, [(0, 0, 10, 0)]),
        "reserved": ([sel], [(0, 0, 10, 0, 1)]),
        "n_vars_above_the_cap": ([sel], [(0, 0, 41, 0)]),
        "below_one_element": ([sel], [(0, 0, 6, 0)]),
        "below_one_element_b32": ([b32], [(0, 0, 1, 0)]),
        "outputs_overlap": ([sel, b32], [(0, 0, 10, 0), (1, 3, 3, 7)]),
        "units_leave_31_bits": ([b32], [(0, 0, 40, j << 38) for j in range(8)]),
    }
    n_exprs = len(hal._exprs)
    try:
        for name, (members, jobs) in cases.items():
            with pytest.raises(F.BnError) as e:
                hal.expr_compile_tower_batch(members, jobs)
            assert e.value.kind == "InputValidation", name
            assert len(hal._exprs) == n_exprs, name
        L = F.lib()
        hs = (C.c_void_p * 1)(sel.handle)
        desc, offs = (C.c_uint32 * 4)(0, 0, 10, 0), (C.c_uint64 * 1)(0)
        h = C.c_void_p()
        assert L.bn_expr_compile_tower_batch(hal._h, None, 1, desc, offs, 1, C.byref(h)) == F.BN_ERR_INPUT_VALIDATION and not h.value
        assert L.bn_expr_compile_tower_batch(hal._h, hs, 1, None, offs, 1, C.byref(h)) == F.BN_ERR_INPUT_VALIDATION and not h.value
        assert L.bn_expr_compile_tower_batch(hal._h, hs, 1, desc, None, 1, C.byref(h)) == F.BN_ERR_INPUT_VALIDATION and not h.value
        assert L.bn_expr_compile_tower_batch(hal._h, hs, 1, desc, offs, 1, None) == F.BN_ERR_INPUT_VALIDATION
        assert L.bn_expr_compile_tower_batch(None, hs, 1, desc, offs, 1, C.byref(h)) == F.BN_ERR_INPUT_VALIDATION and not h.value
        hs[0] = None
        assert L.bn_expr_compile_tower_batch(hal._h, hs, 1, desc, offs, 1, C.byref(h)) == F.BN_ERR_INPUT_VALIDATION and not h.value
    finally:
        for e in (sel, b32, plain, good):
            hal._exprs.remove(e)
            e.free()
