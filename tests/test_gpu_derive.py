"""bn_derive_columns_batch (csrc/kernels_derive.hip, abi_derive.cpp) against tests/derive_ref.py, bit for bit -- never against the device's
own output.  Every inner column, term and output sits at an odd 16-byte base between canary frames (tests/adversarial.py); inputs must be
unchanged after the call; every batch runs twice from resident inputs.  Shapes are the smallest at which a path can go wrong: both
sides of the 64-bit word, the 128-bit element and the 1024-element unit, in bit coordinates (a value of level l is 2^l bits)."""
import ctypes as C

import numpy as np
import pytest

import adversarial as A
import derive_ref as D

pytestmark = pytest.mark.gpu

ARENA = 6 << 20  # elements
UNIT_ELEMS = 4096  # outputs of one workgroup, taken 1024 at a time
VARIANTS = (D.CIRCULAR_LEFT, D.LOGICAL_LEFT, D.LOGICAL_RIGHT)
VARIANT_NAMES = {D.CIRCULAR_LEFT: "circular_left", D.LOGICAL_LEFT: "logical_left", D.LOGICAL_RIGHT: "logical_right"}


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    with binius_amd.Context(0, ARENA) as h:
        yield h


# ---- inputs: (level, n_vars, seed) -> values, computed once and never modified; seed "zero" / "ones": extreme data
_VALUES = {}


def values(key):
    if key not in _VALUES:
        level, n_vars, seed = key
        if seed == "zero":
            v = D.constant(0, level, 1 << n_vars)
        elif seed == "ones":
            v = D.constant((1 << (1 << level)) - 1, level, 1 << n_vars)
        else:
            v = D.random_values(np.random.default_rng([0xD1, level, n_vars, seed]), level, n_vars)
        v.setflags(write=False)
        _VALUES[key] = v
    return _VALUES[key]


def elems(level, n_vars):
    return max(1, (1 << (n_vars + level)) >> 7)


# ---- specs: what a job is, independent of where its columns live
def shift_spec(level, n_vars, block_size, shift_offset, variant, seed=0):
    return {"kind": "shifted", "level": level, "n_vars": n_vars, "block_size": block_size, "shift_offset": shift_offset, "variant": variant,
            "inputs": [(level, n_vars, seed)]}


def repeat_spec(level, n_vars, inner_n_vars, seed=0):
    return {"kind": "repeating", "level": level, "n_vars": n_vars, "inner_n_vars": inner_n_vars, "inputs": [(level, inner_n_vars, seed)]}


def pad_spec(level, inner_n_vars, n_pad_vars, start_index, nonzero_index, seed=0):
    return {"kind": "zero_padded", "level": level, "n_vars": inner_n_vars + n_pad_vars, "inner_n_vars": inner_n_vars, "start_index": start_index,
            "nonzero_index": nonzero_index, "inputs": [(level, inner_n_vars, seed)]}


def xor_spec(level, n_vars, seeds, offset=0):
    return {"kind": "xor", "level": level, "n_vars": n_vars, "offset": offset, "inputs": [(level, n_vars, s) for s in seeds]}


def expected(spec):
    ins = [values(k) for k in spec["inputs"]]
    if spec["kind"] == "shifted":
        return D.shifted(ins[0], spec["block_size"], spec["shift_offset"], spec["variant"])
    if spec["kind"] == "repeating":
        return D.repeating(ins[0], spec["n_vars"])
    if spec["kind"] == "zero_padded":
        return D.zero_padded(ins[0], spec["n_vars"] - spec["inner_n_vars"], spec["start_index"], spec["nonzero_index"])
    return D.xor_combination(ins, spec["offset"], spec["level"], spec["n_vars"])


def job_of(spec, out, inputs):
    """The dict Context.derive_columns_batch takes, from a spec, its output slice and its input slices."""
    jb = {k: v for k, v in spec.items() if k != "inputs"}
    jb["out"] = out
    if spec["kind"] == "shifted":
        jb["variant"] = VARIANT_NAMES[spec["variant"]]
    if spec["kind"] == "xor":
        jb["terms"] = inputs
    else:
        jb["inner"] = inputs[0]
    return jb


def run_batch(hal, specs):
    """Place, derive, compare every output with the restatement and every input with what was uploaded, frames included; twice."""
    alloc = hal.dev_alloc()
    placed, lead = {}, 1
    for spec in specs:
        for key in spec["inputs"]:
            if key not in placed:
                placed[key] = A.place(hal, alloc, D.pack(values(key), key[0]), lead)
                lead = (lead + 2) % 16
    outs = []
    for spec in specs:
        outs.append(A.place(hal, alloc, elems(spec["level"], spec["n_vars"]), lead))
        lead = (lead + 2) % 16
    jobs = [job_of(spec, out[0], [placed[k][0] for k in spec["inputs"]]) for spec, out in zip(specs, outs)]
    want = [D.pack(expected(spec), spec["level"]) for spec in specs]
    for _ in range(2):
        before = hal.derive_counters()
        hal.derive_columns_batch(jobs)
        after = hal.derive_counters()
        assert {k: after[k] - before[k] for k in after} == {"calls": 1, "launches": 1, "jobs": len(specs)}
        for i, (spec, (_, check)) in enumerate(zip(specs, outs)):
            try:
                check(want[i])
            except AssertionError as e:
                raise AssertionError("job %d %r: %s" % (i, spec, e)) from None
        for _, check in placed.values():
            check()
    return jobs, outs, want


# ---- shifted
def shift_specs(level, seed=0):
    """Block bits {2, 4, 32, 64, 128, 256, the whole column} as far as the level has them (a block is at least two values), offsets
    {1, half the block, block - 1}, all variants; at the smallest column that holds the block (at least one element), at eight elements
    (a unit with a tail) and at 2048 elements (two units)."""
    specs = []
    for out_elems in (1, 8, 2 * UNIT_ELEMS):
        n_vars = out_elems.bit_length() - 1 + 7 - level
        for block_bits in sorted({2, 4, 32, 64, 128, 256, out_elems * 128}):
            block_size = block_bits.bit_length() - 1 - level
            if block_size < 1 or block_size > n_vars:
                continue
            for shift_offset in sorted({1, (1 << block_size) // 2, (1 << block_size) - 1}):
                specs += [shift_spec(level, n_vars, block_size, shift_offset, variant, seed) for variant in VARIANTS]
    return specs


@pytest.mark.parametrize("level", [0, 3, 5, 7])
def test_shifted(hal, level):
    specs = shift_specs(level)
    assert len(specs) >= 24
    run_batch(hal, specs)


def test_shifted_offsets_that_are_no_multiple_of_a_word(hal):
    """Offsets inside a 64-bit word and across it, in blocks of two words up to two units of elements: the funnel's every alignment."""
    specs = []
    for n_vars, block_size in ((7, 7), (11, 8), (11, 11), (18, 9), (18, 18)):
        for shift_offset in (3, 63, 64, 65, 127):
            specs += [shift_spec(0, n_vars, block_size, shift_offset, variant, 1) for variant in VARIANTS]
    for shift_offset in (129, 1000, (1 << 18) - 129):  # whole elements and a remainder
        specs += [shift_spec(0, 18, 18, shift_offset, variant, 1) for variant in VARIANTS]
    run_batch(hal, specs)


# ---- repeating
def repeat_specs():
    """From an inner of 2, 8, 128 and 2^12 bits (as far as the level has them) to one element, 32 elements and two units."""
    specs = []
    for level in (0, 3, 5, 7):
        for inner_bits in (2, 8, 32, 128, 1 << 12):
            inner_n_vars = inner_bits.bit_length() - 1 - level
            if inner_n_vars < 0:
                continue
            for out_elems in (1, 32, 2 * UNIT_ELEMS):
                n_vars = out_elems.bit_length() - 1 + 7 - level
                if n_vars >= inner_n_vars:
                    specs.append(repeat_spec(level, n_vars, inner_n_vars, 2))
    return specs


def test_repeating(hal):
    specs = repeat_specs()
    assert {s["inner_n_vars"] + s["level"] for s in specs} >= {1, 3, 7, 12}
    run_batch(hal, specs)


# ---- zero padded
def pad_specs():
    """start_index in {0, middle, inner_n_vars}, nonzero_index first, middle and last; runs of one bit up to whole elements, periods below
    and above 128 bits, an inner below one element, an output of two units."""
    specs = []
    for level, inner_n_vars, pads in ((0, 10, (1, 3, 8)), (0, 4, (1, 3, 9)), (3, 7, (1, 4)), (3, 2, (2, 5)), (5, 4, (2,)), (7, 3, (1, 8))):
        for n_pad_vars in pads:
            for start_index in sorted({0, inner_n_vars // 2, inner_n_vars}):
                for nonzero_index in sorted({0, (1 << n_pad_vars) // 2, (1 << n_pad_vars) - 1}):
                    if inner_n_vars + n_pad_vars + level >= 7:
                        specs.append(pad_spec(level, inner_n_vars, n_pad_vars, start_index, nonzero_index, 3))
    return specs


def test_zero_padded(hal):
    specs = pad_specs()
    runs = {s["start_index"] + s["level"] for s in specs}
    periods = {s["start_index"] + s["level"] + s["n_vars"] - s["inner_n_vars"] for s in specs}
    assert min(runs) == 0 and max(runs) >= 7 and min(periods) < 7 <= max(periods)
    run_batch(hal, specs)


# ---- XOR combination
def xor_specs():
    from binius_amd._ffi import PEL_MAX_TERMS

    specs = []
    for level, offsets in ((0, (0, 1)), (7, (0, 0x0123456789ABCDEF_FEDCBA9876543210))):
        for n_vars in (7 - level, 18 - level):
            for offset in offsets:
                specs.append(xor_spec(level, n_vars, [], offset))
                specs.append(xor_spec(level, n_vars, [10], offset))
                specs.append(xor_spec(level, n_vars, [10, 11, 12, 13, 14], offset))
                specs.append(xor_spec(level, n_vars, [10, 11, 10], offset))  # a column twice: it cancels
            specs.append(xor_spec(level, n_vars, [10 + (i * i) % 7 for i in range(PEL_MAX_TERMS)], offsets[1]))
    specs.append(xor_spec(3, 9, [10, 11], 0xA7))
    specs.append(xor_spec(5, 12, [10, 11, 12], 0xDEADBEEF))
    return specs


def test_xor_combination(hal):
    run_batch(hal, xor_specs())


# ---- every kind, four levels, five sizes, one call
def mixed_specs():
    return [
        shift_spec(0, 7, 2, 1, D.LOGICAL_LEFT, 4), shift_spec(0, 18, 6, 1, D.CIRCULAR_LEFT, 4), shift_spec(3, 12, 12, 77, D.LOGICAL_RIGHT, 4),
        shift_spec(5, 9, 3, 5, D.CIRCULAR_LEFT, 4), shift_spec(7, 11, 4, 9, D.LOGICAL_LEFT, 4),
        repeat_spec(0, 12, 3, 4), repeat_spec(3, 9, 9, 4), repeat_spec(7, 11, 2, 4),
        pad_spec(0, 7, 5, 3, 17, 4), pad_spec(3, 5, 4, 5, 15, 4), pad_spec(5, 4, 5, 2, 0, 4), pad_spec(7, 0, 9, 0, 300, 4),
        xor_spec(0, 18, [4, 5, 6, 7, 8], 1), xor_spec(3, 4, [4, 5], 0x80), xor_spec(5, 9, [], 7), xor_spec(7, 11, [4, 4, 5], 1 << 127),
    ]


def test_mixed_batch(hal):
    specs = mixed_specs()
    assert {s["kind"] for s in specs} == {"shifted", "repeating", "zero_padded", "xor"} and len({s["level"] for s in specs}) == 4
    assert len({elems(s["level"], s["n_vars"]) for s in specs}) >= 5
    run_batch(hal, specs)


@pytest.mark.parametrize("seed", ["zero", "ones"])
def test_extreme_data(hal, seed):
    specs = []
    for level in (0, 3, 7):
        specs += [s for s in shift_specs(level, seed) if s["n_vars"] + level == 10]
    specs += [dict(s, inputs=[k[:2] + (seed,) for k in s["inputs"]]) for s in mixed_specs()]
    run_batch(hal, specs)


def test_no_jobs_is_a_no_op(hal):
    before = hal.derive_counters()
    hal.derive_columns_batch([])
    assert hal.derive_counters() == before


# ---- validation: one valid call, then one argument wrong per case
def _structs(jobs):
    """The DeriveJob array and term pointer list Context.derive_columns_batch would build."""
    from binius_amd import _ffi as F

    kinds = {"shifted": 0, "repeating": 1, "zero_padded": 2, "xor": 3}
    variants = {"circular_left": 0, "logical_left": 1, "logical_right": 2}
    table, terms = [], []
    for jb in jobs:
        tms = jb.get("terms", [])
        table.append(F.DeriveJob(kinds[jb["kind"]], jb["level"], jb["n_vars"], jb.get("inner_n_vars", 0), jb["inner"].ptr if "inner" in jb else None, jb["out"].ptr,
                                 jb.get("block_size", 0), variants[jb.get("variant", "circular_left")], jb.get("shift_offset", 0), jb.get("start_index", 0), 0,
                                 jb.get("nonzero_index", 0), len(terms), len(tms), F.to_f128(jb.get("offset", 0))))
        terms += [t.ptr for t in tms]
    return table, terms


VALID = [shift_spec(0, 10, 6, 3, D.CIRCULAR_LEFT, 5), repeat_spec(3, 8, 2, 5), pad_spec(0, 8, 2, 3, 1, 5), xor_spec(3, 7, [5, 6], 0x11)]


def _set(index, **fields):
    def change(table, terms, jobs):
        for k, v in fields.items():
            setattr(table[index], k, v(table, jobs) if callable(v) else v)
    return change


def _terms(fn):
    def change(table, terms, jobs):
        fn(terms)
    return change


INVALID = {
    "unknown kind": _set(0, kind=4),
    "level 1": _set(0, tower_level=1),
    "level 2": _set(1, tower_level=2),
    "level 8": _set(1, tower_level=8),
    "null output": _set(0, d_out=None),
    "null inner": _set(1, d_inner=None),
    "misaligned output": _set(0, d_out=lambda t, j: j[0]["out"].ptr + 8),
    "misaligned inner": _set(2, d_inner=lambda t, j: j[2]["inner"].ptr + 4),
    "null term": _terms(lambda terms: terms.__setitem__(1, None)),
    "misaligned term": _terms(lambda terms: terms.__setitem__(0, terms[0] + 8)),
    "output overlaps its own inner": _set(0, d_out=lambda t, j: j[0]["inner"].ptr + 16),
    "output overlaps another job's inner": _set(0, d_out=lambda t, j: j[2]["inner"].ptr),
    "output overlaps another job's term": _set(1, d_out=lambda t, j: j[3]["terms"][1].ptr),
    "output overlaps another output": _set(1, d_out=lambda t, j: j[0]["out"].ptr + 16 * 7),
    "output below one element": _set(3, n_vars=3),
    "n_vars above the limit": _set(1, n_vars=41),
    "reserved set": _set(2, reserved=1),
    "block_size above n_vars": _set(0, block_size=11),
    "shift_offset zero": _set(0, shift_offset=0),
    "shift_offset a whole block": _set(0, shift_offset=64),
    "unknown shift variant": _set(0, shift_variant=3),
    "repeating: inner above the output": _set(1, inner_n_vars=9),
    "zero padded: inner above the output": _set(2, inner_n_vars=11),
    "start_index above inner_n_vars": _set(2, start_index=9),
    "nonzero_index = 2^n_pad_vars": _set(2, nonzero_index=4),
    "too many terms": _set(3, n_terms=65),
    "terms leave the list": _set(3, first_term=1),
    "offset outside the level": _set(3, offset=lambda t, j: __import__("binius_amd")._ffi.to_f128(0x100)),
}


@pytest.fixture(scope="module")
def valid_call(hal):
    jobs, outs, want = run_batch(hal, VALID)
    return jobs, outs, want


@pytest.mark.parametrize("case", sorted(INVALID))
def test_validation(hal, valid_call, case):
    from binius_amd import _ffi as F

    jobs, outs, want = valid_call
    table, terms = _structs(jobs)
    INVALID[case](table, terms, jobs)
    before = hal.derive_counters()
    with pytest.raises(F.BnError) as e:
        hal.derive_columns_raw((F.DeriveJob * len(table))(*table), len(table), (C.c_void_p * len(terms))(*terms), len(terms))
    assert e.value.kind == "InputValidation", case
    assert hal.derive_counters() == before
    for (_, check), w in zip(outs, want):
        check(w)  # nothing was launched: the outputs still hold the valid call's values, the frames are intact


def test_null_tables_are_rejected(hal, valid_call):
    from binius_amd import _ffi as F

    jobs, outs, want = valid_call
    table, terms = _structs(jobs)
    before = hal.derive_counters()
    with pytest.raises(F.BnError) as e:
        hal.derive_columns_raw(None, len(table), (C.c_void_p * len(terms))(*terms), len(terms))
    assert e.value.kind == "InputValidation"
    with pytest.raises(F.BnError) as e:
        hal.derive_columns_raw((F.DeriveJob * len(table))(*table), len(table), None, len(terms))
    assert e.value.kind == "InputValidation"
    assert hal.derive_counters() == before
