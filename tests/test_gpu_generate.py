"""bn_generate_columns_batch (csrc/kernels_generate.hip, abi_generate.cpp) against tests/generate_ref.py, bit for bit -- never against the
device's own output.  Every inner column and output sits at an odd 16-byte base between canary frames (tests/adversarial.py); inputs
must be unchanged after the call; every batch runs twice from resident inputs.  Shapes are the smallest at which a path can go wrong.
A column has a power-of-two number of 16-byte elements, so the sizes beside "one element" and "one chunk" (1024) are the first with a
second chunk (2048) and the first with a second unit (8192): no column has 1025 or 4097 elements."""
import json
import os

import numpy as np
import pytest

import adversarial as A
import generate_ref as G

pytestmark = pytest.mark.gpu

ARENA = 6 << 20  # elements
UNIT_ELEMS = 4096  # outputs of one workgroup, taken 1024 at a time
CHUNK_ELEMS = 1024
SIZES = (1, CHUNK_ELEMS, 2 * CHUNK_ELEMS, 2 * UNIT_ELEMS)  # one element, one chunk, a second chunk, a second unit
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATORS = {int(k).bit_length() - 1: int(v, 16) for k, v in json.load(open(os.path.join(ROOT, "tests", "golden", "field_kats.json")))["multiplicative_generators"].items()}


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    with binius_amd.Context(0, ARENA) as h:
        yield h


# ---- inputs: (level, n_vars, seed) -> values, computed once and never modified; seed "ones": extreme data
_VALUES, _EXPECTED = {}, {}


def values(key):
    if key not in _VALUES:
        level, n_vars, seed = key
        if seed == "ones":
            v = G.constant((1 << (1 << level)) - 1, level, n_vars)
        else:
            v = G.random_values(np.random.default_rng([0x6E, level, n_vars, seed]), level, n_vars)
        v.setflags(write=False)
        _VALUES[key] = v
    return _VALUES[key]


def elems(level, n_vars):
    return max(1, (1 << (n_vars + level)) >> 7)


def n_vars_for(level, out_elems):
    return out_elems.bit_length() - 1 + 7 - level


# ---- specs: what a job is, independent of where its columns live
def proj_spec(level, n_vars, start_index, query_size, query_bits, seed=0):
    return {"kind": "projected_bits", "level": level, "n_vars": n_vars, "start_index": start_index, "query_size": query_size, "query_bits": query_bits,
            "inputs": [(level, n_vars + query_size, seed)]}


def const_spec(level, n_vars, value):
    return {"kind": "constant", "level": level, "n_vars": n_vars, "value": value, "inputs": []}


def index_spec(kind, n_vars, index):
    return {"kind": kind, "level": 0, "n_vars": n_vars, "index": index, "inputs": []}


def incr_spec(level, n_vars):
    return {"kind": "incrementing", "level": level, "n_vars": n_vars, "inputs": []}


def powers_spec(level, n_vars, base):
    return {"kind": "powers", "level": level, "n_vars": n_vars, "value": base, "inputs": []}


def expected(spec):
    """The packed column the restatement gives (computed once per spec: the powers are a Python loop over the oracle's product)."""
    key = json.dumps(spec, sort_keys=True)
    if key not in _EXPECTED:
        k, level, n = spec["kind"], spec["level"], spec["n_vars"]
        if k == "projected_bits":
            v = G.projected_bits(values(tuple(spec["inputs"][0])), spec["start_index"], spec["query_size"], spec["query_bits"])
        elif k == "constant":
            v = G.constant(spec["value"], level, n)
        elif k in ("step_down", "step_up", "select_row"):
            v = getattr(G, k)(n, spec["index"])
        elif k == "incrementing":
            v = G.incrementing(level, n)
        else:
            v = G.powers(spec["value"], level, n)
        _EXPECTED[key] = G.pack(v, level)
    return _EXPECTED[key]


def job_of(spec, out, inputs):
    """The dict Context.generate_columns_batch takes, from a spec, its output slice and its input slices."""
    jb = {k: v for k, v in spec.items() if k != "inputs"}
    jb["out"] = out
    if inputs:
        jb["inner"] = inputs[0]
    return jb


def run_batch(hal, specs):
    """Place, generate, compare every output with the restatement and every input with what was uploaded, frames included; twice."""
    alloc = hal.dev_alloc()
    placed, lead = {}, 1
    for spec in specs:
        for key in spec["inputs"]:
            if key not in placed:
                placed[key] = A.place(hal, alloc, G.pack(values(key), key[0]), lead)
                lead = (lead + 2) % 16
    outs = []
    for spec in specs:
        outs.append(A.place(hal, alloc, elems(spec["level"], spec["n_vars"]), lead))
        lead = (lead + 2) % 16
    jobs = [job_of(spec, out[0], [placed[k][0] for k in spec["inputs"]]) for spec, out in zip(specs, outs)]
    want = [expected(spec) for spec in specs]
    for _ in range(2):
        before = hal.generate_counters()
        hal.generate_columns_batch(jobs)
        after = hal.generate_counters()
        assert {k: after[k] - before[k] for k in after} == {"calls": 1, "launches": 1, "jobs": len(specs)}
        for i, (spec, (_, check)) in enumerate(zip(specs, outs)):
            try:
                check(want[i])
            except AssertionError as e:
                raise AssertionError("job %d %r: %s" % (i, spec, e)) from None
        for _, check in placed.values():
            check()
    return jobs, outs, want


# ---- projection.  w = start_index + level: log2 of a contiguous run in bits; W = w + query_size: log2 of the stride
PROJ_GRID = {  # level -> (start indices, query sizes): (w, W) on every side of 5 / 6 / 7 bits
    0: ((0, 3, 5, 6, 7, 9), (1, 2, 5, 8)),
    3: ((0, 2, 3, 4, 6), (1, 2, 5)),
    5: ((0, 1, 2, 4), (1, 2, 5)),
    7: ((0, 2), (1, 3)),
}


def proj_grid_specs(level, seed):
    specs = []
    starts, sizes = PROJ_GRID[level]
    for s in starts:
        for m in sizes:
            n_vars = max(7 - level, s)  # the smallest output that holds a run: one element, or one run
            for bits in sorted({0, (1 << m) - 1, (1 << m) // 2 - (1 if m > 1 else 0)}):
                specs.append(proj_spec(level, n_vars, s, m, bits, seed))
    return specs


@pytest.mark.parametrize("seed", [0, "ones"])
@pytest.mark.parametrize("level", sorted(PROJ_GRID))
def test_projection_grid(hal, level, seed):
    specs = proj_grid_specs(level, seed)
    regimes = {(s["start_index"] + level >= 7, s["start_index"] + level + s["query_size"] >= 7) for s in specs}
    assert regimes == ({(False, False), (False, True), (True, True)} if level < 7 else {(True, True)})
    run_batch(hal, specs)


@pytest.mark.parametrize("out_elems", SIZES)
def test_projection_sizes(hal, out_elems):
    """Every regime at the sizes on both sides of a chunk and of a unit: whole elements (w >= 7), one run per input element (w < 7 <= W),
    several runs per input element (W < 7: bit j of every 32-bit word of a B1 column is (0, 5, j))."""
    specs = []
    for level, s, m, bits in ((0, 9, 1, 1), (0, 3, 5, 19), (0, 0, 5, 7), (0, 2, 2, 1), (3, 1, 3, 5), (5, 0, 1, 1), (7, 1, 2, 2), (7, 0, 1, 0)):
        n_vars = n_vars_for(level, out_elems)
        if s <= n_vars:
            specs.append(proj_spec(level, n_vars, s, m, bits, 1))
    assert len(specs) >= 6
    run_batch(hal, specs)


# ---- steps and select-row
def index_specs():
    specs = []
    small, big = 8, n_vars_for(0, 2 * UNIT_ELEMS)  # two elements; two units
    chunk_bit, unit_bit = 128 * CHUNK_ELEMS, 128 * UNIT_ELEMS
    for n_vars, indices in ((small, (0, 1, 63, 64, 127, 128, 129, 255, 256)),
                            (big, (0, 64, 129, chunk_bit - 1, chunk_bit, chunk_bit + 1, unit_bit - 1, unit_bit, unit_bit + 1, (1 << big) - 1, 1 << big))):
        for index in indices:
            specs += [index_spec("step_down", n_vars, index), index_spec("step_up", n_vars, index)]
            if index < 1 << n_vars:
                specs.append(index_spec("select_row", n_vars, index))
    return specs


def test_steps_and_select_row(hal):
    specs = index_specs()
    assert {s["kind"] for s in specs} == {"step_down", "step_up", "select_row"}
    run_batch(hal, specs)


# ---- constant
def test_constant(hal):
    specs = []
    for level in G.LEVELS:
        for out_elems in (1, 2 * CHUNK_ELEMS):
            for value in (0, 1, (1 << (1 << level)) - 1):
                specs.append(const_spec(level, n_vars_for(level, out_elems), value))
    specs.append(const_spec(5, 9, 0xDEADBEEF))
    specs.append(const_spec(7, 4, 0x0123456789ABCDEF_FEDCBA9876543210))
    run_batch(hal, specs)


# ---- incrementing
@pytest.mark.parametrize("level", [3, 4, 5, 6, 7])
def test_incrementing(hal, level):
    specs = [incr_spec(level, min(1 << level, 20)), incr_spec(level, 7 - level)]
    if level == 3:
        assert specs[0]["n_vars"] == 8
    if level > 3:
        specs.append(incr_spec(level, n_vars_for(level, 2 * CHUNK_ELEMS)))
    run_batch(hal, specs)


# ---- powers
def power_bases(level):
    rnd = int(np.random.default_rng([0x90, level]).integers(2, 1 << 62)) & ((1 << (1 << level)) - 1) if level < 7 else \
        int.from_bytes(np.random.default_rng([0x90, 7]).bytes(16), "little")
    return (0, 1, GENERATORS[level], max(2, rnd))


@pytest.mark.parametrize("level", [3, 4, 5, 6, 7])
def test_powers(hal, level):
    specs = []
    for out_elems in (1, 2 * UNIT_ELEMS):
        specs += [powers_spec(level, n_vars_for(level, out_elems), base) for base in power_bases(level)]
    run_batch(hal, specs)


# ---- every kind, four levels, one call, jobs in scrambled order
def mixed_specs():
    specs = [
        proj_spec(0, 12, 0, 5, 9, 2), proj_spec(0, 18, 3, 5, 31, 2), proj_spec(3, 9, 6, 1, 1, 2), proj_spec(5, 13, 0, 2, 2, 2), proj_spec(7, 3, 1, 2, 3, 2),
        const_spec(0, 9, 1), const_spec(3, 15, 0x5A), const_spec(7, 0, 1 << 127),
        index_spec("step_down", 18, 100001), index_spec("step_up", 7, 77), index_spec("select_row", 13, 8191),
        incr_spec(3, 8), incr_spec(5, 14), incr_spec(7, 11),
        powers_spec(3, 8, GENERATORS[3]), powers_spec(5, 10, GENERATORS[5]), powers_spec(7, 6, GENERATORS[7]),
    ]
    order = np.random.default_rng(0x5C).permutation(len(specs))
    return [specs[i] for i in order]


def test_mixed_batch(hal):
    specs = mixed_specs()
    assert len({s["kind"] for s in specs}) == 7 and len({s["level"] for s in specs}) == 4
    assert len({elems(s["level"], s["n_vars"]) for s in specs}) >= 5
    run_batch(hal, specs)


def test_no_jobs_is_a_no_op(hal):
    before = hal.generate_counters()
    hal.generate_columns_batch([])
    assert hal.generate_counters() == before


# ---- validation: one valid call, then one argument wrong per case
VALID = [proj_spec(0, 7, 3, 5, 7, 5), const_spec(3, 4, 0xA5), index_spec("step_down", 8, 100), index_spec("step_up", 8, 100), index_spec("select_row", 8, 100),
         incr_spec(5, 4), powers_spec(4, 3, 0xE2DE)]


def _structs(jobs):
    from binius_amd import _ffi as F

    return list(F.Context.generate_job_table(jobs)[0])[: len(jobs)]


def _set(job, **fields):
    def change(table, jobs):
        for k, v in fields.items():
            setattr(table[job], k, v(table, jobs) if callable(v) else v)
    return change


def _f128(value):
    return lambda t, j: __import__("binius_amd")._ffi.to_f128(value)


INVALID = {
    "unknown kind": _set(0, kind=7),
    "level 1": _set(1, tower_level=1),
    "level 2": _set(1, tower_level=2),
    "level 8": _set(1, tower_level=8),
    "step down: index above 2^n_vars": _set(2, index=257),
    "step up: index above 2^n_vars": _set(3, index=257),
    "select row: index = 2^n_vars (the strict bound)": _set(4, index=256),
    "step down at level 3": _set(2, tower_level=3),
    "select row at level 3": _set(4, tower_level=3),
    "query_bits = 2^query_size": _set(0, query_bits=32),
    "query_size zero": _set(0, query_size=0),
    "start_index + query_size above inner_n_vars": _set(0, start_index=8),
    "constant: value above the level": _set(1, value=_f128(0x100)),
    "powers: base above the level": _set(6, value=_f128(0x10000)),
    "powers at level 0": _set(6, tower_level=0, n_vars=7),
    "incrementing: n_vars above 2^level": _set(5, tower_level=3, n_vars=9),
    "incrementing at level 0 is below one element": _set(5, tower_level=0, n_vars=1),
    "null output": _set(1, d_out=None),
    "null inner": _set(0, d_inner=None),
    "misaligned output": _set(1, d_out=lambda t, j: j[1]["out"].ptr + 8),
    "misaligned inner": _set(0, d_inner=lambda t, j: j[0]["inner"].ptr + 4),
    "output overlaps its own inner": _set(0, d_out=lambda t, j: j[0]["inner"].ptr + 16),
    "output overlaps another job's inner": _set(2, d_out=lambda t, j: j[0]["inner"].ptr + 32),
    "output overlaps another output": _set(2, d_out=lambda t, j: j[3]["out"].ptr + 16),
    "output below one element": _set(2, n_vars=6),
    "n_vars above the limit": _set(1, n_vars=41),
    "reserved set": _set(3, reserved=1),
}


@pytest.fixture(scope="module")
def valid_call(hal):
    return run_batch(hal, VALID)


@pytest.mark.parametrize("case", sorted(INVALID))
def test_validation(hal, valid_call, case):
    from binius_amd import _ffi as F

    jobs, outs, want = valid_call
    table = _structs(jobs)
    INVALID[case](table, jobs)
    before = hal.generate_counters()
    with pytest.raises(F.BnError) as e:
        hal.generate_columns_raw((F.GenerateJob * len(table))(*table), len(table))
    assert e.value.kind == "InputValidation", case
    assert hal.generate_counters() == before
    for (_, check), w in zip(outs, want):
        check(w)  # nothing was launched: the outputs still hold the valid call's values, the frames are intact


def test_null_table_is_rejected(hal, valid_call):
    from binius_amd import _ffi as F

    jobs, outs, want = valid_call
    before = hal.generate_counters()
    with pytest.raises(F.BnError) as e:
        hal.generate_columns_raw(None, len(jobs))
    assert e.value.kind == "InputValidation"
    assert hal.generate_counters() == before
