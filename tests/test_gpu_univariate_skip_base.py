"""GPU parity of the univariate round for the wide arms of constraint_system/prove.rs:483-490 (bn_zerocheck_univariate_evals_base:
binius_amd/csrc/kernels_univariate_base.hip + abi_univariate.cpp) against the CPU restatement tests/univariate_skip_base_ref.py
(pinned by tests/test_univariate_skip_base_oracle.py).  Every output is bit-equal, every case runs twice from resident inputs.

Shapes: base_level 4 .. 7; k in {1, 2, 6, 7} (at k <= 2 a block of level 4 / 5 values is smaller than a 16-byte element, at k = 7 a
B32 block is 32 elements); n - k in {0, 1}; columns of every level <= base in one call (a B1 and a B8 column among them);
compositions of degree 1, a product with a constant outside B8, a POW step, a cubic (k <= 6), per-composition and batched output,
max_domain_size equal to and above d 2^k.  The kernel gives one wave to every (tile of x, composition, 64 points) and caps the
workgroups of a launch at 2048: with five compositions of at most 64 points that is 409 tiles, so n - k = 10 (1024 values of x) is
342 tiles of three x whose last tile holds one -- the size at which a workgroup takes several x with a ragged last tile."""
import ctypes as C

import numpy as np
import pytest

import adversarial as A
import univariate_skip_base_ref as B
import univariate_skip_ref as R
from test_gpu_hal import upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, 1 << 22)
    yield ctx
    ctx.close()


def column_levels(base):
    """Two columns at the base level, a B1 and a B8 column, one column at every level between."""
    return [base, base, 0, 3] + list(range(4, base))


def random_column(rng, level, n_vars):
    if level in (0, 3):
        return rng.integers(0, 2 if level == 0 else 256, 1 << n_vars, dtype=np.uint8)
    return rng.integers(0, 256, (1 << n_vars, 1 << (level - 3)), dtype=np.uint8)


def comp_set(base, k):
    """(compositions, degrees) over the columns of column_levels(base); the constant lies outside B8 and inside the base field."""
    cst = (1 << (1 << base)) - 3
    comps = [
        ([("var", 0), ("var", 2), ("add", 0, 1), ("const", 0x1FF), ("add", 2, 3)], 1),                              # degree 1: contributes nothing
        ([("var", 0), ("var", 1), ("mul", 0, 1), ("var", 3), ("add", 2, 3), ("const", cst), ("add", 4, 5)], 2),    # a product, a wide constant
        ([("var", 1), ("const", cst), ("mul", 0, 1), ("var", 2), ("mul", 2, 3), ("var", 3), ("add", 4, 5)], 2),    # constant * wide * B1 + B8
    ]
    if base > 4:
        comps.append(([("var", 4), ("var", 0), ("mul", 0, 1), ("var", len(column_levels(base)) - 1), ("add", 2, 3)], 2))  # a narrower wide column
    if 3 << k <= 256:
        comps.append(([("var", 1), ("pow", 0, 3), ("var", 2), ("add", 1, 2)], 3))                                   # one POW step
        comps.append(([("var", 0), ("var", 1), ("mul", 0, 1), ("var", 3), ("mul", 2, 3), ("var", 0), ("add", 4, 5)], 3))  # a cubic
    return [c for c, _ in comps], [d for _, d in comps]


def run_case(oracle, hal, base, n_vars, k, cols, comps, degrees, D, seed, place=None):
    ch = oracle.random_scalars(0x7D00 + seed, n_vars - k)
    alpha = oracle.random_scalars(0x7D80 + seed, 1)[0]
    want = B.univariate_evals(base, cols, n_vars, k, comps, degrees, ch, D)
    want_b = B.univariate_evals(base, cols, n_vars, k, comps, degrees, ch, D, alpha)
    alloc = hal.dev_alloc()
    checks = []
    if place is None:
        d_cols = [(upload(hal, alloc, B.pack(v, level)), level) for v, level in cols]
    else:
        d_cols = []
        for (v, level), lead in zip(cols, place):
            s, check = A.place(hal, alloc, B.pack(v, level), lead)
            d_cols.append((s, level))
            checks.append(check)
    d_eq = upload(hal, alloc, oracle.ints_to_arr(R.eq_expansion(ch)))
    for _ in range(2):  # resident inputs, run twice: the same values
        got = hal.zerocheck_univariate_evals_base(base, n_vars, k, d_cols, comps, degrees, d_eq, D)
        got_b = hal.zerocheck_univariate_evals_base(base, n_vars, k, d_cols, comps, degrees, d_eq, D, alpha)
        assert got == want, "per-composition output differs (base=%d n=%d k=%d D=%d)" % (base, n_vars, k, D)
        assert got_b == want_b, "batched output differs (base=%d n=%d k=%d D=%d)" % (base, n_vars, k, D)
    for check in checks:
        check()
    return want


@pytest.mark.parametrize("k", [1, 2, 6, 7])
@pytest.mark.parametrize("base", [4, 5, 6, 7])
def test_wide_arms_vs_restatement(oracle, hal, base, k):
    rng = np.random.default_rng(100 * base + k)
    comps, degrees = comp_set(base, k)
    levels = column_levels(base)
    d_top = max(degrees) << k
    for n_vars in (k, k + 1):
        cols = [(random_column(rng, level, n_vars), level) for level in levels]
        want = run_case(oracle, hal, base, n_vars, k, cols, comps, degrees, d_top, 16 * n_vars + base)
        assert all(v == 0 for v in want[0])  # degree 1: the zero polynomial
    if d_top < 256:  # a max domain above d 2^k: the extrapolation
        D = min(256, d_top + (1 << k) + 3)
        run_case(oracle, hal, base, k + 1, k, cols, comps, degrees, D, 99 + base)


def test_several_x_per_workgroup_with_a_ragged_last_tile(oracle, hal):
    """1024 values of x, five compositions of at most 8 points: 342 tiles of three x, one x in the last (see the module's text)."""
    base, k, n_vars = 5, 2, 12
    rng = np.random.default_rng(0x5A)
    comps, degrees = comp_set(base, k)
    comps, degrees = comps[:5], degrees[:5]
    assert len(comps) == 5 and 2048 // 5 == 409 and -(-1024 // 409) == 3 and 1024 - 341 * 3 == 1
    cols = [(random_column(rng, level, n_vars), level) for level in column_levels(base)]
    run_case(oracle, hal, base, n_vars, k, cols, comps, degrees, max(degrees) << k, 0x5A)


def test_sixty_four_steps_over_b128(oracle, hal):
    """The longest composition the op takes, over the widest field: the step values of a workgroup fill 64 KiB of LDS."""
    base, k, n_vars = 7, 1, 2
    rng = np.random.default_rng(0x64)
    steps = [("var", 0), ("var", 1), ("mul", 0, 1)]
    while len(steps) < 63:
        steps += [("const", int.from_bytes(rng.bytes(16), "little")), ("add", len(steps) - 1, len(steps))]
    steps.append(("add", 62, 0))
    assert len(steps) == 64
    cols = [(random_column(rng, 7, n_vars), 7), (random_column(rng, 7, n_vars), 7)]
    run_case(oracle, hal, base, n_vars, k, cols, [steps], [2], 4, 0x64)


@pytest.mark.parametrize("base,k", [(5, 7), (7, 2)])
def test_adversarial_columns_at_odd_bases_between_canaries(oracle, hal, base, k):
    """All-ones and all-zero columns beside random ones, every column at an odd multiple of 16 bytes inside a canary frame."""
    n_vars = k + 1
    rng = np.random.default_rng(0xAD + base)
    w = 1 << (base - 3)
    ones = np.full((1 << n_vars, w), 0xFF, dtype=np.uint8)
    zeros = np.zeros((1 << n_vars, w), dtype=np.uint8)
    cols = [(ones, base), (random_column(rng, base, n_vars), base), (np.ones(1 << n_vars, dtype=np.uint8), 0), (np.full(1 << n_vars, 0xFF, dtype=np.uint8), 3),
            (zeros, base)]
    comps = [
        [("var", 0), ("var", 1), ("mul", 0, 1), ("var", 3), ("add", 2, 3)],
        [("var", 0), ("var", 0), ("mul", 0, 1), ("var", 2), ("mul", 2, 3)],
        [("var", 4), ("var", 1), ("mul", 0, 1), ("var", 0), ("add", 2, 3)],
    ]
    run_case(oracle, hal, base, n_vars, k, cols, comps, [2, 2, 2], 2 << k, 0xAD, place=[1, 3, 5, 7, 9])


def test_base_3_forwards_and_b8_tables_agree_across_bases(oracle, hal):
    """base_level = 3 is bn_zerocheck_univariate_evals; a B8 table at base 5 gives what it gives at base 3."""
    n_vars, k = 8, 6
    rng = np.random.default_rng(0xF3)
    vals = [rng.integers(0, 2, 1 << n_vars, dtype=np.uint8), rng.integers(0, 256, 1 << n_vars, dtype=np.uint8), rng.integers(0, 256, 1 << n_vars, dtype=np.uint8)]
    levels = [0, 3, 3]
    comps = [[("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("mul", 2, 3), ("const", 0x53), ("add", 4, 5)], [("var", 1), ("pow", 0, 2), ("var", 2), ("add", 1, 2)]]
    degrees, D = [3, 2], 3 << k
    ch = oracle.random_scalars(0x7E00, n_vars - k)
    alloc = hal.dev_alloc()
    d_cols = [(upload(hal, alloc, R.pack(v, level)), level) for v, level in zip(vals, levels)]
    d_eq = upload(hal, alloc, oracle.ints_to_arr(R.eq_expansion(ch)))
    old = hal.zerocheck_univariate_evals(n_vars, k, d_cols, comps, degrees, d_eq, D)
    assert old == R.univariate_evals(list(zip(vals, levels)), n_vars, k, comps, degrees, ch, D)
    assert hal.zerocheck_univariate_evals_base(3, n_vars, k, d_cols, comps, degrees, d_eq, D) == old
    assert hal.zerocheck_univariate_evals_base(5, n_vars, k, d_cols, comps, degrees, d_eq, D) == old


def raw_call(hal, base, n_vars, k, columns, comps, degrees, eq, D, out):
    """bn_zerocheck_univariate_evals_base with a caller-held output array; returns the status."""
    from binius_amd import _ffi as F

    mls = (F.HalMultilinear * max(1, len(columns)))()
    for i, (sl, level) in enumerate(columns):
        mls[i].kind, mls[i].tower_level, mls[i].d_evals, mls[i].len, mls[i].n_vars_ml = F.HAL_ML_TRANSPARENT, level, sl.ptr, sl.len, n_vars
    flat, offs = [], [0]
    for steps in comps:
        flat += list(steps)
        offs.append(len(flat))
    return F.lib().bn_zerocheck_univariate_evals_base(hal._h, base, n_vars, k, mls, len(columns), F.make_steps(flat), (C.c_uint32 * len(offs))(*offs),
                                                      (C.c_uint32 * len(degrees))(*degrees), len(comps), eq.ptr, eq.len, D, None, out)


def test_validation_errors(oracle, hal):
    from binius_amd import _ffi as F

    alloc = hal.dev_alloc()
    base, n_vars, k = 5, 8, 3
    rng = np.random.default_rng(0xE0)
    col = upload(hal, alloc, B.pack(random_column(rng, 5, n_vars), 5))
    assert col.len == (1 << n_vars) >> 2
    eq = upload(hal, alloc, oracle.ints_to_arr(R.eq_expansion(oracle.random_scalars(5, n_vars - k))))
    quad = [("var", 0), ("var", 0), ("mul", 0, 1), ("const", 0xFFFFFFFE), ("add", 2, 3)]
    n_out = 8
    out = (F.F128 * n_out)()
    # the valid call first: the cases below differ from it in one argument each
    assert raw_call(hal, base, n_vars, k, [(col, 5)], [quad], [2], eq, 16, out) == 0
    assert any(F.from_f128(out[i]) for i in range(n_out))
    cases = [
        (2, n_vars, k, [(col, 5)], [quad], [2], eq, 16),                                       # base 2
        (8, n_vars, k, [(col, 5)], [quad], [2], eq, 16),                                       # base 8
        (4, n_vars, k, [(col, 5)], [[("var", 0), ("var", 0), ("mul", 0, 1)]], [2], eq, 16),    # a column above the base
        (base, n_vars, k, [(col, 1)], [quad], [2], eq, 16),                                    # a level-1 column
        (base, n_vars, k, [(col, 5)], [quad[:3] + [("const", 1 << 32), ("add", 2, 3)]], [2], eq, 16),  # a constant outside the base field
        (base, n_vars, k, [(col.slice(0, col.len // 2), 5)], [quad], [2], eq, 16),             # a wrong packed length
    ]
    sentinel = 0xA5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5
    for args in cases:
        for i in range(n_out):
            out[i] = F.to_f128(sentinel)
        hal.prof_begin()
        rc = raw_call(hal, *args, out)
        prof = hal.prof_end()
        assert rc == F.BN_ERR_INPUT_VALIDATION, args
        assert all(F.from_f128(out[i]) == sentinel for i in range(n_out)), "a rejected call wrote its output"
        assert prof["round_eval"][1] == 0, "a rejected call launched the round evaluation"
    # (the counter does move for the valid call)
    hal.prof_begin()
    assert raw_call(hal, base, n_vars, k, [(col, 5)], [quad], [2], eq, 16, out) == 0
    assert hal.prof_end()["round_eval"][1] >= 1


def test_old_entry_point_still_rejects_a_wide_column_and_constant(oracle, hal):
    import binius_amd

    alloc = hal.dev_alloc()
    n_vars, k = 8, 3
    wide = upload(hal, alloc, oracle.random_b128(6, (1 << n_vars) >> 3))  # a level-4 column
    b8 = upload(hal, alloc, oracle.random_b128(7, (1 << n_vars) >> 4))
    eq = upload(hal, alloc, oracle.ints_to_arr(R.eq_expansion(oracle.random_scalars(5, n_vars - k))))
    quad = [("var", 0), ("var", 0), ("mul", 0, 1)]
    for cols, comp in (([(wide, 4)], quad), ([(b8, 3)], quad + [("const", 0x100), ("add", 2, 3)])):
        with pytest.raises(binius_amd.BnError) as e:
            hal.zerocheck_univariate_evals(n_vars, k, cols, [comp], [2], eq, 16)
        assert e.value.kind == "InputValidation"
