"""GPU parity of the batched fold of the univariate round of the univariate-skip zerocheck (bn_univariate_fold_batch: binius_amd/csrc/
kernels_univariate_fold.hip + abi_univariate_fold.cpp; reference: fold_univariate_round, sumcheck/prove/zerocheck.rs:384-434) against
the CPU restatement's fold (tests/zerocheck_skip_ref.py, pinned against oracle.fold_right by tests/test_zerocheck_skip_oracle.py).
Everything is bit-exact and nothing is compared with the device's own output, except where a test says that the op ALSO equals the
per-column bn_fold_right.  Outputs hold a canary before the call, so a result also pins that they are overwritten, not accumulated.
Every case runs twice from resident inputs and must give the same values.  One context per module."""
import numpy as np
import pytest

import adversarial as A
import zerocheck_skip_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, 1 << 22)
    yield ctx
    ctx.close()


def values(seed, level, n_vars):
    return np.random.default_rng(seed).integers(0, 2 if level == 0 else 256, 1 << n_vars, dtype=np.uint8)


def delta(hal, before):
    now = hal.univariate_fold_counters()
    return {k: now[k] - before[k] for k in now}


def run_batch(oracle, hal, cols, k, coeffs, also_fold_right=False):
    """cols: [(values, level, n_vars)].  One call for all columns at odd 16-byte bases between canary frames; every output against the
    restatement, frames intact, inputs unchanged.  Returns the counter deltas of the first call."""
    alloc = hal.dev_alloc()
    d_cols, d_outs, in_checks, out_checks, lead = [], [], [], [], 1
    for v, level, n_vars in cols:
        s, chk = A.place(hal, alloc, R.pack(v, level), lead)
        o, ochk = A.place(hal, alloc, 1 << (n_vars - k), lead + 8)
        lead += 2
        d_cols.append((s, level, n_vars))
        d_outs.append(o)
        in_checks.append(chk)
        out_checks.append(ochk)
    wants = [oracle.ints_to_arr(R.fold(v, k, coeffs)) for v, _, _ in cols]
    got = None
    for _ in range(2):  # resident inputs, run twice: the same values
        before = hal.univariate_fold_counters()
        hal.univariate_fold_batch(d_cols, k, coeffs, d_outs)
        got = got or delta(hal, before)
        for t, (ochk, want) in enumerate(zip(out_checks, wants)):
            try:
                ochk(want)
            except AssertionError as e:
                raise AssertionError("column %d (level %d, n_vars %d, k %d): %s" % (t, cols[t][1], cols[t][2], k, e))
        for chk in in_checks:
            chk()
    if also_fold_right:
        d_q = alloc.alloc(1 << k)
        hal.copy_h2d(oracle.ints_to_arr(list(coeffs)), d_q)
        single = alloc.alloc(max(w.shape[0] for w in wants))
        for (s, level, n_vars), want in zip(d_cols, wants):
            if n_vars + level < 7:
                continue  # (less than one element: bn_fold_right has no such shape)
            o = single.slice(0, want.shape[0])
            hal.fill(o, A.CANARY)
            hal.fold_right(s, level, d_q, o)
            assert np.array_equal(hal.copy_d2h(o), want), "fold_right differs (level %d, n_vars %d)" % (level, n_vars)
    return got


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("k", [1, 3, 6, 7, 8])
def test_one_column_vs_restatement(oracle, hal, k, level):
    """n = k: one output; k + 11: more than one workgroup's tile (2048 outputs, 512 for rows of 64 bytes and more); level 3 at k = 8:
    the tables in two passes."""
    coeffs = oracle.random_scalars(0x5F00 + 16 * k + level, 1 << k)
    for n_vars in (k, k + 1, k + 6, k + 11):
        d = run_batch(oracle, hal, [(values(1000 * k + 10 * n_vars + level, level, n_vars), level, n_vars)], k, coeffs)
        assert d == {"calls": 1, "launches": 1, "columns": 1}


@pytest.mark.parametrize("k", [7, 4])
def test_mixed_batch_is_one_launch(oracle, hal, k):
    """37 columns of both levels and five sizes (one of them below one 16-byte element at level 0, k = 4) in one call: ONE launch;
    equal to the per-column bn_fold_right as well."""
    coeffs = R.lagrange_at(1 << k, oracle.random_scalars(0x5E00 + k, 1)[0])
    cols = []
    for t in range(37):
        level = (0, 3, 0, 0, 3)[t % 5]
        n_vars = k + (0, 1, 5, 9, 12)[(t * 3) % 5]
        cols.append((values(0x5D00 + t, level, n_vars), level, n_vars))
    assert {c[1] for c in cols} == {0, 3} and len({c[2] for c in cols}) == 5
    d = run_batch(oracle, hal, cols, k, coeffs, also_fold_right=True)
    assert d == {"calls": 1, "launches": 1, "columns": 37}


@pytest.mark.parametrize("kind", ["zero", "ones", "single"])
def test_extreme_coefficients(oracle, hal, kind):
    k = 7
    coeffs = {"zero": [0] * 128, "ones": [A.ALL_ONES] * 128, "single": [0] * 77 + [oracle.random_scalars(0x5C00, 1)[0]] + [0] * 50}[kind]
    cols = [(values(0x5B00 + level, level, 13), level, 13) for level in (0, 3)]
    cols.append((np.full(1 << 12, 255, dtype=np.uint8), 3, 12))
    cols.append((np.ones(1 << 14, dtype=np.uint8), 0, 14))
    run_batch(oracle, hal, cols, k, coeffs)


def test_no_columns_is_a_no_op(hal):
    before = hal.univariate_fold_counters()
    hal.univariate_fold_batch([], 7, [0] * 128, [])
    assert delta(hal, before) == {"calls": 0, "launches": 0, "columns": 0}


def test_validation_errors(oracle, hal):
    import binius_amd
    from binius_amd._ffi import DevSlice

    alloc = hal.dev_alloc()
    n_vars, k = 12, 4
    coeffs = oracle.random_scalars(0x5A00, 1 << k)
    col = alloc.alloc(1 << (n_vars + 3 - 7))
    hal.copy_h2d(R.pack(values(0x5A01, 3, n_vars), 3), col)
    out = alloc.alloc(1 << (n_vars - k))
    hal.fill(out, A.CANARY)
    # the valid call first: the cases below differ from it in one argument each
    hal.univariate_fold_batch([(col, 3, n_vars)], k, coeffs, [out])
    want = hal.copy_d2h(out)
    assert np.array_equal(want, oracle.ints_to_arr(R.fold(values(0x5A01, 3, n_vars), k, coeffs)))
    before = hal.univariate_fold_counters()
    cases = [
        ([(col, 4, n_vars - 1)], k, coeffs, [DevSlice(out.ptr, out.len // 2)]),              # a level outside {0, 3}
        ([(col, 7, n_vars - 4)], k, coeffs, [DevSlice(out.ptr, out.len // 16)]),
        ([(col, 3, n_vars)], 0, coeffs[:1], [DevSlice(out.ptr, 1 << n_vars)]),                # k = 0
        ([(col, 3, n_vars)], 9, coeffs * 32, [DevSlice(out.ptr, 1 << (n_vars - 9))]),         # k > 8
        ([(col, 3, 3)], k, coeffs, [out]),                                                    # k > n_vars
        ([(DevSlice(col.ptr + 8, col.len - 1), 3, n_vars)], k, coeffs, [out]),                # a misaligned column
        ([(col, 3, n_vars)], k, coeffs, [DevSlice(out.ptr + 4, out.len)]),                    # a misaligned output
        ([(col, 3, n_vars)], k, coeffs, [DevSlice(col.ptr + 16 * (col.len - 1), out.len)]),   # the output overlaps its column
        ([(col, 3, n_vars)], k, coeffs, [None]),                                              # a null output
        ([(col, 3, n_vars)], k, coeffs[:-1], [out]),                                          # not 2^k coefficients
        ([(col, 3, n_vars)], k, coeffs, [DevSlice(out.ptr, out.len // 2)]),                   # an output of the wrong length
        ([(col, 3, n_vars), (col, 3, n_vars)], k, coeffs, [out]),                             # not one output per column
    ]
    for args in cases:
        with pytest.raises(binius_amd.BnError) as e:
            hal.univariate_fold_batch(*args)
        assert e.value.kind == "InputValidation", args
    assert delta(hal, before) == {"calls": 0, "launches": 0, "columns": 0}
    assert np.array_equal(hal.copy_d2h(out), want)  # nothing was launched
