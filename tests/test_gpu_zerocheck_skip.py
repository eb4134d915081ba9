"""GPU parity of the batched univariate-skip zerocheck prover (bnh_zerocheck_batch_prove: binius_amd/host/zerocheck.hpp over
bn_zerocheck_univariate_evals, bn_univariate_fold_batch, the eq-ind sumcheck prover and bn_partial_eval_high_batch; reference: sumcheck/
prove/batch_zerocheck.rs:166-293) against the CPU restatement tests/zerocheck_skip_ref.py (pinned by tests/test_zerocheck_skip_oracle.py):
EVERY output, bit for bit.  The definition holds without the constraints, so the keccak witnesses are random; on the satisfying
witnesses the device's transcript also passes the restatement's verifier.  Every case runs twice from resident inputs and must give the
same values; every validation case is an error."""
import functools

import numpy as np
import pytest

import zerocheck_skip_ref as R
from test_gpu_hal import upload
from test_gpu_hal_wide import keccak_constraints
from test_zerocheck_skip_oracle import b1_table, b8_table, samples, shapes, u32_add_table

pytestmark = pytest.mark.gpu

CUBIC = ([("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("mul", 2, 3), ("var", 3), ("add", 4, 5)],
         [("var", 0), ("var", 1), ("mul", 0, 1), ("var", 2), ("mul", 2, 3)], 3)  # a b c + d


def cubic_table(n_vars, seed):
    """B8 columns a, b, c, d = a b c."""
    rng = np.random.default_rng(seed)
    a, b, c = (rng.integers(0, 256, 1 << n_vars, dtype=np.uint8) for _ in range(3))
    mul = R.b8_tables()[0]
    return {"n_vars": n_vars, "cols": [(a, 3), (b, 3), (c, 3), (mul[mul[a, b], c], 3)], "comps": [CUBIC]}


def keccak_table(n_vars, seed):
    n_mls, cons = keccak_constraints(3)
    rng = np.random.default_rng(seed)
    return {"n_vars": n_vars, "cols": [(rng.integers(0, 2, 1 << n_vars, dtype=np.uint8), 0) for _ in range(n_mls)], "comps": [(s, si, 2) for s, si in cons]}


CASES = {
    "b1_9_7": (7, True, lambda: [b1_table(9, 21)]),
    "b8_9_7": (7, True, lambda: [b8_table(9, 22)]),
    "n_eq_k": (7, True, lambda: [b1_table(7, 23)]),
    "batch_5_7_9_12_at_7": (7, True, lambda: [b1_table(5, 24), b8_table(7, 25), u32_add_table(4, 26), b1_table(12, 27)]),
    "cubic_8_6": (6, True, lambda: [cubic_table(8, 28)]),
    "tiny_bit_columns_at_3": (3, True, lambda: [b1_table(2, 29), b1_table(5, 30), b8_table(6, 31)]),
    "padded_b8_tables_at_7": (7, True, lambda: [b8_table(5, 33), b8_table(6, 34), b1_table(9, 35)]),
    "keccak_13_7": (7, False, lambda: [keccak_table(13, 32)]),
}


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, 1 << 22)
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def expected(name):
    import oracle

    k, _, make = CASES[name]
    tables = make()
    args = samples(oracle, 0x100 + sorted(CASES).index(name), tables, k)
    return tables, k, args, R.prove(tables, k, *args)


def device_tables(hal, alloc, tables):
    return [(t["n_vars"], [(upload(hal, alloc, R.pack(v, level)), level) for v, level in t["cols"]], t["comps"]) for t in tables]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_equals_the_restatement(hal, name):
    from binius_amd._host import ZerocheckBatchPlan

    tables, k, args, want = expected(name)
    alloc = hal.dev_alloc()
    d_tables = device_tables(hal, alloc, tables)
    scratch = alloc.alloc(ZerocheckBatchPlan.scratch_elems(d_tables, k))
    folds = hal.univariate_fold_counters()
    for _ in range(2):  # resident inputs, run twice: the same values
        plan = ZerocheckBatchPlan(hal, d_tables, k, *args, scratch)
        got = plan.run()
        for key in ("message", "round_coeffs", "final_evals", "reduction_round_coeffs", "reduction_final_evals", "skipped_challenges", "unskipped_challenges",
                    "concat_multilinear_evals"):
            assert got[key] == want[key], "%s differs (%s)" % (key, name)
    now = hal.univariate_fold_counters()
    assert now["calls"] - folds["calls"] == 2 and now["launches"] - folds["launches"] == 2  # ONE fold launch per proof, whatever the tables
    assert now["columns"] - folds["columns"] == 2 * sum(len(t["cols"]) for t in tables)
    if CASES[name][1]:  # a satisfying witness: the device's transcript passes the restatement's verifier
        skipped, unskipped, evals = R.verify(shapes(tables), k, *args, got)
        assert evals == R.column_evals(tables, k, skipped, unskipped)


def test_validation_errors(oracle, hal):
    import binius_amd
    from binius_amd._host import ZerocheckBatchPlan

    tables = [b1_table(7, 41), b8_table(9, 42)]
    k = 7
    args = samples(oracle, 0x200, tables, k)
    alloc = hal.dev_alloc()
    d = device_tables(hal, alloc, tables)
    scratch = alloc.alloc(ZerocheckBatchPlan.scratch_elems(d, k))
    ZerocheckBatchPlan(hal, d, k, *args, scratch).run()  # the valid call first: the cases below differ from it in one argument each
    wide = (d[1][0], [(c[0], 4) for c in d[1][1]], d[1][2])
    cubic = (d[1][0], d[1][1], [(s, si, 3) for s, si, _ in d[1][2]])
    zero = (d[1][0], d[1][1], [(s, si, 0) for s, si, _ in d[1][2]])
    short = binius_amd._ffi.DevSlice(scratch.ptr, scratch.len - 1)
    cases = [
        ([d[1], d[0]], k, args, scratch),                        # claims out of order
        ([d[0]], 8, ([], args[1][:1], args[2], [], args[4], oracle.random_scalars(0x201, 8)), scratch),  # k > the largest n_vars
        ([d[0], wide], k, args, scratch),                        # a level other than 0 or 3
        ([d[0], cubic], k, args, scratch),                       # degree 3 at k = 7: d 2^k > 256
        ([d[0], zero], k, args, scratch),                        # degree 0
        (d, 0, (oracle.random_scalars(0x202, 9), args[1], args[2], oracle.random_scalars(0x203, 9), args[4], []), scratch),  # k = 0
        (d, k, args, short),                                     # a short scratch
        (d, k, (args[0][:-1],) + args[1:], scratch),             # too few zerocheck challenges
        (d, k, args[:1] + (args[1][:1],) + args[2:], scratch),   # not one coefficient per table
    ]
    folds = hal.univariate_fold_counters()
    for tabs, kk, a, scr in cases:
        with pytest.raises(binius_amd.BnError) as e:
            ZerocheckBatchPlan(hal, tabs, kk, *a, scr).run()
        assert e.value.kind == "InputValidation", (kk, len(tabs))
    assert hal.univariate_fold_counters() == folds  # nothing got as far as the fold
