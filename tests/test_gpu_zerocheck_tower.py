"""GPU parity of the batched univariate-skip zerocheck prover for tables over B16 .. B128 (bnh_zerocheck_batch_prove_tower:
binius_amd/host/zerocheck.hpp over bn_zerocheck_univariate_evals_base, bn_univariate_fold_batch + bn_fold_right, the eq-ind sumcheck
prover and bn_partial_eval_high_batch) against the CPU restatement tests/univariate_skip_base_ref.py (pinned by
tests/test_univariate_skip_base_oracle.py): EVERY output, bit for bit, twice from resident inputs.  The witnesses satisfy their
constraints, so the device's transcript also passes the restatement's verifier and the evaluations equal the columns' own.  A batch
needs a table of at least k variables: the B32 table of one variable at k = 3 comes with a B8 table of four."""
import functools

import pytest

import univariate_skip_base_ref as B
import zerocheck_skip_ref as Z
from test_gpu_hal import upload
from test_univariate_skip_base_oracle import product_table, samples
from test_zerocheck_skip_oracle import b1_table, b8_table, shapes

pytestmark = pytest.mark.gpu

CASES = {
    "b32_mul_9_7": (7, lambda o: [product_table(o, 51, 9, 5)]),
    "b128_mul_8_7": (7, lambda o: [product_table(o, 52, 8, 7)]),
    "cubic_b16_8_6": (6, lambda o: [product_table(o, 53, 8, 4, cubic=True)]),
    "batch_b32_2_b1_5_b8_9_b64_12_at_7": (7, lambda o: [product_table(o, 55, 2, 5), b1_table(5, 54), b8_table(9, 56), product_table(o, 57, 12, 6)]),
    "b32_of_one_variable_at_3": (3, lambda o: [product_table(o, 58, 1, 5), b8_table(4, 59)]),
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

    k, make = CASES[name]
    tables = make(oracle)
    args = samples(oracle, 0x300 + sorted(CASES).index(name), tables, k)
    return tables, k, args, B.prove(tables, k, *args)


def device_tables(hal, alloc, tables):
    return [(t["n_vars"], [(upload(hal, alloc, B.pack(v, level)), level) for v, level in t["cols"]], t["comps"]) for t in tables]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_equals_the_restatement(hal, name):
    from binius_amd._host import ZerocheckBatchPlan

    tables, k, args, want = expected(name)
    alloc = hal.dev_alloc()
    d_tables = device_tables(hal, alloc, tables)
    scratch = alloc.alloc(ZerocheckBatchPlan.scratch_elems(d_tables, k, tower=True))
    narrow = sum(1 for t in tables for _, level in t["cols"] if level <= 3)
    # a wide column of at least one 16-byte element (after the padding to k variables) takes one bn_fold_right
    wide = sum(1 for t in tables for _, level in t["cols"] if level > 3 and max(t["n_vars"], k) + level >= 7)
    folds = hal.univariate_fold_counters()
    for _ in range(2):  # resident inputs, run twice: the same values
        plan = ZerocheckBatchPlan(hal, d_tables, k, *args, scratch, tower=True)
        got = plan.run()
        for key in ("message", "round_coeffs", "final_evals", "reduction_round_coeffs", "reduction_final_evals", "skipped_challenges", "unskipped_challenges",
                    "concat_multilinear_evals"):
            assert got[key] == want[key], "%s differs (%s)" % (key, name)
        assert plan.phases()["fold"][1] == wide + (1 if narrow else 0)
    now = hal.univariate_fold_counters()
    # ONE batched fold per proof for the narrow columns of all tables, none for a batch without them
    assert now["calls"] - folds["calls"] == (2 if narrow else 0) and now["launches"] - folds["launches"] == (2 if narrow else 0)
    assert now["columns"] - folds["columns"] == 2 * narrow
    skipped, unskipped, evals = Z.verify(shapes(tables), k, *args, got)
    assert evals == B.column_evals(tables, k, skipped, unskipped)


def test_old_entry_points_still_reject_level_4(oracle, hal):
    import binius_amd
    from binius_amd._host import ZerocheckBatchPlan

    tables = [product_table(oracle, 60, 8, 4)]
    k = 7
    args = samples(oracle, 0x3F0, tables, k)
    alloc = hal.dev_alloc()
    d = device_tables(hal, alloc, tables)
    scratch = alloc.alloc(ZerocheckBatchPlan.scratch_elems(d, k, tower=True))
    ZerocheckBatchPlan(hal, d, k, *args, scratch, tower=True).run()  # the valid call first
    with pytest.raises(binius_amd.BnError) as e:
        ZerocheckBatchPlan(hal, d, k, *args, scratch).run()
    assert e.value.kind == "InputValidation"
    out = alloc.alloc(2)
    with pytest.raises(binius_amd.BnError) as e:
        hal.univariate_fold_batch([(d[0][1][0][0], 4, 8)], k, oracle.random_scalars(0x3F1, 1 << k), [out])
    assert e.value.kind == "InputValidation"
