"""GPU parity of the ring-switch prover (RingSwitchPlan = bnh_ring_switch_prove, binius_amd/host/ring_switch.hpp; reference:
ring_switch::prove, core/src/ring_switch/prove.rs:42-144) against the CPU restatement (tests/ring_switch_ref.py, pinned by
tests/test_ring_switch_oracle.py): the transcript -- each prefix's mixed tensor element, the row-batched evaluations -- and every
transparent, bit-exact.  The counters pin ONE bn_ring_switch_eq_ind_batch launch for all claims and one bn_partial_eval_high_batch call
per distinct suffix.  Every case runs twice from resident inputs.  One context per module."""
import numpy as np
import pytest

import adversarial as A
import ring_switch_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, 1 << 22)
    yield ctx
    ctx.close()


def run_case(oracle, hal, case):
    from binius_amd._host import RingSwitchPlan

    want = R.prove(case)
    alloc = hal.dev_alloc()
    cols, col_checks = [], []
    for t, (arr, level, n_vars) in enumerate(case["columns"]):
        s, chk = A.place(hal, alloc, arr, 2 * t + 1)
        cols.append((s, level, n_vars))
        col_checks.append(chk)
    n_scratch = RingSwitchPlan.scratch_elems(case["suffixes"], case["claims"])
    scratch, scratch_chk = A.place(hal, alloc, n_scratch, 5)
    plan = RingSwitchPlan(hal, cols, case["pool"], case["suffixes"], [k for _off, k in case["prefixes"]], case["claims"], scratch, case["mixing"], case["row"])
    distinct_suffixes = len({(case["suffixes"][c[1]][0], case["suffixes"][c[1]][1]) for c in case["claims"]})
    for _ in range(2):
        rs0, pe0 = hal.ring_switch_counters(), hal.partial_eval_counters()
        plan.run()
        rs1, pe1 = hal.ring_switch_counters(), hal.partial_eval_counters()
        assert {k: rs1[k] - rs0[k] for k in rs1} == {"calls": 1, "launches": 1, "jobs": len(case["claims"]), "queries": distinct_suffixes}
        assert pe1["calls"] - pe0["calls"] == distinct_suffixes
        assert plan.mixed_tensor_elems() == want["mixed"]
        assert plan.row_batched_evals() == want["row_batched_evals"]
        ts = plan.transparents()
        assert len(ts) == len(case["claims"])
        for i, t in enumerate(ts):
            assert scratch.ptr <= t.ptr and t.ptr + 16 * t.len <= scratch.ptr + 16 * scratch.len
            assert np.array_equal(hal.copy_d2h(t), want["transparents"][i]), "transparent of claim %d" % i
        scratch_chk(body=False)
        for chk in col_checks:
            chk()
        assert set(plan.phase_times_ms()) == set(RingSwitchPlan.PHASES)
    return plan


def test_seven_claims_four_levels(oracle, hal):
    run_case(oracle, hal, R.seven_claim_case())


def test_keccak_claim_graph_reduced(oracle, hal):
    """175 claims over 100 one-bit columns of 2^13 values, three suffixes."""
    case = R.keccak_case()
    assert len(case["claims"]) == 175 and len(case["columns"]) == 100 and len(case["suffixes"]) == 3
    run_case(oracle, hal, case)


def test_u32_add_claim_graph(oracle, hal):
    """Five claims over four columns, two suffixes, 2^10 rows of 32 bits."""
    case = R.u32_add_case()
    assert len(case["claims"]) == 5 and len(case["columns"]) == 4 and len(case["suffixes"]) == 2
    run_case(oracle, hal, case)


def test_rejections_launch_nothing(oracle, hal):
    import binius_amd
    from binius_amd._host import RingSwitchPlan

    case = R.seven_claim_case()
    alloc = hal.dev_alloc()
    cols = []
    for arr, level, n_vars in case["columns"]:
        s = alloc.alloc(arr.shape[0])
        hal.copy_h2d(arr, s)
        cols.append((s, level, n_vars))
    kappas = [k for _off, k in case["prefixes"]]
    n_scratch = RingSwitchPlan.scratch_elems(case["suffixes"], case["claims"])
    scratch = alloc.alloc(n_scratch)
    hal.fill(scratch, A.CANARY)
    rs0, pe0 = hal.ring_switch_counters(), hal.partial_eval_counters()
    bad_claims = list(case["claims"])
    ci, si, _pi = bad_claims[2]
    bad_claims[2] = (ci, si, 0)  # TowerLevelMismatch: a byte column's claim under a bit column's prefix
    small = [(cols[0][0], 0, 6)] + cols[1:]  # n_vars + level < 7
    variants = [
        (cols, case["suffixes"], kappas, bad_claims, scratch, case["mixing"], case["row"]),
        (small, case["suffixes"], kappas, case["claims"], scratch, case["mixing"], case["row"]),
        (cols, case["suffixes"], kappas, case["claims"], scratch.slice(0, n_scratch - 1), case["mixing"], case["row"]),
        (cols, case["suffixes"], kappas, case["claims"], scratch, case["mixing"][:-1], case["row"]),
        (cols, case["suffixes"], kappas, case["claims"], scratch, case["mixing"], case["row"][:-1]),
    ]
    for cs, sf, ks, cl, sc, mx, rw in variants:
        with pytest.raises(binius_amd.BnError) as e:
            RingSwitchPlan(hal, cs, case["pool"], sf, ks, cl, sc, mx, rw).run()
        assert e.value.kind == "InputValidation"
    assert hal.ring_switch_counters() == rs0 and hal.partial_eval_counters() == pe0
    assert np.array_equal(hal.copy_d2h(scratch), np.tile(oracle.ints_to_arr([A.CANARY]), (n_scratch, 1)))
