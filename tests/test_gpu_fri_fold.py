"""GPU parity of bn_fri_fold on every twiddle field (B8 .. B64), every pass form of launch_fri_fold (kernels_misc.hip: k_fri_pass<3 .. 6>,
k_fri_pass_multi<2 / 3, false>, k_fri_pass_multi<2, true>) and the degenerate challenge counts (none, interleave only, a fold to one
element, log_len = 0), on the cases of tests/fri_cases.py.  The forms are reached by shape, and `Context.fri_counters()`
(bn_fri_counters) says which ones a call launched: every case asserts the hand-written list of its passes.

Every case: the output is oracle.fri_fold's, bit for bit.  Nothing is compared with the device's own output.  Input and output sit at
odd multiples of 16 bytes between canary frames (tests/adversarial.py); the input must be unchanged and every frame intact.  The table
and the oracle are pinned on the CPU by tests/test_oracle_fri_cases.py.
"""
import numpy as np
import pytest

import adversarial as A
import fri_cases as F

pytestmark = pytest.mark.gpu

# the largest case: 2^21 elements in, 2^19 out, each between two frames
ARENA = (1 << 21) + (1 << 19) + 4 * A.FRAME + 64


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, ARENA)
    yield ctx
    ctx.close()


def moved(before, after):
    assert sorted(before) == sorted(after) == sorted(F.FORMS + ("copies",))
    return {k: after[k] - before[k] for k in before}


def device_case(hal, oracle, c, chs=None):
    """One bn_fri_fold call of case `c` (with the challenges `chs`, default the case's own) against oracle.fri_fold."""
    import binius_amd

    want = F.reference(oracle, c, chs)
    chs = F.challenges(oracle, c) if chs is None else list(chs)
    s = binius_amd.ntt_s_evals(c.tw_level, c.log_domain)
    assert np.array_equal(s, F.s_evals(oracle, c))
    alloc = hal.dev_alloc()
    din, chk_in = A.place(hal, alloc, F.data(oracle, c), 1)
    dout, chk_out = A.place(hal, alloc, F.out_len(c), 9)
    chk_out()  # (the body holds the canary)
    c0 = hal.fri_counters()
    hal.fri_fold(s, c.tw_level, c.log_domain, c.log_len, c.log_batch, chs, din, dout)
    c1 = hal.fri_counters()
    chk_out(want)
    chk_in()
    assert moved(c0, c1) == F.expected_counters(c), "case %s: launched %s, expected the passes %s" % (c.id, moved(c0, c1), c.passes)
    return want


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_fri_fold_case(hal, oracle, case):
    device_case(hal, oracle, case)


@pytest.mark.parametrize("z", [0, 1, A.ALL_ONES], ids=["zero", "one", "all_ones"])
@pytest.mark.parametrize("cid", ["A", "E", "G"])
def test_constant_challenges(hal, oracle, cid, z):
    c = F.BY_ID[cid]
    device_case(hal, oracle, c, [z] * F.n_challenges(c))


def test_no_challenge_is_a_copy(hal, oracle):
    c = F.BY_ID["K"]
    assert F.n_challenges(c) == 0 and F.in_len(c) == F.out_len(c)
    want = device_case(hal, oracle, c)
    assert np.array_equal(want, F.data(oracle, c))
    assert F.expected_counters(c) == {"one": 0, "inter2": 0, "inter3": 0, "ntt2": 0, "ntt3": 0, "copies": 1}


def test_a_rejected_call_counts_nowhere(hal, oracle):
    import binius_amd

    c = F.BY_ID["L2"]
    s = binius_amd.ntt_s_evals(c.tw_level, c.log_domain)
    alloc = hal.dev_alloc()
    din, chk_in = A.place(hal, alloc, F.data(oracle, c), 1)
    dout, chk_out = A.place(hal, alloc, F.out_len(c), 9)
    c0 = hal.fri_counters()
    for tw_level, n_ch in ((2, 3), (7, 3), (5, 2)):  # no such twiddle field (twice); fewer challenges than log_batch
        with pytest.raises(binius_amd.BnError) as e:
            hal.fri_fold(s, tw_level, c.log_domain, c.log_len, c.log_batch, [1] * n_ch, din, dout)
        assert e.value.kind == "InputValidation"
    assert hal.fri_counters() == c0
    chk_in()
    chk_out()


def test_the_cached_basis_follows_the_call(hal, oracle):
    """The twiddle basis of a call is uploaded only when it differs from the last call's (upload_s_evals): calls with different bases
    in turn, on two contexts and on one, must each fold with their own."""
    import binius_amd

    c_c, c_g, c_a, c_h = (F.BY_ID[k] for k in "CGAH")
    assert not np.array_equal(F.s_evals(oracle, c_c), F.s_evals(oracle, c_g)) and not np.array_equal(F.s_evals(oracle, c_a), F.s_evals(oracle, c_h))
    small = F.in_len(c_c) + F.out_len(c_c) + 4 * A.FRAME + 64
    assert small >= F.in_len(c_g) + F.out_len(c_g) + 4 * A.FRAME + 64
    with binius_amd.Context(0, small) as h1, binius_amd.Context(0, small) as h2:
        for ctx, c in ((h1, c_c), (h2, c_g), (h1, c_g), (h2, c_c), (h1, c_c), (h2, c_g)):
            device_case(ctx, oracle, c)
    for c in (c_a, c_h, c_a):
        device_case(hal, oracle, c)
