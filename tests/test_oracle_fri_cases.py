"""Pins of the case table of tests/fri_cases.py, on the CPU, so that tests/test_gpu_fri_fold.py checks what it was written to check:

* on every case the oracle's two restatements of the fold agree (fri_fold: crates/compute/src/cpu/layer.rs:304-391, pass by pass;
  fold_interleaved: crates/ntt/src/fri.rs, the interleave challenges as one tensor product);
* the library's host-side twiddle basis is the oracle's for every case's field and domain;
* the cases that stand for their twiddle field read basis entries wider than the next smaller field, so that a product that dropped the
  upper half of a twiddle cannot pass them -- with the measured widths stated, and the reason why B64 needs log_len >= 17;
* the table holds every field, every pass form but the measurement one, the degenerate challenge counts, and its hand-written pass lists
  are what the schedule of launch_fri_fold (restated here from its comment) gives.
"""
import numpy as np
import pytest

import fri_cases as F


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_the_two_restatements_agree(oracle, case):
    c = case
    want = F.reference(oracle, c)
    assert want.shape == (F.out_len(c), 2)
    other = oracle.arr(F.out_len(c))
    assert oracle.fold_interleaved(F.s_evals(oracle, c), c.tw_level, c.log_domain, c.log_len, c.log_batch, F.challenges(oracle, c),
                                   F.data(oracle, c), other) == 0
    assert np.array_equal(want, other)
    if F.n_challenges(c) == 0:
        assert np.array_equal(want, F.data(oracle, c))
    else:
        assert not np.array_equal(want, F.data(oracle, c)[: F.out_len(c)])


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_library_basis_is_the_oracles(ffi, oracle, case):
    assert np.array_equal(ffi.ntt_s_evals(case.tw_level, case.log_domain), F.s_evals(oracle, case))


# the widest basis entry each of these cases reads, in bits (measured with the oracle; asserted below, not trusted)
WIDTHS = {"A": 64, "B": 64, "C": 49, "E": 8, "F": 8, "F2": 8, "G": 16, "H": 32, "M": 32}


@pytest.mark.parametrize("cid", sorted(WIDTHS))
def test_representative_cases_read_twiddles_wider_than_the_next_smaller_field(oracle, cid):
    c = F.BY_ID[cid]
    got = F.widest_twiddle_bits(F.s_evals(oracle, c), c)
    assert got == WIDTHS[cid]
    assert got > (1 << (c.tw_level - 1)), "case %s would pass with its twiddles cut to B%d" % (cid, 1 << (c.tw_level - 1))
    assert got <= (1 << c.tw_level)


def test_rows_read_are_inside_the_basis():
    for c in F.CASES:
        rows = F.fold_rows(c)
        assert len(rows) == c.n_fold
        for row, n in rows:
            assert 0 <= row < c.log_domain <= 64 and 0 <= n <= c.log_domain - 1 - row
    # the last level of a fold to one element has no twiddle bits and reads the row at log_domain - 1; the offset of case D is 30 .. 39
    assert F.fold_rows(F.BY_ID["D"])[-1] == (39, 0) and [r for r, _ in F.fold_rows(F.BY_ID["D"])] == list(range(30, 40))
    assert F.fold_rows(F.BY_ID["E"])[-1] == (7, 0)


def test_small_b64_folds_read_only_32_bit_twiddles(oracle):
    """Why the B64 cases have log_len >= 17: whatever the domain, a B64 fold round at log_len <= 16 reads basis entries of at most 32
    bits, so a pass that kept only the low 32 bits of a B64 twiddle -- the cut that the table product of the B8 .. B32 passes makes by
    design -- is exact on it.  (log_domain 33, log_len 17 is the first shape over 32 bits: 49.)"""
    for log_domain in (33, 40, 64):
        s = oracle.ntt_s_evals(6, log_domain)
        for L in range(1, 17):
            row = log_domain - L
            assert all(int(s[row * 64 + b]).bit_length() <= 32 for b in range(L - 1)), (log_domain, L)
    s = oracle.ntt_s_evals(6, 33)
    widths = {L: max(int(s[(33 - L) * 64 + b]).bit_length() for b in range(L - 1)) for L in (17, 19)}
    assert widths == {17: 49, 19: 64}
    s = oracle.ntt_s_evals(6, 40)
    assert max(int(s[30 * 64 + b]).bit_length() for b in range(9)) == 32
    s = oracle.ntt_s_evals(6, 64)
    assert max(int(s[56 * 64 + b]).bit_length() for b in range(7)) == 8


def schedule(tw_level, log_len, log_batch, n_challenges):
    """The pass forms of a call, from the comment in launch_fri_fold: a call without challenges is one copy; otherwise, while the pass reads
    2^14 elements or more, three interleave challenges per pass (two when only two are left to go), two challenges per pass as soon as a
    fold round is among them for twiddle fields up to B32, and everywhere else one challenge per pass."""
    if n_challenges == 0:
        return [], 1
    cur, c, out = 1 << (log_len + log_batch), 0, []
    while c < n_challenges:
        left, inter = n_challenges - c, max(log_batch - c, 0)
        form, take = "one", 1
        if cur >= (1 << 14):
            if inter >= 3:
                form, take = "inter3", 3
            elif inter == 2:
                form, take = "inter2", 2
            elif tw_level <= 5 and left >= 2:
                form, take = "ntt2", 2
        out.append(form)
        cur >>= take
        c += take
    return out, 0


def test_case_table_is_complete():
    cases = F.CASES
    assert len(cases) == 17 and [c.id for c in cases] == ["A", "B", "C", "D", "E", "F", "F2", "G", "H", "I", "J1", "J2", "K", "L1", "L2", "L3", "M"]
    assert {c.tw_level for c in cases} == {3, 4, 5, 6}
    assert {f for c in cases for f in c.passes} == {"one", "inter2", "inter3", "ntt2"}  # all but the measurement form
    assert any(c.copies == 1 and not c.passes for c in cases)
    assert any(F.n_challenges(c) == 0 for c in cases)
    assert any(c.n_fold == 0 and c.log_batch > 0 for c in cases)  # n_challenges == log_batch
    assert any(c.n_fold == c.log_len > 0 for c in cases)  # n_challenges == log_batch + log_len
    assert any(c.log_len == 0 for c in cases)
    assert any(c.log_domain - c.log_len >= 30 for c in cases)
    # B64 butterflies from 2^14 elements up stay one per pass; the grid of k_fri_pass (2048 x 256 threads) strides
    assert any(c.tw_level == 6 and c.n_fold >= 2 and c.log_len >= 14 and c.passes[-c.n_fold :] == ["one"] * c.n_fold for c in cases)
    assert any((F.in_len(c) >> 1) > 2048 * 256 and c.passes[0] == "one" for c in cases)
    # a two-level pass with both levels butterflies, and one with an interleave level in it
    assert any(c.passes[0] == "ntt2" and c.log_batch == 0 for c in cases) and any(c.passes[0] == "ntt2" and c.log_batch == 1 for c in cases)
    # both sides of the 2^14 threshold
    assert {F.in_len(c) for c in cases if c.id in ("J1", "J2")} == {1 << 14, 1 << 13}
    for c in cases:
        assert 3 <= c.tw_level <= 6 and c.log_len <= c.log_domain <= min(64, 1 << c.tw_level) and c.n_fold <= c.log_len, c.id
        assert F.in_len(c) <= (1 << 21)
        assert (c.passes, c.copies) == schedule(c.tw_level, c.log_len, c.log_batch, F.n_challenges(c)), c.id
        assert F.expected_counters(c)["ntt3"] == 0
