"""The case table of bn_fri_fold's parity tests, shared by tests/test_oracle_fri_cases.py (which pins the table on the CPU) and
tests/test_gpu_fri_fold.py (which runs it on the device).

launch_fri_fold (binius_amd/csrc/kernels_misc.hip) cuts a call into passes of five forms, and `Context.fri_counters()`
(bn_fri_counters) says which ones a call launched.  A case is (tw_level, log_domain, log_len, log_batch, n_fold) -- the call folds
2^(log_len + log_batch) elements with log_batch + n_fold challenges down to 2^(log_len - n_fold) -- plus the pass forms it must be
served by, in launch order, written out by hand: a case that was chosen to reach a kernel fails when a threshold moves and it stops
reaching it.

What a B64 case needs: a fold round at log_len = L reads the first L - 1 entries of row log_domain - L of the 64 x 64 twiddle basis, and
for B64 those stay within 32 bits for every L <= 16 at any log_domain (pinned in tests/test_oracle_fri_cases.py).  A B64 pass that cut
its twiddles to 32 bits -- which the table product of the B8 .. B32 passes does by design -- would pass any smaller B64 case, so the cases
that stand for B64 have log_len >= 17.
"""
from collections import namedtuple

import numpy as np

FORMS = ("one", "inter2", "inter3", "ntt2", "ntt3")  # the keys of Context.fri_counters(), next to "copies"

FriCase = namedtuple("FriCase", "id tw_level log_domain log_len log_batch n_fold passes copies why")

CASES = [
    FriCase("A", 6, 33, 19, 0, 3, ["one", "one", "one"], 0, "B64 twiddles of 64 bits; butterflies stay one per pass at 2^19"),
    FriCase("B", 6, 34, 20, 1, 1, ["one", "one"], 0,
            "2^21 in: the first pass has 2^20 outputs and the grid of k_fri_pass strides; one interleave and one butterfly pass of k_fri_pass<6>"),
    FriCase("C", 6, 33, 17, 3, 2, ["inter3", "one", "one"], 0, "49-bit twiddles behind a three-level interleave pass"),
    FriCase("D", 6, 40, 10, 2, 10, ["one", "one", "one", "one", "one", "one", "one", "one", "one", "one", "one", "one"], 0,
            "fold to one element (the last level has no twiddle bits); basis rows 30 to 39"),
    FriCase("E", 3, 8, 8, 2, 8, ["one", "one", "one", "one", "one", "one", "one", "one", "one", "one"], 0, "the whole B8 domain down to one element"),
    FriCase("F", 3, 8, 8, 7, 3, ["inter3", "one", "one", "one", "one", "one", "one", "one"], 0, "B8 behind a wide batch"),
    FriCase("F2", 3, 6, 5, 0, 2, ["one", "one"], 0, "log_domain > log_len for B8"),
    FriCase("G", 4, 16, 14, 1, 3, ["ntt2", "one", "one"], 0, "an interleave and a butterfly level in one pass, B16"),
    FriCase("H", 5, 17, 16, 0, 4, ["ntt2", "ntt2"], 0, "32-bit twiddles in the table product of the two-level pass"),
    FriCase("I", 5, 15, 14, 2, 1, ["inter2", "one"], 0, "a single butterfly at 2^14"),
    FriCase("J1", 5, 14, 14, 0, 2, ["ntt2"], 0, "exactly at the 2^14 threshold"),
    FriCase("J2", 5, 14, 13, 0, 2, ["one", "one"], 0, "just below the threshold"),
    FriCase("K", 5, 12, 10, 0, 0, [], 1, "no challenge: the copy"),
    FriCase("L1", 6, 40, 0, 3, 0, ["one", "one", "one"], 0, "log_len = 0"),
    FriCase("L2", 5, 12, 10, 3, 0, ["one", "one", "one"], 0, "interleave only, small"),
    FriCase("L3", 4, 12, 12, 4, 0, ["inter3", "one"], 0, "interleave only, large"),
    FriCase("M", 5, 18, 14, 4, 2, ["inter3", "ntt2", "one"], 0, "every form in one call"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def n_challenges(c):
    return c.log_batch + c.n_fold


def in_len(c):
    return 1 << (c.log_len + c.log_batch)


def out_len(c):
    return 1 << (c.log_len - c.n_fold)


def expected_counters(c):
    """The difference in Context.fri_counters() across the call."""
    d = {k: c.passes.count(k) for k in FORMS}
    d["copies"] = c.copies
    assert sum(d.values()) == len(c.passes) + c.copies
    return d


def fold_rows(c):
    """(row, entries) of the twiddle basis that each fold round reads: round at log_len = L reads the first L - 1 entries of row log_domain - L."""
    return [(c.log_domain - L, L - 1) for L in range(c.log_len, c.log_len - c.n_fold, -1)]


def widest_twiddle_bits(s_evals, c):
    """Bit length of the widest basis entry the case reads (0: it reads none)."""
    stride = 64
    return max([int(s_evals[row * stride + b]).bit_length() for row, n in fold_rows(c) for b in range(n)], default=0)


# ---- inputs and references: computed once per process, handed out read-only
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def _seed(c):
    return 0xF01D00 + 16 * CASES.index(c)


def s_evals(oracle, c):
    key = ("s", c.tw_level, c.log_domain)
    if key not in _cache:
        _cache[key] = _frozen(oracle.ntt_s_evals(c.tw_level, c.log_domain))
    return _cache[key]


def data(oracle, c):
    key = ("data", c.id)
    if key not in _cache:
        _cache[key] = _frozen(oracle.random_b128(_seed(c), in_len(c)))
    return _cache[key]


def challenges(oracle, c):
    return oracle.random_scalars(_seed(c) + 1, n_challenges(c))


def reference(oracle, c, chs=None):
    """oracle.fri_fold of the case's data with the case's challenges (or `chs`)."""
    chs = challenges(oracle, c) if chs is None else list(chs)
    assert len(chs) == n_challenges(c)
    key = ("ref", c.id, tuple(chs))
    if key not in _cache:
        out = oracle.arr(out_len(c))
        assert oracle.fri_fold(s_evals(oracle, c), c.tw_level, c.log_domain, c.log_len, c.log_batch, chs, data(oracle, c), out) == 0
        _cache[key] = _frozen(np.ascontiguousarray(out))
    return _cache[key]
