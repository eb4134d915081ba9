"""Does the device's "is this table a tensor expansion" look at EVERY entry?

The weighted shadow of the literal MLE-check (csrc/abi_kernels.cpp "weighted shadow") replaces the caller's indicator table by the ratios
rho_k = eq[2^k] / eq[0] from the first fold on -- if shadow_check_table (csrc/abi.cpp) says the table has that structure everywhere.  The
answer comes from k_check_tensor and k_check_tensor_head (csrc/kernels_misc.hip), the one place in the project where a kernel answers yes or
no: a wrong "yes" raises nothing, every later round polynomial is simply that of another table, and every test that hands in a genuine
expansion stays green.  So the tables here are wrong in ONE comparison each (tests/tensor_check_ref.py isolate(), pinned entry by entry in
tests/test_oracle_tensor_check.py) and each one must be refused.

The driver is the literal prover behind its handle (BN_MLECHECK=eager, BN_MLECHECK_SHADOW=1): evaluate, fold, evaluate.  The check runs when the
first fold arrives; its verdict shows in the context's counters -- a refused table: shadow_created +1, shadow_rounds +1, shadow_dropped +1;
an accepted one: +1, +2, +0.  One context for the module, so that a refusal is followed by an acceptance and the other way round many
times over: the flag the kernels raise is cleared by the host after a "no" and by nobody else.

Read off k_check_tensor / k_check_tensor_head / check_tensor_layout as they stand, and what each probe below holds in place:
  * the loop `for (i0 = lo + part * 1024 + tid; i0 < hi && i0 < n; i0 += n_wg * 1024)`: a bound one stride short, or a stride one workgroup
    too long, leaves out the last trip -- `trip == last` probes of every range >= 11, and each range's last entry;
  * the mask `in = i < hi && i < n` of the four entries a lane keeps in flight (i0 + 256 j): ranges 8 and 9 are shorter than the 1024
    entries of one trip, so j = 1 .. 3 (range 8) and j = 2, 3 (range 9) must stay out and j = 0 (and 1) must stay in -- the K = 9 sweep
    probes every entry of range 8, the structured sets lanes 0, 63, 64, 255 of every j that is inside; a mask that were `i0 + 256 j < hi`
    with the wrong j, or dropped a slot, accepts one of them;
  * the lookups `first_wg[k]`, `first_wg[k + 1]`: workgroup -> range by the prefix sums of check_tensor_layout (one workgroup per 4096
    entries, 1 .. 512 per range).  Off by one range, or `part` taken from the wrong prefix, and either the first entries of a range
    (2^k + 1, lanes 0 .. 255 of part 0) or those of its LAST workgroup (part = n_wg - 1, K >= 14) go unvisited;
  * `want.x != g.x || want.y != g.y || want.z != g.z || want.w != g.w`: test_each_word_is_compared flips bit 0 and bit 31 of each 32-bit
    word of one entry that no other comparison reads;
  * the head kernel: `i >= 1 && i < n`, i = threadIdx.x of 256, kt = top bit of i, the generic product -- all of 1 .. 255 at K = 9.
Narrow any of these so that one class of entries is skipped and at least one named probe turns from refused to accepted: for the index
arithmetic, tests/test_oracle_tensor_check.py shows it on a model of the partition (tensor_check_ref.visits) -- every narrowing listed there
leaves out an entry that is probed here, at every size at which it leaves out anything.

Not reached: the cap of 512 workgroups per range (k >= 22, tables of n_vars >= 24).  There only the trip count of the loop differs -- 8 and
more instead of 4 -- the strides and masks are the ones exercised here."""
import numpy as np
import pytest

import adversarial
import tensor_check_ref as T
from test_gpu_mlecheck_shadow import _run, upload

pytestmark = pytest.mark.gpu

COMPS = [(0, 1)]
SUMS = [0x0123456789ABCDEF0FEDCBA987654321]  # (the literal prover does not validate its claim; transcripts are compared with an oracle fed the same)
MAX_N_VARS = 18
REFUSED, ACCEPTED = (1, 1, 1), (1, 2, 0)  # (shadow_created, shadow_rounds, shadow_dropped) of evaluate, fold, evaluate


class Rig:
    """One context; per n_vars two random multilinears (uploaded once), room for the table (uploaded per probe) and scratch."""

    def __init__(self, oracle, hal):
        self.oracle, self.hal, self.alloc, self.sizes = oracle, hal, hal.dev_alloc(), {}
        self.bc, self.z = oracle.random_scalars(0x7E5700, 2)

    def size(self, n_vars):
        if n_vars not in self.sizes:
            o = self.oracle
            mls = [o.random_b128(0x7E5000 + 16 * n_vars + j, 1 << n_vars) for j in range(2)]
            coords = o.random_scalars(0x7E5100 + n_vars, n_vars)
            self.sizes[n_vars] = {
                "mls": mls, "d": [upload(self.hal, self.alloc, x) for x in mls], "eq": self.alloc.alloc(1 << (n_vars - 1)),
                "scratch": self.alloc.alloc(3 << (n_vars - 1)), "coords": coords, "table": T.expansion(coords[: n_vars - 1]),
            }
        return self.sizes[n_vars]

    def _counters(self):
        c = self.hal.arm_counters()
        return c["shadow_created"], c["shadow_rounds"], c["shadow_dropped"]

    def _begin(self, n_vars, table, coords):
        from binius_amd._host import MlecheckProver

        s = self.size(n_vars)
        assert table.shape == (1 << (n_vars - 1), 2)
        self.hal.copy_h2d(table, s["eq"])  # (a write into the table ends whatever the last instance left behind)
        before = self._counters()
        return s, before, MlecheckProver(self.hal, n_vars, s["d"], s["eq"], coords, s["scratch"], COMPS, SUMS)

    def verdict(self, n_vars, table):
        """Counter deltas of evaluate, fold, evaluate on this table."""
        _, before, prover = self._begin(n_vars, table, self.size(n_vars)["coords"])
        try:
            prover.execute(self.bc)
            prover.fold(self.z)
            prover.execute(self.bc)
        finally:
            prover.close()
        return tuple(a - b for a, b in zip(self._counters(), before))

    def prove(self, n_vars, table, coords):
        """The whole literal prove against the oracle's on the same table; returns the counter deltas."""
        o = self.oracle
        ch = o.random_scalars(0x7E5200 + n_vars, n_vars)
        s, before, prover = self._begin(n_vars, table, coords)
        try:
            got = []
            for r in range(n_vars):
                got.append(prover.execute(self.bc))
                prover.fold(ch[r])
            finals = prover.finish()
        finally:
            prover.close()
        delta = tuple(a - b for a, b in zip(self._counters(), before))
        want_coeffs, want_finals = o.bivariate_mlecheck_prove([x.copy() for x in s["mls"]], n_vars, table.copy(), coords, COMPS, SUMS, self.bc, ch)
        assert got == want_coeffs
        assert finals == want_finals
        return delta


@pytest.fixture(scope="module")
def rig(oracle):
    import binius_amd

    env = pytest.MonkeyPatch()
    env.setenv("BN_MLECHECK", "eager")  # the literal trait-call sequence
    env.setenv("BN_MLECHECK_SHADOW", "1")  # (read when the context is made)
    try:
        with binius_amd.Context(0, 5 << MAX_N_VARS) as hal:
            yield Rig(oracle, hal)
    finally:
        env.undo()


def refuse_all(rig, K, probes, every=32):
    """probes: (table, what) pairs, each of which must be refused; a genuine table must be accepted before the first, after every
    `every` refusals and after the last."""
    n_vars, good = K + 1, rig.size(K + 1)["table"]
    assert rig.verdict(n_vars, good) == ACCEPTED, "K = %d: the genuine table was refused" % K
    n = 0
    for table, what in probes:
        got = rig.verdict(n_vars, table)
        assert got == REFUSED, "ACCEPTED a table that is no tensor expansion -- %s (created, rounds, dropped = %s)" % (what, got)
        n += 1
        if n % every == 0:
            got = rig.verdict(n_vars, good)
            assert got == ACCEPTED, "K = %d: the genuine table was refused after %d refusals, the last for %s (%s)" % (K, n, what, got)
    got = rig.verdict(n_vars, good)
    assert got == ACCEPTED, "K = %d: the genuine table was refused after %d refusals (%s)" % (K, n, got)
    return n


def test_every_entry_of_a_small_table(rig):
    """K = 9, the smallest table that gets a shadow: every entry once.  1 .. 255 are the head kernel's, 256 .. 511 range 8, whose one
    workgroup has three of its four slots masked out; powers of two and entry 0 are altered alone (the defining entries: their ratio
    changes with them, what fails is what is built on them)."""
    K, t = 9, rig.size(10)["table"]

    def probes():
        yield T.alter(t, 0), "K = 9, p = 0: entry 0 altered, every ratio changes"
        for p in range(1, 1 << K):
            if p & (p - 1):
                yield T.isolate(t, p), T.describe(K, p)
            else:
                yield T.alter(t, p), T.describe(K, p) + " (defining entry, altered alone)"

    assert refuse_all(rig, K, probes()) == 512


@pytest.mark.parametrize("K", [10, 11, 12, 13, 14, 17])
def test_structured_entries(rig, K):
    """Per range k = 8 .. K - 1, dealt to n_wg = clamp(2^k / 4096, 1, 512) workgroups of 1024 entries per trip: first and last workgroup,
    first and last trip, each of the four slots in flight, lanes 0, 63, 64, 255; each range's second and last entry; five entries of
    the head.  K = 14 is the first size with a range dealt to two workgroups, K = 17 has ranges with 2, 4, 8 and 16.  (The cap of 512
    workgroups, k >= 22 and n_vars >= 24, is not reached: see the module's docstring.)"""
    t = rig.size(K + 1)["table"]
    probes = T.probe_indices(K)  # (the layout is restated there and pinned in numbers by the CPU suite, not asked of the code under test)
    assert refuse_all(rig, K, ((T.isolate(t, p), T.describe(K, p)) for p in probes)) == len(probes)


def test_each_word_is_compared(rig):
    """One entry of the top range -- nobody's predecessor, so no other comparison can rescue a word that is not looked at -- with one
    bit flipped: the lowest and the highest of each 32-bit word."""
    K, t = 13, rig.size(14)["table"]
    p = (1 << 12) + 2741
    refuse_all(rig, K, ((T.flip(t, p, bit), T.describe(K, p) + ", bit %d flipped" % bit) for bit in (0, 31, 32, 63, 64, 95, 96, 127)))


@pytest.mark.parametrize("n_vars,p,regime", [
    (10, 77, (6, 0, 0)),                                       # the head
    (10, 256 + 133, (8, 0, 0)),                                # range 8
    (14, (1 << 12) + 3 * 1024 + 2 * 256 + 64, (12, 0, 3)),     # range 12, last trip
    (15, (1 << 13) + 1024 + 2048 + 256 + 63, (13, 1, 1)),      # the second workgroup of range 13 (K = 14), its second trip
    (15, (1 << 14) - 1, (13, 1, 3)),                           # the last entry of the table
])
def test_refused_tables_get_the_literal_transcript(oracle, monkeypatch, n_vars, p, regime):
    """What the probes above take on trust from the counters: a "no" hands the instance to kernels that use the table AS GIVEN -- the
    whole transcript equals the oracle's on the same altered table."""
    assert T.where(p)[:3] == regime  # (range, workgroup of the range, trip)

    def spoil(t):
        t = T.isolate(t, p)
        assert T.failing(t) == [p]
        return t

    c = _run(oracle, monkeypatch, n_vars, 2, COMPS, 0x7E5300 + n_vars, table=spoil, reps=1)
    assert (c["shadow_created"], c["shadow_rounds"], c["shadow_dropped"]) == REFUSED, T.describe(n_vars - 1, p)


def test_degenerate_and_edge_coordinates(rig):
    """A coordinate 0 or 1 has no ratio (eq[2^k] = 0, or eq[0] = 0): the host gives up before the kernel runs, the shadow ends with
    the first fold and the literal kernels answer.  Then coordinates from the corners of the tower (its subfields' generators, the top
    basis element, all ones) through the host's one-inversion ratios and the nibble tables the kernel builds from them: the shadow
    serves every round."""
    n_vars = 12
    K, base = n_vars - 1, rig.size(n_vars)["coords"]
    for pos in (0, 7, 8, K - 1):
        for v in (0, 1):
            coords = list(base)
            coords[pos] = v
            table = T.expansion(coords[:K])
            assert T.failing(table) is None
            assert rig.prove(n_vars, table, coords) == REFUSED, "coordinate %d = %d" % (pos, v)
    edge = [x for x in adversarial.EDGE_SCALARS if x not in (0, 1)]
    coords = [edge[i % len(edge)] for i in range(n_vars)]
    table = T.expansion(coords[:K])
    assert T.failing(table) == []
    created, rounds, dropped = rig.prove(n_vars, table, coords)
    assert (created, rounds) == (1, n_vars), (created, rounds, dropped)


def test_a_refusal_does_not_outlive_its_instance(rig):
    """A refused table keeps the SMALLER rounds of its instance from starting a shadow of their own (blocked_below); an instance at
    least as large lifts that.  (The smaller instance in between cannot be told from a later round of the refused one: its transcript
    is right either way, its counters are nobody's business.)"""
    big, small = rig.size(14), rig.size(12)
    p = (1 << 12) + 1024 + 63
    assert rig.prove(14, T.isolate(big["table"], p), big["coords"]) == REFUSED
    rig.prove(12, small["table"], small["coords"])
    created, rounds, dropped = rig.prove(14, big["table"], big["coords"])
    assert (created, rounds) == (1, 14), (created, rounds, dropped)
