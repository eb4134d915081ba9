"""The claim-group evaluation group_eval (csrc/abi_group.cpp): the routes a fixed set of call sequences takes, their values and the bytes they leave.

Every sequence drives the C ABI directly -- execute() is calculate_round_evals (bn_kernel_launch), fold() the reference's PreFold
(copy_d2d of evals_0 into a fresh buffer, bn_extrapolate_line_batch there) and then in place -- on ONE region of the arena that a
NumPy array mirrors (Region of test_gpu_fold_entry.py).  The model is folded with oracle.extrapolate_line and evaluated with
oracle.round_evals: never the device's output.  Every evaluation must equal the oracle's; after the sequence the whole region --
the folded arrays, the inputs and everything between them -- equals the model byte for byte.

Routes.  A router can stay bit-exact while it sends work down a slower route, and the counter assertions of test_gpu_group.py are
inequalities.  ROUTES holds ALL 14 bn_group_counters deltas of each sequence (the final read of the region included) as literals,
recorded on the MI355X from the commit BEFORE group_eval was split into named routes, in two separate runs that agreed on every
counter: none of the 14 depends on timing, none is left out.  The refactored library must reproduce them with ==.  Every sequence
sets BN_GROUP_HT_MAX_LOG2, BN_GROUP_HT_WORK_LOG2, BN_GROUP_CHAIN_MIN_LOG2 and BN_GROUP_SPEC itself (the hosting default depends on
whether the host has VPCLMULQDQ, the chain default needs 2^21 rows).  The hosted sequences need a host with carry-less
multiplication at all (arm_counters()['ht_max'] != 0) and skip elsewhere, as tests/deferred_states.py does.

Which row fails if a branch misbehaves (route order of group_eval, then the planners):

  gate, parse, "not ours"             every single-claim suite passes through them; the refusals of parse: test_parse_refuses_*
  hosted hit (host_answer)            hosted, hosted-rest, hosted-odd-fold (hosted_evals)
  ahead hit (answer + record)         front-spec1 (spec_hits; the NEXT round's riders need the session record() refreshed)
  ahead hit lost to a foreign write   front-fill (spec_hits one lower than front-spec1, values the oracle's)
  ahead sums of other claims          front-claims (same arrays, same m and k, other claims: no hit, the values of the claims named)
  make room (legacy_to_group)         not here (no sequence leaves single-claim state behind): a plain deferred fold that moves over
                                      is test_gpu_fold_entry's interleave-8 and test_gpu_deferred_visibility's state S1
  match: ref[i] as output             every sequence from its second round on (jobs_fused)
  match: read, not as output          reread (flushed_folds from inside the evaluation; the batch in front is erased, so the ref
                                      taken before the flush must be looked up again or the values differ)
  match: unhost_touching              hosted-odd-fold (the second hand-over reads what the first left), test_gpu_deferred_visibility
  hand-over, a deferred fold riding   hosted, hosted-rest, hosted-odd-fold (hosted_started; src0 of an absorbed PreFold copy in the
                                      second hand-over of hosted-odd-fold)
  hand-over, nothing deferred         hosted (the second start, after the write-back)
  hand-over, rest folded plainly      hosted-rest (not counted in flushed_folds: its 6 are the prover's five-array folds, which are no
                                      hosted prover's expected fold, so each ends the hosting and the next evaluation starts it again)
  hosted fold, expected               hosted (hosted_folds); not the expected one: hosted-odd-fold (write-back, the device folds)
  write-back by a read; host read     hosted (hosted_writebacks 1; the read inside a current array moves nothing)
  riders (spec_jobs), record_ahead    front-spec1, front-two-z; none with BN_GROUP_SPEC=0: front-spec0
  loose array as a kind-3 job         loose-chain (jobs_fold); in the plain prefold: loose-prefold (prefolds)
  plan_chained: kind 0, degree one    disjoint-chain; second pass (shared array): piop-chain
  plan_chained: kind 4, chain, acquire  piop-chain (chains; a missing acquire or order shows in the values)
  plan_chained: kind 1                every sequence's first round; chained behind a fold: square-one-chain, square-two-chain
  plan_chained: kind 3, one / two     square-one-chain / square-two-chain (jobs_fold 1 / 1 per round for 1 / 2 arrays); an array
                                      named by no claim: loose-chain
  plan_prefold: kind 0 / 4 / 1        disjoint / piop-prefold / square-one-prefold
  plain prefold, one launch each      piop-prefold, square-one-prefold, front-two-z (prefolds: two per round, no merge)
  merged ragged prefold               front-spec1 (prefolds rises by one per round where front-two-z shows two)
  retirement, g.on                    every sequence (a fold retired twice or never shows in the bytes)

Not repeated here: session eviction past 16 provers (test_gpu_group.py::test_more_hosted_provers_than_sessions_keep_their_folds)
and the refusal of more than kGroupMaxJobs jobs, which plans without chains and then falls back to the eager kernels
(test_gpu_group_wide.py), at the sizes they need.  Not provoked, checked by reading only: the path behind a launch that
launch_group refuses (launch_refused: the folds the plain launches in front have performed are retired, the others stay deferred
and are flushed) and every HIP-error path -- there is no failure-injection switch."""
import numpy as np
import pytest

from deferred_states import env, moved
from test_gpu_fold_entry import Region

pytestmark = pytest.mark.gpu

KEYS = ("launches", "jobs_fused", "jobs_eval", "prefolds", "spec_jobs", "spec_hits", "evals", "flushed_folds", "hosted_started", "hosted_evals",
        "hosted_folds", "hosted_writebacks", "jobs_fold", "chains")
OFF = dict(BN_GROUP_HT_MAX_LOG2=0, BN_GROUP_HT_WORK_LOG2=17, BN_GROUP_CHAIN_MIN_LOG2=63, BN_GROUP_SPEC=0)
HOST6 = dict(OFF, BN_GROUP_HT_MAX_LOG2=6)  # (hosted sessions from 2^6 elements per array)
CHAIN = dict(OFF, BN_GROUP_CHAIN_MIN_LOG2=0)
_WANT = {}  # the oracle's round sums, once per (region seed, arrays, size, claims)


def evaluate(rg, offs, n_rem, comps, bc, what=""):
    """calculate_round_evals of the arrays at offs (2^n_rem elements each): the device's values must be the oracle's on the model"""
    from binius_amd.sumcheck import bivariate_product_expr, calculate_round_evals

    n = 1 << n_rem
    model = [rg.mem[o : o + n].copy() for o in offs]
    key = (tuple(offs), n_rem, tuple(comps), bc, b"".join(x.tobytes() for x in model))
    if key not in _WANT:
        rc, _WANT[key] = rg.oracle.round_evals(model, n_rem, comps, bc)
        assert rc == 0
    cache = rg.hal.__dict__.setdefault("_group_routes_exprs", {})
    for c in comps:
        if c not in cache:
            cache[c] = bivariate_product_expr(rg.hal, *c)
    coeffs, pw = [], 1
    for _ in comps:
        coeffs.append(pw)
        pw = rg.oracle.mul(pw, bc)
    got = calculate_round_evals(rg.hal, n_rem, coeffs, [rg.d(o, n) for o in offs], [cache[c] for c in comps])
    assert list(got) == list(_WANT[key]), "%s (%d variables left): the round values are not the oracle's" % (what, n_rem)


class Prover:
    """m arrays of 2^log_n elements from `base` on, m fresh buffers of half that size behind them.  named: the arrays an evaluation
    names (the others belong to the fold batch alone)."""

    def __init__(self, rg, base, m, log_n, comps, bc, named=None):
        n = 1 << log_n
        self.rg, self.m, self.comps, self.bc, self.n_rem = rg, m, comps, bc, log_n
        self.inputs = [base + j * n for j in range(m)]
        self.fresh = [base + m * n + j * (n // 2) for j in range(m)]
        self.cur, self.pre_fold = list(self.inputs), True
        self.named = list(range(m)) if named is None else named

    @staticmethod
    def elems(m, log_n):
        return 3 * m * (1 << log_n) // 2

    def execute(self, what="execute"):
        evaluate(self.rg, [self.cur[j] for j in self.named], self.n_rem, self.comps, self.bc, what)

    def fold(self, z, into=None):
        """the PreFold fold the first time (or into the buffers `into`: copy the lower halves there, fold there), in place afterwards"""
        half = 1 << (self.n_rem - 1)
        src = self.cur
        dst = self.fresh if self.pre_fold and into is None else into
        if dst is not None:
            for s, d in zip(src, dst):
                self.rg.copy(s, d, half)
        else:
            dst = src
        self.rg.fold(dst, [s + half for s in src], half, z)
        self.cur, self.pre_fold, self.n_rem = list(dst), False, self.n_rem - 1


def rounds(provers, zs, until=0, before_execute=None):
    """front-loaded rounds (execute on every prover, the challenge(s), fold on every prover) while a prover has more than `until`
    variables left.  zs: an iterator of challenges or, for provers that fold by different ones, of tuples."""
    r = 0
    while any(p.n_rem > until for p in provers):
        alive = [p for p in provers if p.n_rem > until]
        for p in alive:
            if before_execute is not None:
                before_execute(r, p)
            p.execute("round %d" % r)
        z = next(zs)
        for i, p in enumerate(alive):
            p.fold(z[i] if isinstance(z, tuple) else z)
        r += 1


def read_back(rg, off, n):
    """copy_d2h of n elements at off: the model's"""
    got = rg.hal.copy_d2h(rg.d(off, n))
    assert np.array_equal(got, rg.mem[off : off + n]), "a host read of [%d, %d) differs from the model" % (off, off + n)


# ---- the sequences: fn(rg, zs, bc) on a fresh context; the smallest shapes at which each branch exists
def seq_one(m, comps, named=None, log_n=8):
    def fn(rg, zs, bc):
        rounds([Prover(rg, 0, m, log_n, comps, bc, named)], zs)

    return fn, Prover.elems(m, log_n)


def seq_hosted(rg, zs, bc):
    """group launches at 2^8 and 2^7, the hand-over at 2^6 with the deferred fold riding on it, hosted evaluations and folds, one
    write-back forced by a read of a folded buffer beyond the current array, a second hand-over with nothing deferred, a read
    inside a current array answered by the host, then hosted to the end"""
    p = Prover(rg, 0, 4, 8, [(0, 2), (1, 3)], bc)
    rounds([p], zs, until=4)
    c = rg.hal.group_counters()
    read_back(rg, p.fresh[0], 1 << 6)
    assert rg.hal.group_counters()["hosted_writebacks"] == c["hosted_writebacks"] + 1
    p.execute("after the write-back")
    c = rg.hal.group_counters()
    read_back(rg, p.cur[1] + 2, 5)
    assert rg.hal.group_counters() == c, "a read inside a hosted prover's current array moves nothing"
    p.fold(next(zs))
    rounds([p], zs)


def seq_hosted_rest(rg, zs, bc):
    """the fold batch holds one array the evaluations never name: loose before the hand-over, folded plainly by it"""
    rounds([Prover(rg, 0, 5, 8, [(0, 1), (2, 3)], bc, named=[0, 1, 2, 3])], zs)


def seq_hosted_odd_fold(rg, zs, bc):
    """hosted at 2^6, one host fold, a hosted evaluation, then a fold OUT of place (not the expected one: the copies' ordering writes
    the host's folds back, the device folds), a second hand-over with that fold -- src0 differs from x0 -- riding on it"""
    p = Prover(rg, 0, 4, 8, [(0, 2), (1, 3)], bc)
    rounds([p], zs, until=5)
    p.execute("hosted")
    spare = Prover.elems(4, 8)
    p.fold(next(zs), into=[spare + 16 * j for j in range(4)])
    rounds([p], zs)


def seq_front(spec_z):
    def fn(rg, zs, bc):
        a = Prover(rg, 0, 3, 6, [(0, 2), (1, 2)], bc)
        b = Prover(rg, Prover.elems(3, 6), 3, 8, [(0, 2), (1, 2)], bc)
        rounds([a, b], zs if spec_z == "one" else iter(zip(zs, zs)))

    return fn, Prover.elems(3, 6) + Prover.elems(3, 8)


def seq_front_fill(rg, zs, bc):
    """round 2: a's execute has computed b's sums ahead; a fill into one of b's arrays before b's execute"""
    a = Prover(rg, 0, 3, 6, [(0, 2), (1, 2)], bc)
    b = Prover(rg, Prover.elems(3, 6), 3, 8, [(0, 2), (1, 2)], bc)

    def foreign(r, p):
        if r == 2 and p is b:
            rg.fill(b.cur[0] + 1, 2, 0x1234567)

    rounds([a, b], zs, before_execute=foreign)


def seq_front_claims(rg, zs, bc):
    """round 2: a's execute has computed b's sums ahead -- for the claims of b's last evaluation; b asks for other claims over the
    same arrays: no ahead hit, and the sums b gets are those of the claims it names"""
    a = Prover(rg, 0, 3, 6, [(0, 2), (1, 2)], bc)
    b = Prover(rg, Prover.elems(3, 6), 3, 8, [(0, 2), (1, 2)], bc)

    def other_claims(r, p):
        if r == 2 and p is b:
            b.comps = [(0, 1), (1, 2)]

    rounds([a, b], zs, before_execute=other_claims)


def seq_reread(rg, zs, bc):
    """two deferred batches, a's in front; a request that names b's folded arrays (outputs) AND a's unfolded inputs (read by a's
    fold, not its output): a's batch runs from inside the evaluation, b's moves to the front"""
    a = Prover(rg, 0, 3, 7, [(0, 1), (1, 2)], bc)
    b = Prover(rg, Prover.elems(3, 7), 3, 8, [(0, 1), (1, 2)], bc)
    a.execute()
    b.execute()
    z = next(zs)
    a.fold(z)
    b.fold(z)
    evaluate(rg, [b.cur[0], a.inputs[0], b.cur[1], a.inputs[1]], 7, [(0, 1), (2, 3)], bc, "b's outputs against a's inputs")
    rounds([a, b], zs)


SEQUENCES = {
    # name: (settings, sequence, elements of its region); the sequences of one shape (the name up to the first "-") share the region's
    # contents and so the oracle's sums
    "disjoint": (OFF, *seq_one(4, [(0, 2), (1, 3)])),
    "disjoint-chain": (CHAIN, *seq_one(4, [(0, 2), (1, 3)])),
    "hosted": (HOST6, seq_hosted, Prover.elems(4, 8)),
    "piop-chain": (CHAIN, *seq_one(4, [(0, 3), (1, 3), (2, 3)])),
    "piop-prefold": (OFF, *seq_one(4, [(0, 3), (1, 3), (2, 3)])),
    "square-one-chain": (CHAIN, *seq_one(3, [(0, 0), (1, 2)])),
    "square-two-chain": (CHAIN, *seq_one(2, [(0, 0), (1, 1)])),
    "square-one-prefold": (OFF, *seq_one(3, [(0, 0), (1, 2)])),
    "loose-chain": (CHAIN, *seq_one(5, [(0, 1), (1, 2)], named=[0, 1, 2, 3])),
    "loose-prefold": (OFF, *seq_one(5, [(0, 1), (1, 2)], named=[0, 1, 2, 3])),
    "front-spec1": (dict(OFF, BN_GROUP_SPEC=1), *seq_front("one")),
    "front-spec0": (OFF, *seq_front("one")),
    "front-two-z": (dict(OFF, BN_GROUP_SPEC=1), *seq_front("two")),
    "front-fill": (dict(OFF, BN_GROUP_SPEC=1), seq_front_fill, Prover.elems(3, 6) + Prover.elems(3, 8)),
    "front-claims": (dict(OFF, BN_GROUP_SPEC=1), seq_front_claims, Prover.elems(3, 6) + Prover.elems(3, 8)),
    "reread": (OFF, seq_reread, Prover.elems(3, 7) + Prover.elems(3, 8)),
    "hosted-rest": (HOST6, seq_hosted_rest, Prover.elems(5, 8)),
    "hosted-odd-fold": (HOST6, seq_hosted_odd_fold, Prover.elems(4, 8) + 64),
}
SHAPES = sorted({name.split("-")[0] for name in SEQUENCES})
# bn_group_counters deltas in the order of KEYS (see the module docstring for where they were recorded)
ROUTES = {
    "disjoint": (8, 14, 2, 0, 0, 0, 8, 1, 0, 0, 0, 0, 0, 0),
    "disjoint-chain": (8, 14, 2, 0, 0, 0, 8, 1, 0, 0, 0, 0, 0, 0),
    "hosted": (2, 2, 2, 0, 0, 0, 8, 0, 2, 6, 6, 2, 0, 0),
    "piop-chain": (8, 21, 3, 0, 0, 0, 8, 1, 0, 0, 0, 0, 0, 7),
    "piop-prefold": (8, 21, 3, 7, 0, 0, 8, 1, 0, 0, 0, 0, 0, 0),
    "square-one-chain": (8, 7, 9, 0, 0, 0, 8, 1, 0, 0, 0, 0, 7, 7),
    "square-two-chain": (8, 0, 16, 0, 0, 0, 8, 1, 0, 0, 0, 0, 7, 7),
    "square-one-prefold": (8, 7, 9, 7, 0, 0, 8, 1, 0, 0, 0, 0, 0, 0),
    "loose-chain": (8, 14, 2, 0, 0, 0, 8, 1, 0, 0, 0, 0, 14, 7),
    "loose-prefold": (8, 14, 2, 7, 0, 0, 8, 1, 0, 0, 0, 0, 0, 0),
    "front-spec1": (9, 24, 4, 7, 10, 5, 14, 2, 0, 0, 0, 0, 0, 0),
    "front-spec0": (14, 24, 4, 12, 0, 0, 14, 2, 0, 0, 0, 0, 0, 0),
    "front-two-z": (9, 24, 4, 12, 10, 5, 14, 2, 0, 0, 0, 0, 0, 0),
    "front-fill": (10, 24, 6, 7, 10, 4, 14, 2, 0, 0, 0, 0, 0, 0),
    "front-claims": (10, 24, 6, 7, 10, 4, 14, 2, 0, 0, 0, 0, 0, 0),
    "reread": (16, 24, 8, 12, 0, 0, 16, 3, 0, 0, 0, 0, 0, 0),
    "hosted-rest": (2, 2, 2, 1, 0, 0, 8, 6, 6, 6, 0, 0, 0, 0),
    "hosted-odd-fold": (2, 2, 2, 0, 0, 0, 8, 0, 2, 6, 5, 2, 0, 0),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_fixed_sequences_take_the_recorded_routes(oracle, name):
    import binius_amd

    settings, fn, total = SEQUENCES[name]
    seed = SHAPES.index(name.split("-")[0])
    stream = oracle.random_scalars(0x6E0D + seed, 24)
    with env(**settings):
        with binius_amd.Context(0, total + 4096) as hal:
            if settings["BN_GROUP_HT_MAX_LOG2"] and hal.arm_counters()["ht_max"] == 0:
                pytest.skip("hosted sessions need the host tail: this host has no PCLMULQDQ or BN_HOST_TAIL=0 is set")
            rg = Region(hal, oracle, 0x6E00 + seed, total)
            before = hal.group_counters()
            fn(rg, iter(stream[1:]), stream[0])
            rg.check()
            after = hal.group_counters()
    got = tuple(after[k] - before[k] for k in KEYS)
    print("ROUTE", repr(name), got)
    assert name in ROUTES, "no recorded route"
    assert got == ROUTES[name], (name, "recorded -> got", moved(dict(zip(KEYS, ROUTES[name])), dict(zip(KEYS, got))))


# ---- the argument checks of parse: "not handled", nothing of the group path moves, the single-claim path answers
def _recorded(hal, rg, offs, n_rem, comps, bc):
    from binius_amd.sumcheck import bivariate_product_expr, round_eval_kernel

    coeffs = [1, bc]
    exprs = [bivariate_product_expr(hal, *c) for c in comps]
    kernel, mem_maps = round_eval_kernel(n_rem, coeffs, [rg.d(o, 1 << n_rem) for o in offs], exprs)
    ops, ret_ids, log_chunks = hal.record(kernel, mem_maps)
    return mem_maps, ops, ret_ids, log_chunks


def _refused(oracle, seed, mutate, model_of):
    import binius_amd

    n_rem, comps, n = 6, [(0, 2), (1, 3)], 1 << 6
    offs = [j * n for j in range(4)]
    bc = oracle.random_scalars(0x6E1D + seed, 1)[0]
    with env(**OFF):
        with binius_amd.Context(0, 4 * n + 4096) as hal:
            rg = Region(hal, oracle, 0x6E10 + seed, 4 * n)
            mem_maps, ops, ret_ids, log_chunks = _recorded(hal, rg, offs, n_rem, comps, bc)
            mutate(rg, mem_maps, ops)
            before = hal.group_counters()
            got = hal.kernel_launch(mem_maps, ops, ret_ids, log_chunks)
            assert hal.group_counters() == before, "a request parse refuses moves nothing of the group path"
            rc, want = oracle.round_evals(model_of([rg.mem[o : o + n].copy() for o in offs]), n_rem, comps, bc)
            assert rc == 0 and list(got) == list(want)
            rg.check()


def test_parse_refuses_a_local_defined_twice(oracle):
    def mutate(rg, mem_maps, ops):
        first = [i for i, o in enumerate(ops) if o["op"] == "add"][0]
        ops.insert(first + 1, dict(ops[first]))

    _refused(oracle, 0, mutate, lambda arrays: arrays)


def test_parse_refuses_a_sum_over_one_local_and_one_mapped_half(oracle):
    """the first claim's sum at infinity reads array 2's mapped upper half where its Local stands: (a_0 + a_1) * b_1 -- the
    oracle's value at infinity for an array 2 whose lower half is zero"""

    def mutate(rg, mem_maps, ops):
        last_add = [i for i, o in enumerate(ops) if o["op"] == "add"][-1]
        op = ops[last_add + 2]  # (decl_value, then the first claim's sum)
        assert op["op"] == "sum"
        rows = list(op["rows"])
        rows[2] = (3 * 2 + 1, rows[2][1], rows[2][2])
        op["rows"] = rows

    def model_of(arrays):
        arrays[2][: arrays[2].shape[0] // 2] = 0
        return arrays

    # (the value at 1 of claim 0 does not read array 2's lower half, claim 1 does not read array 2 at all)
    _refused(oracle, 1, mutate, model_of)


def test_parse_refuses_two_arrays_sharing_a_lower_half(oracle):
    def mutate(rg, mem_maps, ops):
        mem_maps[3 * 1] = mem_maps[0]

    def model_of(arrays):
        arrays[1][: arrays[1].shape[0] // 2] = arrays[0][: arrays[0].shape[0] // 2]
        return arrays

    _refused(oracle, 2, mutate, model_of)
