"""The fold entry point bn_extrapolate_line_batch_scaled (csrc/abi_fold.cpp): the branches of its route order and of the flush
that no other suite pins, and the routes a fixed set of call sequences takes.

Memory.  Every case keeps its buffers in ONE region of the arena, mirrored by one NumPy array that is folded with
oracle.extrapolate_line (as tests/deferred_states.py does): never the device's own output, never another context's.  After the
case the region is compared byte for byte.

Routes.  A router can stay bit-exact while it sends everything down the slow path, so ROUTES holds the counter deltas of fixed
call sequences on a default context -- recorded once, on the MI355X, from the commit BEFORE the entry point was split into a
request and named routes, and written here as literals.  Only counters that do not depend on timing are compared: `hits`,
`expired` and the `ns_*` fields of bn_arm_counters depend on how fast the host arrives at an armed kernel and are left out, and so
is `cancels`, which counts armed kernels and so follows the same timing.  Nothing here runs with profiling on (it changes routes).

Which test fails if a branch of the entry point or of the flush misbehaves (found by reading the tests):

  wide batch in pieces            test_gpu_group_wide::test_wide_prover_eager_path (100 / 128 arrays, transcripts); bytes: here
  second chained fold (pend2)     test_gpu_two_round::test_two_round_launches_answer_two_rounds_each (hosted == launches)
  copies absorbed, all            test_gpu_two_round::test_compiled_prover_same_transcript... (PreFold inputs unmodified)
  absorption clash (copy chain)   test_gpu_lazy_vs_eager::test_random_call_sequences ("chain", against eager); against the model: here
  absorption, some but not all    here (no other suite issues a copy the batch does not own between a PreFold copy and its fold)
  claim groups                    test_gpu_group*, test_gpu_deferred_visibility (state S2)
  independent second prover       test_gpu_group::test_front_loaded_batch_vs_oracle[sizes [6, 8], ks [1, 1]] (evals on the group path)
  host tail fold                  test_gpu_two_round::test_host_tail_takes_the_last_rounds (ht_rounds)
  ... unabsorbed copies first     test_gpu_two_round::test_deferred_copies_and_the_host_tail_keep_their_order
  resident tail continues         test_gpu_caller_stream (launches of profile class `tail`), test_gpu_sumcheck::test_rounds_through_resident_tail
  armed round continues / cancel  test_gpu_sumcheck::test_armed_rounds_serve_the_small_rounds, ::test_armed_round_with_other_arrays_is_cancelled
  pre survives, fin_y dies        test_gpu_two_round::test_two_round_launches..., ::test_two_round_path_survives_foreign_calls
  shadow survives, table check    test_gpu_mlecheck_shadow::test_literal_mlecheck_runs_on_the_shadow, ::test_a_table_that_is_no_tensor_expansion...
  shadow_advance                  test_gpu_mlecheck_shadow::test_literal_mlecheck_runs_on_the_shadow (shadow_rounds == 2 n_vars, transcripts)
  flush_pending, park             test_gpu_deferred_visibility (state S1); eager flush at once: smoke(), test_gpu_lazy_vs_eager
  publish-tiny, one fold          test_gpu_sumcheck::test_tiny_fold_results_are_mirrored_to_the_host; scaled: ::test_extrapolate_line_batch_scaled[1, 2]
  publish-tiny, two folds; fin_y  test_gpu_two_round::test_two_round_launches... (BN_HOST_TAIL=0: the final reads of _drive)
  host-valued mirror (host tail)  test_gpu_two_round::test_host_tail_takes_the_last_rounds (the final reads of _drive)
  scaled fold flushed             test_gpu_sumcheck::test_extrapolate_line_batch_scaled[5 ..] (by a read); by a call that is no read: here
  invalid arguments               test_gpu_sumcheck::test_extrapolate_line_batch_scaled_validation (two of them); all, with the counters: here"""
import ctypes as C

import numpy as np
import pytest

from deferred_states import env, moved

pytestmark = pytest.mark.gpu

ARM_KEYS = ("hosted", "two_round", "shadow_created", "shadow_rounds", "shadow_dropped", "ht_started", "ht_rounds", "ht_flushed")


def elems(values):
    return np.array([(v & ((1 << 64) - 1), v >> 64) for v in values], dtype=np.uint64).reshape(-1, 2)


class Region:
    """`total` elements of the arena and the model of the same elements; every call goes to both"""

    def __init__(self, hal, oracle, seed, total):
        self.hal, self.oracle = hal, oracle
        self.mem = oracle.random_b128(0xF01D0000 + seed, total)
        hal.sync()
        self.dev = hal.dev_alloc().alloc(total)
        hal.copy_h2d(self.mem, self.dev)

    def d(self, off, n):
        return self.dev.slice(off, off + n)

    def copy(self, src, dst, n):
        self.hal.copy_d2d(self.d(src, n), self.d(dst, n))
        self.mem[dst : dst + n] = self.mem[src : src + n].copy()

    def fill(self, off, n, value):
        self.hal.fill(self.d(off, n), value)
        self.mem[off : off + n] = elems([value])[0]

    def fold(self, x0, x1, n, z, mask=0, hi_scale=0):
        """one batch: x0[i] | x1[i] -> x0[i], n elements each; bit i of mask: the upper half of the result times hi_scale"""
        if mask:
            self.hal.extrapolate_line_batch_scaled([self.d(o, n) for o in x0], [self.d(o, n) for o in x1], z, mask, hi_scale)
        else:
            self.hal.extrapolate_line_batch([self.d(o, n) for o in x0], [self.d(o, n) for o in x1], z)
        for i, (lo, hi) in enumerate(zip(x0, x1)):
            f = self.mem[lo : lo + n].copy()
            assert self.oracle.extrapolate_line(f, self.mem[hi : hi + n].copy(), z) == 0
            if (mask >> i) & 1:
                f[n // 2 :] = self.oracle.mul_vec(np.ascontiguousarray(f[n // 2 :]), elems([hi_scale] * (n // 2)))
            self.mem[lo : lo + n] = f

    def check(self):
        self.hal.sync()
        got = self.hal.copy_d2h(self.dev)
        if not np.array_equal(got, self.mem):
            raise AssertionError("device memory differs from the model at element %d" % int(np.nonzero((got != self.mem).any(axis=1))[0][0]))


def counters(hal):
    c = {"arm." + k: v for k, v in hal.arm_counters().items()}
    c.update({"group." + k: v for k, v in hal.group_counters().items()})
    return c


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, 1 << 16)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def hal_no_group():
    import binius_amd

    with env(BN_GROUP=0):
        ctx = binius_amd.Context(0, 1 << 16)
    yield ctx
    ctx.close()


# ---- memory: the branches no other suite compares byte for byte
@pytest.mark.parametrize("count", [33, 65])
def test_wide_batch_runs_in_pieces(hal_no_group, oracle, count):
    """More arrays than one launch's 32 where the claim groups do not apply (BN_GROUP=0): pieces of 32, one and two piece boundaries
    crossed, the last piece a single array.  Arrays of 2^4 elements, folded in place."""
    hal, n = hal_no_group, 8
    rg = Region(hal, oracle, count, 2 * n * count + 64)
    z = oracle.random_scalars(0xF01D + count, 1)[0]
    before = counters(hal)
    rg.fold([2 * n * j for j in range(count)], [2 * n * j + n for j in range(count)], n, z)
    rg.check()
    assert not [k for k in moved(before, counters(hal)) if k.startswith("group.")], "BN_GROUP=0: nothing of the group path moves"


@pytest.mark.parametrize("mask", [1, 2, 3])
def test_scaled_fold_flushed_by_a_foreign_call(hal, oracle, mask):
    """A deferred scaled fold that a foreign call (not a host read: no publishing launch) forces out: the plain fold, then one
    scale pass per marked array."""
    n = 32
    rg = Region(hal, oracle, 0x100 + mask, 6 * n)
    z, hs, v = oracle.random_scalars(0xF02D + mask, 3)
    rg.fold([0, 2 * n], [n, 3 * n], n, z, mask, hs)
    rg.fill(4 * n, n, v)
    rg.check()


def test_copy_chain_is_not_absorbed(hal, oracle):
    """s -> d1 -> d2, then the fold of d1 and d2: absorbing the second copy would read d1 while the batch writes it.  Both copies
    run, in issue order, before the fold."""
    n = 32
    rg = Region(hal, oracle, 0x200, 3 * 64)
    s, d1, d2 = 0, 64, 128
    z = oracle.random_scalars(0xF03D, 1)[0]
    rg.copy(s, d1, n)
    rg.copy(d1, d2, n)
    rg.fold([d1, d2], [s + n, s + n], n, z)
    rg.check()


@pytest.mark.parametrize("count", [2, 3])
def test_partial_absorption_runs_every_copy_in_issue_order(hal, oracle, count):
    """Deferred copies of which the batch could absorb all but one: none is absorbed.  The one in the middle reads what the first
    wrote, so the order shows.  count = 2 parks in the single-claim slot (the copies run in its flush), count = 3 is the claim
    groups' (the copies run before the batch is handed over)."""
    n = 16
    rg = Region(hal, oracle, 0x300 + count, (2 * count + count + 1) * n)
    ins = [2 * n * j for j in range(count)]
    fresh = [2 * n * count + n * j for j in range(count)]
    spare = 3 * n * count
    z = oracle.random_scalars(0xF04D + count, 1)[0]
    rg.copy(ins[0], fresh[0], n)
    rg.copy(fresh[0], spare, n)  # (not a destination of the batch; reads the first copy's destination)
    for j in range(1, count):
        rg.copy(ins[j], fresh[j], n)
    rg.fold(fresh, [o + n for o in ins], n, z)
    rg.check()


def test_invalid_arguments_are_rejected_and_move_nothing(hal, oracle):
    """Null pointers, a scale mask beyond the batch, an odd length with a mask, a mask without a scale, a scaled batch of more than
    32 arrays, more arrays than BN_FOLD_CALL_MAX: BN_ERR_INPUT_VALIDATION before anything is looked at -- no counter moves, and a
    fold that was deferred before the calls is still performed exactly once."""
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION, F128, lib, to_f128

    n = 16
    rg = Region(hal, oracle, 0x400, 8 * n)
    z0 = oracle.random_scalars(0xF05D, 1)[0]
    rg.fold([0, 2 * n], [n, 3 * n], n, z0)  # (deferred: what the rejected calls must leave alone)
    before = counters(hal)
    z, hs = to_f128(3), to_f128(5)
    wide = 257
    p0 = (C.c_void_p * wide)(*([rg.d(4 * n, n).ptr] * wide))
    p1 = (C.c_void_p * wide)(*([rg.d(5 * n, n).ptr] * wide))
    f = lib().bn_extrapolate_line_batch_scaled
    NP, NF = C.POINTER(C.c_void_p)(), C.POINTER(F128)()
    cases = {
        "null ctx": (None, p0, p1, 1, n, C.byref(z), 0, NF),
        "null z": (hal._h, p0, p1, 1, n, NF, 0, NF),
        "null evals_0": (hal._h, NP, p1, 1, n, C.byref(z), 0, NF),
        "null evals_1": (hal._h, p0, NP, 1, n, C.byref(z), 0, NF),
        "mask beyond the batch": (hal._h, p0, p1, 2, n, C.byref(z), 4, C.byref(hs)),
        "odd length with a mask": (hal._h, p0, p1, 1, n - 1, C.byref(z), 1, C.byref(hs)),
        "mask without a scale": (hal._h, p0, p1, 1, n, C.byref(z), 1, NF),
        "scaled batch of 33": (hal._h, p0, p1, 33, n, C.byref(z), 1, C.byref(hs)),
        "count > BN_FOLD_CALL_MAX": (hal._h, p0, p1, wide, n, C.byref(z), 0, NF),
    }
    for name, args in cases.items():
        assert f(*args) == BN_ERR_INPUT_VALIDATION, name
    assert lib().bn_extrapolate_line_batch(hal._h, p0, p1, wide, n, C.byref(z)) == BN_ERR_INPUT_VALIDATION
    assert counters(hal) == before
    rg.check()


# ---- routes: fixed call sequences, counter deltas recorded from the commit before the split (see the module docstring)
def upload(hal, alloc, arr):
    d = alloc.alloc(arr.shape[0])
    hal.copy_h2d(arr, d)
    return d


def seq_sumcheck(oracle, n_vars):
    """one compiled single-claim sumcheck (first fold out of place into scratch, later folds in place, finish() reads the results)"""
    import binius_amd
    from binius_amd._host import SumcheckPlan

    mls = [oracle.random_b128(0xF0600000 + 64 * n_vars + j, 1 << n_vars) for j in range(2)]
    rc, claim = oracle.inner_product(mls[0], 7, mls[1])
    assert rc == 0
    stream = oracle.random_scalars(0xF06D + n_vars, n_vars + 1)
    want = oracle.bivariate_sumcheck_prove([x.copy() for x in mls], n_vars, [(0, 1)], [claim], stream[0], stream[1:])
    with binius_amd.Context(0, 8 << n_vars) as hal:
        alloc = hal.dev_alloc()
        d = [upload(hal, alloc, x) for x in mls]
        plan = SumcheckPlan(hal, n_vars, d, alloc.alloc(2 << (n_vars - 1)), [(0, 1)], [claim], stream[0], stream[1:])
        before = counters(hal)
        plan.run()
        delta = moved(before, counters(hal))
        assert (plan.round_coeffs(), plan.final_evals()) == tuple(want), "the transcript is not the oracle's"
        return delta, hal.arm_counters()["ht_max"]


def seq_mlecheck(oracle, n_vars):
    """one compiled MLE-check, the literal trait-call sequence (BN_MLECHECK=eager: a * b * eq every round, fold of a and b, the
    table folded by adding its halves)"""
    import binius_amd
    from binius_amd._host import MlecheckPlan
    from test_gpu_mlecheck_shadow import _instance

    mls, eq_ch, half, sums, bc, ch = _instance(oracle, n_vars, 2, [(0, 1)], 0xF0700000)
    want = oracle.bivariate_mlecheck_prove([x.copy() for x in mls], n_vars, half.copy(), eq_ch, [(0, 1)], sums, bc, ch)
    with env(BN_MLECHECK="eager"):
        with binius_amd.Context(0, 10 << n_vars) as hal:
            alloc = hal.dev_alloc()
            d = [upload(hal, alloc, x) for x in mls]
            eq_dev = upload(hal, alloc, half)
            plan = MlecheckPlan(hal, n_vars, d, eq_dev, eq_ch, alloc.alloc(3 << (n_vars - 1)), [(0, 1)], sums, bc, ch)
            before = counters(hal)
            plan.run()
            delta = moved(before, counters(hal))
            assert plan.last_mode() == 0
            assert (plan.round_coeffs(), plan.final_evals()) == tuple(want), "the transcript is not the oracle's"
            return delta, hal.arm_counters()["ht_max"]


def seq_interleave(oracle, n_vars):
    """two provers take turns on one context: each one's fold arrives while the other's is deferred"""
    import binius_amd
    from binius_amd.sumcheck import bivariate_product_expr, calculate_round_evals

    with binius_amd.Context(0, 8 << n_vars) as hal:
        alloc = hal.dev_alloc()
        inst = []
        for k in range(2):
            mls = [oracle.random_b128(0xF0800000 + 16 * k + j, 1 << n_vars) for j in range(2)]
            inst.append({"cur": [x.copy() for x in mls], "d": [upload(hal, alloc, x) for x in mls]})
        zs = oracle.random_scalars(0xF08D, 2 * n_vars)
        expr = bivariate_product_expr(hal, 0, 1)
        before = counters(hal)
        for r in range(n_vars):
            for k, it in enumerate(inst):
                if r > 0:
                    z = zs[2 * (r - 1) + k]
                    halves = [x.split_half() for x in it["d"]]
                    hal.extrapolate_line_batch([lo for lo, _ in halves], [hi for _, hi in halves], z)
                    nxt = []
                    for x in it["cur"]:
                        f = x[: len(x) // 2].copy()
                        assert oracle.extrapolate_line(f, x[len(x) // 2 :].copy(), z) == 0
                        nxt.append(f)
                    it["cur"], it["d"] = nxt, [lo for lo, _ in halves]
                nv = n_vars - r
                got = calculate_round_evals(hal, nv, [1], it["d"], [expr])
                rc, want = oracle.round_evals(it["cur"], nv, [(0, 1)], 1)
                assert rc == 0 and got == want, "instance %d round %d" % (k, r)
        for it in inst:
            for dd, x in zip(it["d"], it["cur"]):
                assert np.array_equal(hal.copy_d2h(dd), x)
        return moved(before, counters(hal)), hal.arm_counters()["ht_max"]


SEQUENCES = {
    "sumcheck-6": (seq_sumcheck, 6),
    "sumcheck-9": (seq_sumcheck, 9),
    "sumcheck-12": (seq_sumcheck, 12),
    "sumcheck-13": (seq_sumcheck, 13),
    "mlecheck-8": (seq_mlecheck, 8),
    "interleave-8": (seq_interleave, 8),
}
HT_MAX = 4096  # the host tail's hand-over size on the host the deltas were recorded on (VPCLMULQDQ); counters absent from a row did not move
ROUTES = {
    "sumcheck-6": {"arm.two_round": 1, "arm.ht_started": 1, "arm.ht_rounds": 5, "arm.ht_flushed": 1},
    "sumcheck-9": {"arm.two_round": 1, "arm.ht_started": 1, "arm.ht_rounds": 7, "arm.ht_flushed": 1},
    "sumcheck-12": {"arm.two_round": 1, "arm.ht_started": 1, "arm.ht_rounds": 11, "arm.ht_flushed": 1},
    "sumcheck-13": {"arm.two_round": 1, "arm.ht_started": 1, "arm.ht_rounds": 11, "arm.ht_flushed": 1},
    "mlecheck-8": {},  # (below the shadow's smallest table: the three-factor kernel answers every round, every fold is a plain deferred one)
    "interleave-8": {"arm.two_round": 14, "arm.ht_started": 14},  # (each prover's fold ends the other's host tail before it has folded)
}


def route_delta(oracle, name):
    fn, n_vars = SEQUENCES[name]
    delta, ht_max = fn(oracle, n_vars)
    keep = {k: v for k, v in delta.items() if k.startswith("group.") or k[len("arm.") :] in ARM_KEYS}
    return keep, ht_max


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_fixed_sequences_take_the_recorded_routes(oracle, name):
    got, ht_max = route_delta(oracle, name)
    print(name, got)
    if ht_max != HT_MAX:
        pytest.skip("the deltas were recorded where the host tail takes over 2^12 elements; here ht_max = %d" % ht_max)
    assert got == ROUTES[name], (name, got)
