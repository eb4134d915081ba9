"""GPU parity of the GKR grand-product argument: bn_product_tree_layers (binius_amd/csrc/kernels_prodtree.hip + abi_prodtree.cpp;
reference: gkr_gpa/gkr_gpa.rs:38-90) against tests/gkr_gpa_ref.py product_layers, and bnh_gkr_gpa_prove (binius_amd/host/gkr_gpa.hpp;
reference: gkr_gpa/prove.rs:33-296) against gpa_prove and the verifier checker of the same file (pinned by
tests/test_gkr_gpa_oracle.py).  Everything is bit-exact and nothing is compared with the device's own output.  One context per
module; the oracle's layers are computed once per (seed, n_vars, length)."""
import functools

import numpy as np
import pytest

import adversarial as A
import gkr_gpa_ref as R

pytestmark = pytest.mark.gpu

CANARY_ROW = np.array([A.CANARY & A.M64, A.CANARY >> 64], dtype=np.uint64)
ARENA_ELEMS = (1 << 25) + (1 << 23)


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, ARENA_ELEMS)
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def random_case(seed, n_vars, length):
    """(input or None, layers) of SplitMix64 data."""
    import oracle

    vals = oracle.random_b128(seed, length) if length else None
    return vals, R.product_layers(vals, n_vars)


def run_trees(hal, cases):
    """cases: [(n_vars, input array or None, expected layers)].  One call of the op for all of them; every layer of every tree,
    the product, arena[0] (a sentinel) and the input (unchanged) are checked."""
    import oracle

    alloc = hal.dev_alloc()
    ins, arenas = [], []
    for n, vals, _ in cases:
        if vals is None or vals.shape[0] == 0:
            ins.append(None)
        else:
            d = alloc.alloc(vals.shape[0])
            hal.copy_h2d(vals, d)
            ins.append(d)
        a = alloc.alloc(1 << n)
        hal.fill(a, A.CANARY)
        arenas.append(a)
    products = hal.product_tree_layers([n for n, _, _ in cases], ins, arenas)
    for t, (n, vals, layers) in enumerate(cases):
        what = "tree %d (n_vars %d, %d elements)" % (t, n, 0 if vals is None else vals.shape[0])
        assert products[t] == oracle.arr_to_ints(layers[0])[0], "%s: product differs" % what
        got = hal.copy_d2h(arenas[t])
        assert np.array_equal(got[0], CANARY_ROW), "%s: arena[0] was written" % what
        for j in range(n):
            assert np.array_equal(got[1 << j : 2 << j], layers[j]), "%s: layer %d differs" % (what, j)
        if ins[t] is not None:
            assert np.array_equal(hal.copy_d2h(ins[t]), vals), "%s: the input was modified" % what
    return products


def trunc_lengths(n):
    full = 1 << n
    odd = (full * 3) // 5 | 1  # (no multiple of the wave batch of 224, which is even)
    return sorted({0, 1, full - 1, min(full, odd), full >> 1, min(full, (full >> 1) + 1)})


@pytest.mark.parametrize("n_vars", list(range(18)))
def test_single_tree_full_input(hal, n_vars):
    vals, layers = random_case(0x9A000 + n_vars, n_vars, 1 << n_vars)
    run_trees(hal, [(n_vars, vals, layers)])


@pytest.mark.parametrize("n_vars", [0, 1, 2, 5, 8, 9, 12, 15, 16, 17, 18, 20])  # (20: the two-batch form of the big kernel)
def test_truncated_inputs(hal, n_vars):
    for length in trunc_lengths(n_vars):
        vals, layers = random_case(0x9B000 + n_vars, n_vars, length)
        run_trees(hal, [(n_vars, vals, layers)])


def test_batch_of_mixed_trees_in_one_call(hal):
    cases = []
    for t in range(48):
        n = t % 15
        lens = trunc_lengths(n)
        length = (1 << n) if t % 3 == 0 else lens[t % len(lens)]
        vals, layers = random_case(0x9C000 + t, n, length)
        cases.append((n, vals, layers))
    # two trees above the small form's 2^15 in the same call, one of them truncated
    for n, length in ((16, 1 << 16), (17, 70001)):
        vals, layers = random_case(0x9C800 + n, n, length)
        cases.append((n, vals, layers))
    run_trees(hal, cases)


@pytest.mark.parametrize("kind", ["zero", "sub0", "sub3", "sub5", "sparse", "dense", "nib8", "nib7", "limb2"])
def test_adversarial_operands(hal, kind):
    cases = []
    for n in (10, 16):
        vals = A.operands(kind, 0x9D000 + n, 1 << n)
        cases.append((n, vals, R.product_layers(vals, n)))
    ones = np.zeros((1 << 16, 2), dtype=np.uint64)
    ones[:, 0] = 1
    cases.append((16, ones, R.product_layers(ones, 16)))
    run_trees(hal, cases)


@pytest.mark.parametrize("n_vars,pos", [(10, 777), (16, 40001), (17, 131071)])
def test_a_single_zero_zeroes_exactly_its_ancestors(hal, n_vars, pos):
    import oracle

    vals = oracle.random_b128(0x9E000 + n_vars, 1 << n_vars).copy()
    assert ((vals[:, 0] | vals[:, 1]) != 0).all()
    vals[pos] = 0
    layers = R.product_layers(vals, n_vars)
    for j in range(n_vars + 1):  # (the expectation itself: in a field only the ancestors vanish)
        zero = np.flatnonzero((layers[j][:, 0] | layers[j][:, 1]) == 0)
        assert zero.tolist() == [pos % (1 << j)]
    run_trees(hal, [(n_vars, vals, layers)])


@pytest.mark.parametrize("n_vars", [22, 24])
def test_large_tree_layer_by_layer(hal, n_vars):
    import oracle

    vals = oracle.random_b128(0x9F000 + n_vars, 1 << n_vars)
    run_trees(hal, [(n_vars, vals, R.product_layers(vals, n_vars))])


def test_validation_errors_leave_the_context_usable(hal):
    from binius_amd._ffi import BnError, DevSlice

    alloc = hal.dev_alloc()
    inp, arena = alloc.alloc(16), alloc.alloc(8)
    with pytest.raises(BnError) as e:
        hal.product_tree_layers([3], [inp], [arena])  # 16 elements for 2^3
    assert e.value.kind == "InputValidation"
    with pytest.raises(BnError) as e:
        hal.product_tree_layers([3], [inp.slice(0, 8)], [None])
    assert e.value.kind == "InputValidation"
    with pytest.raises(BnError) as e:
        hal.product_tree_layers([29], [inp], [DevSlice(arena.ptr, 1 << 29)])
    assert e.value.kind == "InputValidation"
    with pytest.raises(BnError) as e:
        hal.product_tree_layers([3], [inp.slice(4, 12)], [inp.slice(0, 8)])  # the arena overlaps its input
    assert e.value.kind == "InputValidation"
    vals, layers = random_case(0x9A000 + 7, 7, 1 << 7)
    run_trees(hal, [(7, vals, layers)])


# ---------------------------------------------------------------------------------------------- the prover
def transcript(oracle, n_vars, seed):
    m = max(n_vars)
    bc, gc = oracle.random_scalars(seed, max(1, m))[:m], oracle.random_scalars(seed + 1, max(1, m))[:m]
    flat = oracle.random_scalars(seed + 2, m * (m - 1) // 2 + 1)
    sc, off = [], 0
    for j in range(m):
        sc.append(flat[off : off + j])
        off += j
    return bc, sc, gc


def run_prover(hal, shapes, inputs, bc, sc, gc):
    """The device prover over freshly uploaded inputs; returns its output in gpa_prove's shape.  The inputs must come back unchanged."""
    from binius_amd._host import GkrGpaPlan

    alloc = hal.dev_alloc()
    n_vars = [n for n, _ in shapes]
    ins, arenas = [], []
    for (n, _), vals in zip(shapes, inputs):
        if vals is None:
            ins.append(None)
        else:
            d = alloc.alloc(vals.shape[0])
            hal.copy_h2d(vals, d)
            ins.append(d)
        arenas.append(alloc.alloc(1 << n))
    scratch = alloc.alloc(GkrGpaPlan.scratch_elems(n_vars))
    plan = GkrGpaPlan(hal, n_vars, ins, arenas, scratch, bc, sc, gc)
    plan.run()
    for d, vals in zip(ins, inputs):
        if d is not None:
            assert np.array_equal(hal.copy_d2h(d), vals), "the prover wrote to an input"
    return plan.output()


def assert_same_proof(got, want):
    for key in ("products", "round_proofs", "layer_evals", "final_points", "final_evals"):
        assert got[key] == want[key], "%s differ from the CPU restatement" % key


def test_prover_mixed_batch_vs_restatement(oracle, hal):
    shapes = [(5, 32), (3, 5), (7, 100), (0, 1), (5, 0), (1, 2), (7, 128)]
    inputs = [oracle.random_b128(0xA1000 + 17 * t, ln) if ln else None for t, (_, ln) in enumerate(shapes)]
    n_vars = [n for n, _ in shapes]
    bc, sc, gc = transcript(oracle, n_vars, 0xA1800)
    want = R.gpa_prove(inputs, n_vars, bc, sc, gc)
    got = run_prover(hal, shapes, inputs, bc, sc, gc)
    assert_same_proof(got, want)
    R.gpa_verify(n_vars, got["products"], got, bc, sc, gc)


@pytest.mark.parametrize("n_vars", [1, 2, 6, 11, 14])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_prover_equal_sized_trees_vs_restatement(oracle, hal, k, n_vars):
    shapes = [(n_vars, 1 << n_vars)] * k
    inputs = [oracle.random_b128(0xA2000 + 64 * n_vars + t, 1 << n_vars) for t in range(k)]
    bc, sc, gc = transcript(oracle, [n_vars] * k, 0xA2800 + n_vars)
    want = R.gpa_prove(inputs, [n_vars] * k, bc, sc, gc)
    got = run_prover(hal, shapes, inputs, bc, sc, gc)
    assert_same_proof(got, want)


def test_prover_at_2_20_passes_the_verifier(oracle, hal):
    """k = 4 trees of 2^20 (one truncated): no CPU prover at this size -- the verifier's equations and the final claims against
    mle_evaluate of the ONE-padded inputs, the products against the oracle's layers."""
    n, k = 20, 4
    lens = [1 << n, 1 << n, (1 << n) - 12345, 1 << n]
    shapes = [(n, ln) for ln in lens]
    inputs = [oracle.random_b128(0xA3000 + t, ln) for t, ln in enumerate(lens)]
    bc, sc, gc = transcript(oracle, [n] * k, 0xA3800)
    got = run_prover(hal, shapes, inputs, bc, sc, gc)
    points, evals = R.gpa_verify([n] * k, got["products"], got, bc, sc, gc)
    assert points == got["final_points"] and evals == got["final_evals"]
    for t in range(k):
        padded = R.pad_ones(inputs[t], n)
        assert evals[t] == oracle.mle_evaluate(padded, n, points[t]), "claim %d: the final claim is not the input's evaluation" % t
    assert got["products"][2] == oracle.arr_to_ints(R.product_layers(inputs[2], n)[0])[0]


def test_prover_validation_errors(oracle, hal):
    from binius_amd._ffi import BnError
    from binius_amd._host import GkrGpaPlan

    alloc = hal.dev_alloc()
    inp, arena, scratch = alloc.alloc(8), alloc.alloc(8), alloc.alloc(4)
    bc, sc, gc = transcript(oracle, [3], 0xA4000)
    with pytest.raises(BnError) as e:
        GkrGpaPlan(hal, [3], [inp], [arena], scratch, bc, sc, gc).run()  # scratch needs 8 + 4
    assert e.value.kind == "InputValidation"
    with pytest.raises(BnError) as e:
        GkrGpaPlan(hal, [3], [inp], [None], alloc.alloc(12), bc, sc, gc).run()
    assert e.value.kind == "InputValidation"


def test_pad_with_ones(oracle, hal):
    """bn_pad_with_ones: several arrays in one launch; the sources unchanged, nothing written past a destination."""
    alloc = hal.dev_alloc()
    shapes = [(0, 0), (0, 1), (4, 5), (9, 300), (9, 512), (13, 1), (13, 8191)]
    srcs, dsts, vals = [], [], []
    for t, (n, ln) in enumerate(shapes):
        v = oracle.random_b128(0xA5000 + t, ln) if ln else None
        d = None
        if ln:
            d = alloc.alloc(ln)
            hal.copy_h2d(v, d)
        block = alloc.alloc((1 << n) + 1)
        hal.fill(block, A.CANARY)
        srcs.append(d), dsts.append(block), vals.append(v)
    hal.pad_with_ones([n for n, _ in shapes], srcs, [b.slice(0, b.len - 1) for b in dsts])
    for (n, ln), d, block, v in zip(shapes, srcs, dsts, vals):
        got = hal.copy_d2h(block)
        assert np.array_equal(got[: 1 << n], R.pad_ones(v, n)), "padded copy differs (2^%d from %d)" % (n, ln)
        assert np.array_equal(got[1 << n], CANARY_ROW), "written past the destination"
        if d is not None:
            assert np.array_equal(hal.copy_d2h(d), v)
