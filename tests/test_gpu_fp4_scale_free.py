"""The FP4 matrix instruction without block scales (csrc/gram_fp4.hpp BN_FP4_MFMA: v_mfma_f32_32x32x64_f8f6f4 cbsz:4 blgp:4 in
place of the scaled form with scales of 2^0): every kernel that issues it, bit for bit against the oracle, on three operand fills.

  random    SplitMix64, what every other parity test uses
  ones      every element all ones: every accumulator entry counts every point of its workgroup (rows of its chunk), the largest
            counts the f32 accumulators meet at these sizes
  one_bit   exactly one pseudo-random bit set per element (adversarial.operands "sparse"): almost every product term is zero

Cases (dispatch on 256 compute units):
  * a sumcheck transcript at n_vars = 21: round 0 (2^20 points) on k_roundeval_fp4_ws, the claim's inner product on its split
    form, the fused launches from 2^21 down to 2^19 elements on k_foldeval_mfma_fp4;
  * inner_product of two 2^20-element vectors (2^19 points per half: below the FP4 switch, the int8 split kernel) and of two
    2^21-element vectors (2^20 points per half: k_roundeval_fp4_ws, split form);
  * fold_right of 2^20 elements with 16 vector entries at levels 5, 6, 7 (rows of 512, 1024, 2048 bits): kernels_linmap.hip;
  * in a fresh process with BN_FP4_MIN_LOG2=0 (the switch is read once): the transcript at n_vars = 12, and what reaches the
    three-workgroup kernel k_roundeval_fp4 on such a device -- a matrix-core round evaluation needs one tile of 256 points per compute
    unit, so at n_vars = 12 the 9-lane kernels answer whatever the switch says --: the transcript at n_vars = 18 (round 0: 2^17
    points), inner_product of two 2^20-element vectors and of two vectors of 2 (2^17 + 777) elements (the ragged last tile).

The oracle results are computed once per fill and size and shared (_REF)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adversarial as A
from test_gpu_group import _threads, oracle_single

pytestmark = pytest.mark.gpu

FILLS = ("random", "ones", "one_bit")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def ref(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def fill(kind, seed, n):
    """(n, 2) uint64 array of BinaryField128b elements of the fill `kind`."""
    if kind == "ones":
        return np.full((n, 2), np.uint64((1 << 64) - 1), dtype=np.uint64)
    return A.operands("sparse" if kind == "one_bit" else "random", seed, n)


def fast_ip(oracle, a, b):
    got = oracle.fast_inner_product(np.ascontiguousarray(a), np.ascontiguousarray(b), _threads())
    if got is None:  # a host without PCLMULQDQ: the scalar oracle
        rc, got = oracle.inner_product(np.ascontiguousarray(a), 7, np.ascontiguousarray(b))
        assert rc == 0
    return got


def upload(hal, alloc, arr):
    d = alloc.alloc(arr.shape[0])
    hal.copy_h2d(arr, d)
    return d


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, (1 << 23) + (1 << 21))
    yield ctx
    ctx.close()
    _REF.clear()


def sumcheck_case(hal, oracle, kind, n_vars):
    """One product claim over two multilinears of the fill: the claim from the device inner product, then the whole transcript."""
    from binius_amd._host import SumcheckPlan

    mls = ref(("mls", kind, n_vars), lambda: [fill(kind, 0x5CF40000 + j, 1 << n_vars) for j in range(2)])
    alloc = hal.dev_alloc()
    d = [upload(hal, alloc, x) for x in mls]
    scratch = alloc.alloc(2 << (n_vars - 1))
    claim = ref(("claim", kind, n_vars), lambda: fast_ip(oracle, mls[0], mls[1]))
    assert hal.inner_product(d[0], 7, d[1]) == claim, (kind, n_vars)
    stream = oracle.random_scalars(0xC4A1 + n_vars, n_vars + 1)
    bc, ch = stream[0], stream[1:]
    want = ref(("sumcheck", kind, n_vars), lambda: oracle_single(oracle, mls, n_vars, [(0, 1)], [claim], bc, ch))
    plan = SumcheckPlan(hal, n_vars, d, scratch, [(0, 1)], [claim], bc, ch)
    plan.run()
    got_coeffs, got_finals = plan.round_coeffs(), plan.final_evals()
    for r in range(n_vars):
        assert list(got_coeffs[r]) == list(want[0][r]), "round %d differs from the oracle (%s, n = %d)" % (r, kind, n_vars)
    assert list(got_finals) == list(want[1]), (kind, n_vars)
    for j in range(2):
        assert np.array_equal(hal.copy_d2h(d[j]), mls[j])  # the inputs are never modified


@pytest.mark.parametrize("kind", FILLS)
def test_sumcheck_transcript_n21(hal, oracle, kind):
    """n_vars = 21 is the smallest size at which round 0 takes the wave-specialised kernel (2^20 points, whole tiles, >= 2 per
    compute unit) and the first fused launch the FP4 fused kernel."""
    sumcheck_case(hal, oracle, kind, 21)
    g = hal.fp4_last_grids()
    if hal.fold_counters()["n_cu"] == 256:
        assert g["re_ws"] == 1 and g["re_grid"] * g["re_tiles"] >= (1 << 20) // 256, g
        assert g["fe_grid"] > 0 and g["fe_grid"] * g["fe_tiles"] >= 512, g


@pytest.mark.parametrize("log_n", [20, 21])
@pytest.mark.parametrize("kind", FILLS)
def test_inner_product_split_form(hal, oracle, kind, log_n):
    """F x F: the two halves of the vectors as two independent products of one launch.  2^20 elements: 2^19 points per half, the
    int8 split kernel under the default switch; 2^21: k_roundeval_fp4_ws."""
    alloc = hal.dev_alloc()
    n_b = 1 << log_n
    a, b = fill(kind, 0x1F40 + log_n, n_b), fill(kind, 0x1F80 + log_n, n_b)
    c0 = hal.inner_product_counters()
    got = hal.inner_product(upload(hal, alloc, a), 7, upload(hal, alloc, b))
    c1 = hal.inner_product_counters()
    assert got == fast_ip(oracle, a, b), (kind, log_n)
    assert c1["mfma_split"] == c0["mfma_split"] + 1, (c0, c1)
    if log_n == 21 and hal.fold_counters()["n_cu"] == 256:
        g = hal.fp4_last_grids()
        assert g["re_ws"] == 1 and g["re_grid"] * g["re_tiles"] >= (n_b // 2) // 256, g


@pytest.mark.parametrize("level", [5, 6, 7])
@pytest.mark.parametrize("kind", FILLS)
def test_fold_right_matrix_core_map(hal, oracle, kind, level):
    """fold_right of 2^20 level-7 elements' worth of matrix with 16 vector entries (test_gpu_at_size's shape): rows of 512, 1024 and
    2048 bits on the matrix cores, the matrix being the masked operand."""
    alloc = hal.dev_alloc()
    log_q = 4
    mat = fill(kind, 0x2F40 + level, (1 << 20) >> (7 - level))
    vec = oracle.random_b128(0x2F80, 1 << log_q)
    out_len = 1 << (20 - log_q)
    dm, dv, do = upload(hal, alloc, mat), upload(hal, alloc, vec), alloc.alloc(out_len)
    exp = oracle.arr(out_len)
    c0 = hal.fold_counters()
    hal.fold_right(dm, level, dv, do)
    c1 = hal.fold_counters()
    assert oracle.fold_right(mat, level, vec, exp) == 0
    assert c1["right_mfma"] == c0["right_mfma"] + 1, (c0, c1)
    assert np.array_equal(hal.copy_d2h(do), exp), (kind, level)
    assert np.array_equal(hal.copy_d2h(dm), mat)


def small_shapes_inner():
    """The body of test_small_shapes_with_the_fp4_switch_at_zero, in its own process."""
    import binius_amd
    import oracle

    assert os.environ.get("BN_FP4_MIN_LOG2") == "0"
    oracle.build()
    with binius_amd.Context(0, 1 << 22) as hal:
        n_cu = hal.fold_counters()["n_cu"]
        for kind in FILLS:
            sumcheck_case(hal, oracle, kind, 12)
            print("n_vars = 12, %s: %r" % (kind, hal.fp4_last_grids()))
            sumcheck_case(hal, oracle, kind, 18)
            g = hal.fp4_last_grids()
            print("n_vars = 18, %s: %r" % (kind, g))
            if n_cu <= 512:  # round 0: 2^17 points = 512 tiles, at least one per compute unit: the three-workgroup FP4 kernel
                assert g["re_ws"] == 0 and g["re_grid"] * g["re_tiles"] >= 512, g
            for n_b in (1 << 20, 2 * (131072 + 777)):
                alloc = hal.dev_alloc()
                a, b = fill(kind, 0x3F40, n_b), fill(kind, 0x3F80, n_b)
                got = hal.inner_product(upload(hal, alloc, a), 7, upload(hal, alloc, b))
                assert got == fast_ip(oracle, a, b), (kind, n_b)
                g = hal.fp4_last_grids()
                print("inner_product of 2 x %d, %s: %r" % (n_b, kind, g))
                if n_cu <= 512:
                    assert g["re_ws"] == 0 and g["re_grid"] * g["re_tiles"] >= (n_b // 2 + 255) // 256, g
    print("small shapes ok")


def test_small_shapes_with_the_fp4_switch_at_zero():
    """BN_FP4_MIN_LOG2=0 sends every matrix-core round evaluation to the FP4 kernels (as test_fp4_matrix_path_on_the_small_shapes
    does): below 2^20 points, and for ragged sizes, that is the three-workgroup kernel k_roundeval_fp4 with its zero-padded last
    tile.  A fresh process, because the switch is read once."""
    env = dict(os.environ, BN_FP4_MIN_LOG2="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_fp4_scale_free as t; t.small_shapes_inner()" % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "small shapes ok" in p.stdout
