"""GPU parity of the additive NTT for every (element, twiddle) field pair the ABI accepts, on the two kernel families that
tests/test_gpu_ntt.py hardly reaches: the LDS-tiled kernel (kernels_ntt_tiled.hip: k_ntt_tiled<uint16_t / uint32_t / uint64_t / uint4>,
mulw_tab<3 / 4 / 5>) and the per-layer kernel (kernels_ntt.hip, the only path for B8 elements, B64 twiddles and transforms below 2^12
elements).  The families are reached by shape -- no switch reroutes a transform in the normal build -- and `Context.ntt_counters()`
(bn_ntt_counters) says which one served a call.

Every case: the forward output is oracle.ntt_forward's; on independent random data the device's inverse is oracle.ntt_inverse's; the
inverse of the forward output is the input.  Nothing is compared with the device's own output.  The data sits at an odd multiple of 16
bytes between canary frames (tests/adversarial.py), which must stay intact.  The oracle is pinned for these pairs against the
definitions by tests/test_oracle_ntt_pairs.py.

Shapes are (log_domain, log_x, log_y, log_z, coset, coset_bits, skip_rounds); index = x | y << log_x | z << (log_x + log_y).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import adversarial as A

pytestmark = pytest.mark.gpu

FAMILIES = ("bs", "tiled", "layer")
# the largest case: 2^26 B128 elements between two frames
ARENA = (1 << 26) + 2 * A.FRAME + 64


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, ARENA)
    yield ctx
    ctx.close()


def rand_bytes(oracle, seed, nbytes):
    assert nbytes % 16 == 0
    return oracle.splitmix_words(seed, nbytes // 8).view(np.uint8)


def as16(b):
    """A byte array as the (n, 2) uint64 array of 16-byte units that place() and the copies take."""
    return np.ascontiguousarray(b).view(np.uint64).reshape(-1, 2)


def s_evals(oracle, tw_level, log_domain):
    import binius_amd

    s = binius_amd.ntt_s_evals(tw_level, log_domain)
    assert np.array_equal(s, oracle.ntt_s_evals(tw_level, log_domain))
    return s


def oracle_pair(oracle, el, tw, s, shape, x, y):
    """(oracle.ntt_forward of x, oracle.ntt_inverse of y): the two references of a case, side by side for the large ones."""
    ld, lx, ly, lz, coset, cb, skip = shape

    def fwd():
        w = x.copy()
        assert oracle.ntt_forward(w, el, tw, s, ld, lx, ly, lz, coset, cb, skip) == 0
        return w

    def inv():
        w = y.copy()
        assert oracle.ntt_inverse(w, el, tw, s, ld, lx, ly, lz, coset, cb, skip) == 0
        return w

    if x.nbytes < (1 << 20):
        return fwd(), inv()
    with ThreadPoolExecutor(2) as ex:
        f, i = ex.submit(fwd), ex.submit(inv)
        return f.result(), i.result()


def moved(before, after):
    return {k: after[k] - before[k] for k in FAMILIES}


def only(family, n):
    return {k: (n if k == family else 0) for k in FAMILIES}


def device_case(hal, family, el, tw, s, shape, x, y, want_f, want_i):
    """x -> forward (= want_f) -> inverse (= x); y -> inverse (= want_i).  All arrays are bytes.  The counters say `family` ran."""
    ld, lx, ly, lz, coset, cb, skip = shape
    assert x.nbytes == y.nbytes == (1 << (lx + ly + lz + el - 3))
    alloc = hal.dev_alloc()
    dx, chk_x = A.place(hal, alloc, as16(x), 1)
    c0 = hal.ntt_counters()
    hal.ntt_forward(dx.ptr, el, tw, s, ld, lx, ly, lz, coset, cb, skip)
    c1 = hal.ntt_counters()
    chk_x(as16(want_f))
    hal.ntt_inverse(dx.ptr, el, tw, s, ld, lx, ly, lz, coset, cb, skip)
    c2 = hal.ntt_counters()
    chk_x(as16(x))
    alloc = hal.dev_alloc()  # (the first block is done with: the largest case fits the arena once)
    dy, chk_y = A.place(hal, alloc, as16(y), 3)
    hal.ntt_inverse(dy.ptr, el, tw, s, ld, lx, ly, lz, coset, cb, skip)
    c3 = hal.ntt_counters()
    chk_y(as16(want_i))
    assert moved(c0, c1) == only(family, 1), "forward: %s ran, not %s" % (moved(c0, c1), family)
    assert moved(c1, c2) == only(family, 1), "inverse: %s ran, not %s" % (moved(c1, c2), family)
    assert moved(c2, c3) == only(family, 1), "inverse: %s ran, not %s" % (moved(c2, c3), family)


def run_case(hal, oracle, family, el, tw, shape, seed=0x9A1):
    ld, lx, ly, lz, coset, cb, skip = shape
    nbytes = 1 << (lx + ly + lz + el - 3)
    s = s_evals(oracle, tw, ld)
    x = rand_bytes(oracle, seed + 2 * (16 * el + tw), nbytes)
    y = rand_bytes(oracle, seed + 2 * (16 * el + tw) + 1, nbytes)
    want_f, want_i = oracle_pair(oracle, el, tw, s, shape, x, y)
    assert not np.array_equal(want_f, x)
    device_case(hal, family, el, tw, s, shape, x, y, want_f, want_i)
    return want_f


# ---------------------------------------------------------------------------------- (a) the tiled kernel
TILED_PAIRS = [(4, 3), (4, 4), (5, 3), (5, 4), (5, 5), (6, 3), (6, 4), (6, 5), (7, 3), (7, 4), (7, 5)]

TW3_SHAPES = [
    (8, 4, 8, 0, 0, 0, 0),  # a 6-layer pass and a 2-layer pass
    (8, 0, 7, 5, 1, 1, 0),  # the run bits above the butterfly bits spill from y into z; a 6-layer pass plus a 1-layer pass
    (8, 3, 8, 2, 0, 0, 2),  # exactly 6 layers
    (8, 6, 5, 1, 5, 3, 0),
    (8, 2, 6, 4, 3, 2, 5),  # one layer left
]
TW4_SHAPES = [
    (13, 0, 13, 0, 0, 0, 0),  # three passes
    (16, 0, 12, 0, 9, 4, 0),  # two full passes, coset
    (16, 1, 11, 1, 1, 1, 3),  # base_layer = 4
    (10, 5, 7, 0, 0, 0, 0),  # seven layers, batch in x only
]
TW4_FULL = (16, 0, 16, 0, 0, 0, 0)  # the whole B16 domain
TW5_SHAPES = TW4_SHAPES + [
    (20, 0, 13, 0, 37, 7, 0),  # base_layer = 0, wide coset
    (24, 0, 7, 5, 3, 2, 0),  # z-spill with base_layer = 15
]


def tiled_cases():
    out = []
    for el, tw in TILED_PAIRS:
        shapes = {3: TW3_SHAPES, 4: TW4_SHAPES, 5: TW5_SHAPES}[tw]
        out += [(el, tw, sh) for sh in shapes]
        if tw == 4 and el in (4, 6):
            out.append((el, tw, TW4_FULL))
    return out


def case_id(c):
    el, tw, sh = c
    return "B%d/B%d-%s" % (1 << el, 1 << tw, "_".join(str(v) for v in sh))


@pytest.mark.parametrize("case", tiled_cases(), ids=case_id)
def test_tiled_pairs(hal, oracle, case):
    el, tw, shape = case
    ld, lx, ly, lz, coset, cb, skip = shape
    assert lx + ly + lz >= 12 and ld <= (1 << tw) and not (tw == 5 and ly >= 14)
    run_case(hal, oracle, "tiled", el, tw, shape)


def test_tiled_case_list_is_complete():
    cases = tiled_cases()
    assert sorted({(el, tw) for el, tw, _ in cases}) == sorted((el, tw) for el in (4, 5, 6, 7) for tw in range(3, min(el, 5) + 1))
    assert len(TILED_PAIRS) == 11 and len(cases) == 4 * 5 + 4 * 4 + 2 + 3 * 6


def patterns(oracle, el, nbytes):
    """An impulse at the last index (its image exposes each layer's twiddles), all bytes 0xFF, zero."""
    eb = 1 << (el - 3)
    imp = np.zeros(nbytes, dtype=np.uint8)
    imp[-eb:] = rand_bytes(oracle, 0x1337 + el, 16)[:eb] | 1  # every byte of the element nonzero
    return {"impulse": imp, "ones": np.full(nbytes, 0xFF, dtype=np.uint8), "zero": np.zeros(nbytes, dtype=np.uint8)}


PATTERN_CASES = [
    ("tiled", 4, 4, (16, 1, 11, 1, 1, 1, 3)),
    ("tiled", 5, 3, (8, 0, 7, 5, 1, 1, 0)),
    ("tiled", 6, 5, (20, 0, 13, 0, 37, 7, 0)),
    ("tiled", 7, 4, (13, 0, 13, 0, 0, 0, 0)),
    ("layer", 3, 3, (8, 1, 6, 1, 1, 2, 0)),
]


@pytest.mark.parametrize("kind", ["impulse", "ones", "zero"])
@pytest.mark.parametrize("family,el,tw,shape", PATTERN_CASES, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_patterned_inputs(hal, oracle, family, el, tw, shape, kind):
    ld, lx, ly, lz, coset, cb, skip = shape
    s = s_evals(oracle, tw, ld)
    x = patterns(oracle, el, 1 << (lx + ly + lz + el - 3))[kind]
    want_f, want_i = oracle_pair(oracle, el, tw, s, shape, x, x)
    if kind == "zero":
        assert not want_f.any() and not want_i.any()
    else:
        assert not np.array_equal(want_f, x) and not np.array_equal(want_i, x)
    device_case(hal, family, el, tw, s, shape, x, x, want_f, want_i)


# ---------------------------------------------------------------------------------- (b) the per-layer kernel
LAYER_PAIRS = [(3, 3), (4, 3), (4, 4), (5, 3), (5, 4), (5, 5), (6, 3), (6, 4), (6, 5), (6, 6), (7, 3), (7, 4), (7, 5), (7, 6)]


def layer_domain(tw):
    return min(1 << tw, 9)  # 8 for B8 twiddles


@pytest.mark.parametrize("el,tw", LAYER_PAIRS, ids=lambda v: str(v))
def test_per_layer_pairs_batched_coset(hal, oracle, el, tw):
    run_case(hal, oracle, "layer", el, tw, (layer_domain(tw), 1, 6, 1, 1, 2, 0))


@pytest.mark.parametrize("el,tw", LAYER_PAIRS, ids=lambda v: str(v))
def test_per_layer_pairs_skip(hal, oracle, el, tw):
    run_case(hal, oracle, "layer", el, tw, (layer_domain(tw), 0, 5, 0, 0, 0, 2))


def test_per_layer_case_list_is_complete():
    assert sorted(LAYER_PAIRS) == sorted((el, tw) for el in range(3, 8) for tw in range(3, min(el, 6) + 1)) and len(LAYER_PAIRS) == 14


@pytest.mark.parametrize(
    "case",
    [
        (3, 3, (8, 7, 8, 7, 0, 0, 0)),  # 2^22 one-byte elements = 2^21 butterflies: the grid (at most 4096 x 256) strides twice
        (3, 3, (8, 0, 6, 0, 1, 2, 0)),
        (6, 6, (20, 0, 20, 0, 0, 0, 0)),
        (7, 6, (24, 1, 17, 0, 3, 2, 1)),
        (6, 6, (40, 0, 12, 0, (1 << 24) + 0x5A5A5, 25, 0)),  # twiddle indices wider than 32 bits
    ],
    ids=case_id,
)
def test_per_layer_only_sizes(hal, oracle, case):
    el, tw, shape = case
    run_case(hal, oracle, "layer", el, tw, shape)


# ---------------------------------------------------------------------------------- (c) dispatch edges
def test_edge_of_the_bit_sliced_threshold(hal, oracle):
    """B32 / B32 at log_y = 13 (tiled) and 14 (bit-sliced): the smaller input is the prefix of the larger (same SplitMix stream)."""
    a = run_case(hal, oracle, "tiled", 5, 5, (14, 0, 13, 0, 0, 0, 0))
    b = run_case(hal, oracle, "bs", 5, 5, (14, 0, 14, 0, 0, 0, 0))
    assert not np.array_equal(a, b[: a.nbytes])


def test_edge_of_the_tiled_threshold(hal, oracle):
    """B64 / B16 with 2^11 elements (per-layer) and 2^12 (tiled)."""
    run_case(hal, oracle, "layer", 6, 4, (12, 0, 11, 0, 0, 0, 0))
    run_case(hal, oracle, "tiled", 6, 4, (12, 0, 12, 0, 0, 0, 0))
    run_case(hal, oracle, "layer", 6, 4, (12, 2, 7, 2, 3, 2, 0))
    run_case(hal, oracle, "tiled", 6, 4, (12, 2, 7, 3, 3, 2, 0))


def test_bit_sliced_declines_wide_batches_and_the_tiled_kernel_takes_14_layers(hal, oracle):
    """B128 / B32, log_y = 14, log_x = 9, log_z = 3: as B32 columns lx + log_z = 11 + 3 > 12, the bit-sliced launcher declines and the
    tiled kernel runs a 14-layer transform (three passes) of 2^12 columns.

    The scalar oracle needs minutes for 2^26 elements with this stride, so the columns are drawn from 32 random ones (a pseudo-random
    one per (x, z)): the oracle transforms each of the 32 once, as a plain transform -- batches are the transform column by column,
    pinned in tests/test_oracle_ntt_pairs.py -- and every one of the 2^26 outputs is compared with the oracle's value."""
    el, tw, K = 7, 5, 32
    shape = (16, 9, 14, 3, 1, 1, 0)
    ld, lx, ly, lz, coset, cb, skip = shape
    s = s_evals(oracle, tw, ld)

    def build(seed, ref):
        cols = oracle.random_b128(seed, K << ly).reshape(K, 1 << ly, 2)
        want = cols.copy()
        with ThreadPoolExecutor(8) as ex:
            assert not any(ex.map(lambda k: ref(want[k], el, tw, s, ld, 0, ly, 0, coset, cb, skip), range(K)))
        pick = (oracle.splitmix_words(seed ^ 0xF00D, 1 << (lx + lz)) % np.uint64(K)).astype(np.intp).reshape(1 << lz, 1 << lx)
        assert len(np.unique(pick)) == K

        def spread(c):  # [z][y][x] = c[pick[z][x]][y]
            cy = np.ascontiguousarray(c.transpose(1, 0, 2)).view(np.complex128)[:, :, 0]  # (one 16-byte item per element)
            out = np.empty((1 << lz, 1 << ly, 1 << lx), dtype=np.complex128)
            for z in range(1 << lz):
                np.take(cy, pick[z], axis=1, out=out[z], mode="clip")
            return out.reshape(-1).view(np.uint8)

        return spread(cols), spread(want)

    x, want_f = build(0xB16, oracle.ntt_forward)
    y, want_i = build(0xB17, oracle.ntt_inverse)
    device_case(hal, "tiled", el, tw, s, shape, x, y, want_f, want_i)


# ---------------------------------------------------------------------------------- (d) validation
def test_rejected_calls_touch_nothing(hal, oracle):
    import binius_amd

    s = binius_amd.ntt_s_evals(6, 9)
    x = rand_bytes(oracle, 0xDEAD, 1 << 12)
    alloc = hal.dev_alloc()
    dx, chk = A.place(hal, alloc, as16(x), 5)
    c0 = hal.ntt_counters()
    #           elem tw  log_domain log_x log_y log_z coset coset_bits skip
    for args in ((5, 2, 4, 0, 4, 0, 0, 0, 0),  # tw_level 2
                 (7, 7, 8, 0, 8, 0, 0, 0, 0),  # tw_level 7
                 (3, 4, 8, 0, 8, 0, 0, 0, 0),  # twiddle field larger than the element field
                 (3, 3, 9, 0, 8, 0, 0, 0, 0),  # B8 twiddles have no domain of 2^9 points
                 (5, 5, 9, 1, 6, 1, 0, 0, 7)):  # skip_rounds > log_y
        for call in (hal.ntt_forward, hal.ntt_inverse):
            with pytest.raises(binius_amd.BnError) as e:
                call(dx.ptr, args[0], args[1], s, *args[2:])
            assert e.value.kind == "InputValidation", args
    chk()
    assert hal.ntt_counters() == c0
    # accepted no-ops: nothing to do, nothing counted
    for args in ((5, 5, 9, 1, 6, 1, 0, 0, 6),  # skip_rounds == log_y
                 (6, 4, 9, 3, 0, 4, 0, 0, 0)):  # log_y == 0
        for call, ref in ((hal.ntt_forward, oracle.ntt_forward), (hal.ntt_inverse, oracle.ntt_inverse)):
            call(dx.ptr, args[0], args[1], s, *args[2:])
            w = x.copy()
            assert ref(w, args[0], args[1], s, *args[2:]) == 0 and np.array_equal(w, x)
    chk()
    assert hal.ntt_counters() == c0
    # and the context still works
    run_case(hal, oracle, "layer", 5, 5, (9, 1, 6, 1, 1, 2, 0))
