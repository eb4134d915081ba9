"""Adversarial operands and framed placement, shared by tests/test_gpu_adversarial.py and tests/test_oracle_adversarial.py.

The parity tests elsewhere feed the kernels SplitMix64 data at allocator-aligned bases.  Here:

* ``operands(kind, seed, n)``: deterministic (n, 2) uint64 arrays of BinaryField128b elements whose VALUES are patterned --
  the matrix-core kernels count sums of GF(2) products in f32 accumulators and read data nibbles as E2M1 codes (bit 3 of a
  nibble is the format's sign bit and travels through separate words), so what arrives matters, not only how much of it.
* ``place(hal, alloc, arr, lead)``: the array at a base that is an ODD multiple of 16 bytes (the contract of
  include/binius_amd.h is 16-byte alignment, nothing more), framed by canaries on both sides.
"""
import numpy as np

M64 = (1 << 64) - 1
ALL_ONES = (1 << 128) - 1

KINDS = ("dense", "sparse", "zero", "nib8", "nib7", "limb0", "limb1", "limb2", "limb3", "sub0", "sub3", "sub5", "same")

# 0, 1, the generator of the tower's second level, an element of B8 \ B4, an element of B32 \ B16, the top basis element, all ones
EDGE_SCALARS = (0, 1, 2, 0x53, 0x9E3779B9, 1 << 127, ALL_ONES)


def _rnd(seed, n):
    import oracle

    return oracle.random_b128(seed & M64, n)


def _bit_arrays(seed, n):
    """One pseudo-random bit position 0 .. 127 per element as (word index, 64-bit mask)."""
    import oracle

    r = oracle.splitmix_words((seed ^ 0xB17B17) & M64, n) & np.uint64(127)
    return (r >> np.uint64(6)).astype(np.int64), np.uint64(1) << (r & np.uint64(63))


def operands(kind, seed, n):
    """(n, 2) uint64 array (lo, hi) of the operand class `kind`:

    dense     all 128 bits set, then one pseudo-random bit cleared per element (127 bits set)
    sparse    exactly one pseudo-random bit set per element
    zero      all zero
    nib8      random AND 0x8888...: only bit 3 of every nibble can be set (the E2M1 sign-bit detour alone)
    nib7      random AND 0x7777...: bit 3 of every nibble clear (everything but the detour)
    limb<j>   random in the 32-bit limb j = 0 .. 3, zero elsewhere
    sub<l>    random elements of the level-l subfield (2^l bits: the low bits of the element in the tower basis), l = 0, 3, 5
    same      random (the class is about pairing: pair() hands out two buffers with equal values)
    random    SplitMix64, what every other parity test uses
    """
    if kind in ("random", "same"):
        return _rnd(seed, n)
    if kind == "zero":
        return np.zeros((n, 2), dtype=np.uint64)
    if kind in ("dense", "sparse"):
        w, m = _bit_arrays(seed, n)
        out = np.zeros((n, 2), dtype=np.uint64)
        out[np.arange(n), w] = m
        return ~out if kind == "dense" else out
    if kind == "nib8":
        return _rnd(seed, n) & np.uint64(0x8888888888888888)
    if kind == "nib7":
        return _rnd(seed, n) & np.uint64(0x7777777777777777)
    if kind.startswith("limb"):
        j = int(kind[4:])
        assert 0 <= j < 4
        out = np.zeros((n, 2), dtype=np.uint64)
        out[:, j >> 1] = _rnd(seed, n)[:, 0] & np.uint64(0xFFFFFFFF << (32 * (j & 1)))
        return out
    if kind.startswith("sub"):
        level = int(kind[3:])
        assert 0 <= level <= 6
        out = np.zeros((n, 2), dtype=np.uint64)
        out[:, 0] = _rnd(seed, n)[:, 0] & np.uint64((1 << (1 << level)) - 1)
        return out
    raise ValueError(kind)


def pair(kind, seed, n):
    """Two operands of a product.  `zero`: a zero array against a random one; `same`: equal values in separate buffers;
    every other kind: two independent arrays of the kind."""
    if kind == "zero":
        return operands("zero", seed, n), operands("random", seed + 1, n)
    if kind == "same":
        a = operands("random", seed, n)
        return a, a.copy()
    return operands(kind, seed, n), operands(kind, seed + 1, n)


def unpack_subfield(a, level):
    """The packed level-`level` values of `a` (2^(7 - level) per element, little-endian memory order, layer.rs inner_product /
    fold_right) as one BinaryField128b element each: a subfield element is the low 2^level bits of its embedding.  Lets the
    PCLMULQDQ oracle's F x F inner product serve as the reference of the subfield x F one (pinned against the scalar oracle in
    tests/test_oracle_adversarial.py)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if level == 0:
        vals = np.unpackbits(raw, bitorder="little")
    elif level == 7:
        return np.ascontiguousarray(a)
    else:
        vals = raw.view({3: np.uint8, 4: np.uint16, 5: np.uint32, 6: np.uint64}[level])
    out = np.zeros((vals.shape[0], 2), dtype=np.uint64)
    out[:, 0] = vals
    return out


def popcounts(a):
    """Set bits per element."""
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], 16), axis=1).sum(axis=1)


# ---- placement
FRAME = 4096  # elements of canary in front of and behind an array: the largest tile a kernel stages is 256 points x 4 arrays
CANARY = 0xC0DEC0DEC0DEC0DE5A5A5A5A5A5A5A5A


def place(hal, alloc, arr, lead):
    """Put `arr` (an (n, 2) array, or a length for an output) into a fresh block FRAME + pad + n + FRAME elements long that is
    filled with CANARY, at the first element behind the front frame whose ADDRESS is `lead` elements modulo 16 -- with an odd
    lead the base is an odd multiple of 16 bytes, and arrays placed with different leads differ in their offset modulo 256
    bytes.  Returns (slice, check): check(expect=None) reads the whole block back and asserts both frames intact and the
    body equal to `expect` (default: what was uploaded -- a read-only input is unchanged; for an output pass the oracle's
    array; check(None) on an output asserts it still holds the canary, i.e. nothing was written; check(body=False) looks at the
    frames only -- scratch space)."""
    n = arr if isinstance(arr, int) else arr.shape[0]
    block = alloc.alloc(FRAME + 16 + n + FRAME)
    at = FRAME + ((lead - (block.ptr // 16 + FRAME)) % 16)
    assert block.ptr % 16 == 0 and (block.ptr // 16 + at) % 16 == lead % 16
    hal.fill(block, CANARY)
    s = block.slice(at, at + n)
    if not isinstance(arr, int):
        hal.copy_h2d(arr, s)
    lo, hi = np.uint64(CANARY & M64), np.uint64(CANARY >> 64)

    def check(expect=None, body=True):
        got = hal.copy_d2h(block)
        for name, part in (("in front of", got[:at]), ("behind", got[at + n :])):
            bad = np.flatnonzero((part[:, 0] != lo) | (part[:, 1] != hi))
            assert bad.size == 0, "canary %s the array broken (lead %d): %d elements, the first at %d" % (name, lead, bad.size, bad[0])
        if not body:
            return None
        body = got[at : at + n]
        if expect is None and isinstance(arr, int):
            assert ((body[:, 0] == lo) & (body[:, 1] == hi)).all(), "an untouched output was written to"
        else:
            want = arr if expect is None else expect
            assert np.array_equal(body, want), "array body differs (lead %d)" % lead
        return body

    return s, check
