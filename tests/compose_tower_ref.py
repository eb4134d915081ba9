"""TEST INFRASTRUCTURE: CPU restatement of bn_compute_composite with a tower-typed expression (bn_expr_compile_tower), written from the
contract of include/binius_amd.h; it does not import binius_amd and uses no packed-word tricks.

A column is its values in the layout of tests/univariate_skip_base_ref.py: level 0 / 3 a uint8 array (0 / 1, or bytes), level 4 .. 7 a
uint8 array of shape (N, 2^(level - 3)) -- the little-endian bytes of every value.  `evaluate` unpacks nothing itself: it takes such
values, embeds every one as a BinaryField128b element (the tower embedding is the identity on the low bits), evaluates the steps with
oracle.compute_composite in B128, asserts that every result is below 2^(2^out_level) -- subfields are closed -- and returns the values at
the output level; `pack` / `unpack` are the (len, 2) uint64 layout of bn_hal_multilinear.

  random_values(rng, level, n)      n uniform values of the level
  constant(value, level, n)         n copies of one value
  embed(values, level)              -> (N, 2) uint64 B128 elements
  evaluate(steps, cols, out_level)  cols: [(values, level), ...] -> values at out_level
  evaluate_packed(...)              the same, packed
  const_level / step_levels         the level rules of the contract (VAR its input's, CONST the smallest that holds it, ADD / MUL the
                                    maximum, POW its base's)
  pack_steps(n_bits)                sum of bit_i * 2^i, left-deep: pack_fp / pack_b8 of m3's gadgets (4 n - 1 steps)"""
import numpy as np

import oracle as o
import univariate_skip_base_ref as U

LEVELS = (0, 3, 4, 5, 6, 7)
pack, unpack, const_level = U.pack, U.unpack, U.const_level


def random_values(rng, level, n):
    if level == 0:
        return rng.integers(0, 2, size=n, dtype=np.uint8)
    if level == 3:
        return rng.integers(0, 256, size=n, dtype=np.uint8)
    return rng.integers(0, 256, size=(n, 1 << (level - 3)), dtype=np.uint8)


def constant(value, level, n):
    assert value < 1 << (1 << level)
    if level in (0, 3):
        return np.full(n, value, dtype=np.uint8)
    row = np.frombuffer(int(value).to_bytes(1 << (level - 3), "little"), dtype=np.uint8)
    return np.tile(row, (n, 1))


def embed(values, level):
    b = U.as_bytes(values)
    assert b.shape[1] == (1 if level in (0, 3) else 1 << (level - 3))
    if level == 0:
        assert (b <= 1).all()
    raw = np.zeros((b.shape[0], 16), dtype=np.uint8)
    raw[:, : b.shape[1]] = b
    return raw.view(np.uint64).reshape(-1, 2).copy()


def step_levels(steps, input_levels):
    levels = []
    for s in steps:
        if s[0] == "var":
            levels.append(input_levels[s[1]])
        elif s[0] == "const":
            levels.append(const_level(s[1]))
        elif s[0] == "pow":
            levels.append(levels[s[1]])
        else:
            levels.append(max(levels[s[1]], levels[s[2]]))
    return levels


def evaluate(steps, cols, out_level):
    """The column out[i] = expr(in_0[i], ...) at out_level, from B128 arithmetic."""
    assert max(step_levels(steps, [lv for _, lv in cols])) <= out_level
    inputs = [embed(v, lv) for v, lv in cols]
    n = inputs[0].shape[0]
    assert all(a.shape[0] == n for a in inputs)
    out = np.zeros((n, 2), dtype=np.uint64)
    rc = o.compute_composite(inputs, out, steps, len(inputs))
    assert rc == 0, rc
    raw = np.ascontiguousarray(out).view(np.uint8).reshape(n, 16)
    width = 1 if out_level in (0, 3) else 1 << (out_level - 3)
    assert not raw[:, width:].any(), "a result left the subfield of the output level"
    vals = raw[:, :width].copy()
    if out_level == 0:
        assert (vals <= 1).all(), "a result left B1"
    return vals.reshape(-1) if out_level in (0, 3) else vals


def evaluate_packed(steps, cols, out_level):
    return pack(evaluate(steps, cols, out_level), out_level)


def pack_steps(n_bits):
    steps, acc = [], None
    for i in range(n_bits):
        steps += [("var", i), ("const", 1 << i), ("mul", len(steps), len(steps) + 1)]
        if acc is not None:
            steps.append(("add", acc, len(steps) - 1))
        acc = len(steps) - 1
    return steps
