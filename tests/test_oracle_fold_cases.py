"""Pins of the case tables of tests/fold_cases.py, on the CPU, so that tests/test_gpu_fold_routes.py checks what it was written to check:

* every row's hand-written route and branch tags are what the restated routing predicates and kernel constants give for its shape on a
  device of 256 compute units, and the sizes written as rules resolve to the sizes the rules are named after on other devices too;
* every branch the tables are there for is claimed by a case;
* the restated constants of k_fold_tab are the kernel's (P, J, G, KG, EB, NU4 per level, written out);
* the names of Context.fold_counters() / inner_product_counters() follow the enums of include/binius_amd.h;
* oracle.fold_left / fold_right / inner_product agree with a pure-Python evaluation of their definitions (sharing only the scalar product,
  which tests/test_oracle_field.py pins to the golden vectors) at the edges the other pins leave out: one vector element, one output, an
  inner product whose length is no power of two; and the oracle-free expectation of the one-hot runs is the oracle's.
"""
import os
import re

import numpy as np
import pytest

import fold_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("case", F.FOLD_CASES, ids=lambda c: c.id)
def test_fold_case_claims_what_its_shape_gives(case):
    c = case
    n_out = F.out_len(c)
    assert n_out & (n_out - 1) == 0 and c.vec_len & (c.vec_len - 1) == 0
    route, tags = F.fold_tags(c.op, c.level, c.vec_len, n_out)
    assert route == c.route, "case %s is answered by %s" % (c.id, route)
    assert tags == c.tags, "case %s: claimed %s, its shape gives %s" % (c.id, sorted(c.tags), sorted(tags))
    assert route.startswith(c.op)
    # the routing above the table kernel: no row of 512 .. 2048 bits with 4096 outputs and more, no long vector over few outputs
    if route == "right_tab":
        assert not (n_out >= 4096 and (c.vec_len << c.level) in (512, 1024, 2048))
    if route == "left_tab":
        assert not (c.vec_len >= 4096 and n_out <= 1024) and not (c.level == 5 and n_out >= 4096 and c.vec_len in (16, 32, 64))
    d, last = F.fold_counters(c.op, c.level, c.vec_len, n_out, F.NOMINAL_CU)
    assert sum(d[k] for k in F.FOLD_ROUTES) == 1 and sum(d[k] for k in F.FOLD_RINGS) == (1 if route.endswith("_mfma") else 0)
    assert (last is not None) == route.endswith("_mfma")


@pytest.mark.parametrize("case", F.IP_CASES, ids=lambda c: c.id)
def test_inner_product_case_claims_what_its_shape_gives(case):
    c = case
    route, tags = F.ip_tags(c.level, F.ip_len(c))
    assert route == c.route, "case %s is answered by %s" % (c.id, route)
    assert tags == c.tags, "case %s: claimed %s, its shape gives %s" % (c.id, sorted(c.tags), sorted(tags))
    assert sum(F.ip_counters(c, F.NOMINAL_CU).values()) == 1


def test_every_branch_is_claimed_by_a_case():
    claimed = set().union(*(c.tags for c in F.FOLD_CASES))
    missing = [t for t in F.FOLD_REQUIRED_TAGS if t not in claimed]
    assert not missing, "no fold case claims %s" % missing
    assert claimed <= set(F.FOLD_REQUIRED_TAGS), "tags that no one asked for: %s" % sorted(claimed - set(F.FOLD_REQUIRED_TAGS))
    assert {c.route for c in F.FOLD_CASES} == set(F.FOLD_ROUTES)
    claimed = set().union(*(c.tags for c in F.IP_CASES))
    missing = [t for t in F.IP_REQUIRED_TAGS if t not in claimed]
    assert not missing, "no inner-product case claims %s" % missing
    assert claimed <= set(F.IP_REQUIRED_TAGS)
    assert {c.route for c in F.IP_CASES} == set(F.IP_ROUTES)
    # the list the tables were written from, spelled out once more (F.FOLD_REQUIRED_TAGS is built with loops)
    for t in ("tab:wide@3", "tab:wide@4", "tab:wide@5", "tab:narrow-right", "tab:left", "tab:chunks>=2@3", "tab:chunks>=2@4", "tab:chunks>=2@5", "tab:vec1",
              "tab:partial-group", "scalar:stride", "scalar:out1", "scalar:vec1", "scalar@0", "scalar@3", "scalar@4", "scalar@5", "scalar@6", "scalar@7",
              "ring<2>:pairs=1", "ring<2>:pairs=2", "ring<2>:pairs=4", "ring<4>:pairs=1", "ring<4>:pairs=2", "ring<4>:pairs=4", "ring<8>:pairs=1",
              "ring<8>:pairs=2", "ring<8>:pairs=4", "ring_left<2>:pairs=1", "ring_left<2>:pairs=2", "ring_left<2>:pairs=4", "ring_left<4>:pairs=1",
              "ring_left<4>:pairs=2", "ring_left<4>:pairs=4", "ring_left<8>:pairs=1", "ring_left<8>:pairs=2", "ring_left<8>:pairs=4",
              "ring:prep<0>:pairs>=2", "ring:prep<3>:pairs>=2", "ring:prep<4>:pairs>=2", "left:pe-routed"):
        assert t in F.FOLD_REQUIRED_TAGS, t


def test_the_issue_s_shapes_are_in_the_table():
    for cid in ("right-l3-v32-o1024", "right-l3-v256-o1024", "right-l4-v128-o1024", "left-l3-v256-o2048", "left-l4-v128-o2048", "right-l0-v1024-o1",
                "right-l7-v1024-o1", "right-l0-v2-ostride2", "right-l6-v2-ostride2", "right-l7-v2-ostride2", "right-l0-v2048-opairs4", "left-l5-v64-opairs4"):
        assert cid in F.FOLD_BY_ID, cid
    for level in (3, 4, 5):
        for op in ("left", "right"):
            for v in (1, 2):
                assert "%s-l%d-v%d-o1024" % (op, level, v) in F.FOLD_BY_ID
    assert sorted(F.ip_len(c) for c in F.IP_CASES if c.level == 5 and F.ip_len(c) > 2000) == [7680, 8192, 8448, 8704]
    assert sorted(F.ip_len(c) for c in F.IP_CASES if c.level == 7) == [1, 2, 3, 1025, 1536, 130560, 130562]
    assert sorted(c.level for c in F.IP_CASES if F.ip_len(c) == 3 << 9) == list(F.LEVELS)


def test_sizes_written_as_rules():
    by = F.FOLD_BY_ID
    assert F.out_len(by["right-l0-v512-opairs2"]) == 1 << 16 and F.out_len(by["right-l0-v512-opairs4"]) == 1 << 17
    assert F.out_len(by["right-l7-v2-ostride2"]) == 1 << 20 and F.mat_len(by["right-l7-v2-ostride2"]) * 16 == 32 << 20
    assert F.ring_pairs(1 << 15, 256) == 1 and F.ring_pairs(1 << 16, 256) == 2 and F.ring_pairs(1 << 17, 256) == 4
    assert F.scalar_outputs_per_thread(1 << 19, 256) == 1 and F.scalar_outputs_per_thread(1 << 20, 256) == 2
    # other devices: the rule still gives what it is named after (out_len asserts minimality itself)
    for n_cu in (64, 104, 120, 228, 256, 304):
        for c in F.FOLD_CASES:
            if isinstance(c.out, tuple):
                n = F.out_len(c, n_cu)
                route, tags = F.fold_tags(c.op, c.level, c.vec_len, n, n_cu)
                assert route == c.route and n & (n - 1) == 0
                if c.out[0] == "pairs":
                    assert F.ring_pairs(n, n_cu) >= c.out[1] and F.ring_grid(n, n_cu) == 2 * n_cu
                else:
                    assert F.scalar_outputs_per_thread(n, n_cu) >= c.out[1] and "scalar:stride" in tags
        lo, hi = (F.ip_len(F.IP_BY_ID["ip-l7-mfma%d" % s], n_cu) for s in (0, 1))
        assert hi == lo + 2
        assert F.ip_route(7, lo, n_cu) == "split9"
        assert F.ip_route(7, hi, n_cu) == "mfma_split"


def test_table_kernel_constants():
    assert F.tab_consts(3) == {"P": 2, "J": 128, "G": 32, "KG": 8, "EB": 1, "NU4": 2}
    assert F.tab_consts(4) == {"P": 4, "J": 64, "G": 32, "KG": 4, "EB": 2, "NU4": 4}
    assert F.tab_consts(5) == {"P": 8, "J": 32, "G": 32, "KG": 2, "EB": 4, "NU4": 8}
    for level in (3, 4, 5):
        c = F.tab_consts(level)
        assert c["J"] * c["P"] * 256 == 65536 and c["KG"] * c["P"] == 16 and c["NU4"] * 16 == c["G"] * c["EB"] and c["G"] == F.G
    # with one or two vectors the lookup loop leaves at its first or second group at level 3 (KG = 8 entries a group) ...
    assert F.tab_consts(3)["KG"] > 2
    # ... and a chunk of level 5 holds exactly one group: its second chunk starts a new table build
    assert F.tab_consts(5)["J"] == F.tab_consts(5)["G"]


def test_counter_names_follow_the_header():
    import binius_amd._ffi as f

    text = open(os.path.join(ROOT, "include", "binius_amd.h")).read()
    fold = re.search(r"enum\s*\{([^}]*BN_FOLD_N[^}]*)\}", text).group(1)
    names = {m.group(1): int(m.group(2)) for m in re.finditer(r"BN_FOLD_(\w+)\s*=\s*(\d+)", fold)}
    assert names.pop("N") == len(f.Context.FOLD_COUNTERS) == len(names)
    assert [k for k, _ in sorted(names.items(), key=lambda kv: kv[1])] == [k.upper() for k in f.Context.FOLD_COUNTERS]
    assert f.Context.FOLD_COUNTERS == F.FOLD_ROUTES + F.FOLD_RINGS + F.FOLD_LAST + F.FOLD_INFO
    ip = re.search(r"enum\s*\{([^}]*BN_IP_N[^}]*)\}", text).group(1)
    names = {m.group(1): int(m.group(2)) for m in re.finditer(r"BN_IP_(\w+)\s*=\s*(\d+)", ip)}
    assert names.pop("N") == len(F.IP_ROUTES)
    assert [k for k, _ in sorted(names.items(), key=lambda kv: kv[1])] == ["MFMA_SPLIT", "SPLIT9", "IP32", "SCALAR"] == [k.upper() for k in F.IP_ROUTES]
    for sym in ("bn_fold_counters", "bn_inner_product_counters"):
        assert sym in f.ABI_SYMBOLS


# ---------------------------------------------------------------------------------------------- the oracle at the edges
def py_limb(packed, idx, level):
    """value idx of the packed level-`level` array: 2^level bits, least-significant first in the little-endian bytes (iter_bases)"""
    bits = 1 << level
    whole = int.from_bytes(np.ascontiguousarray(packed).tobytes(), "little")
    return (whole >> (idx * bits)) & ((1 << bits) - 1)


def py_fold(oracle, left, mat, level, vec, n_out):
    v = oracle.arr_to_ints(vec)
    out = []
    for i in range(n_out):
        acc = 0
        for j in range(len(v)):
            acc ^= oracle.mul(v[j], py_limb(mat, j * n_out + i if left else i * len(v) + j, level))  # (a subfield element embeds as its low bits)
        out.append(acc)
    return out


# (level, vec_len, out_len): one vector element; one output; both; an ordinary shape next to them
EDGE_FOLDS = [(0, 1, 128), (3, 1, 16), (5, 1, 4), (7, 1, 2), (0, 128, 1), (4, 8, 1), (7, 4, 1), (7, 1, 1), (6, 1, 2), (3, 4, 8), (5, 2, 2)]


@pytest.mark.parametrize("level,vec_len,n_out", EDGE_FOLDS)
@pytest.mark.parametrize("left", [True, False], ids=["left", "right"])
def test_oracle_folds_at_the_edges(oracle, left, level, vec_len, n_out):
    n_mat = ((vec_len * n_out) << level) // 128
    assert n_mat >= 1 and n_mat * 128 == (vec_len * n_out) << level
    mat, vec = oracle.random_b128(0xED6E + level, n_mat), oracle.random_b128(0xED6F + vec_len, vec_len)
    out = oracle.arr(n_out)
    assert (oracle.fold_left if left else oracle.fold_right)(mat, level, vec, out) == 0
    assert oracle.arr_to_ints(out) == py_fold(oracle, left, mat, level, vec, n_out)


@pytest.mark.parametrize("level,n_b", [(0, 3 << 7), (3, 48), (4, 24), (5, 12), (6, 6), (7, 3), (7, 1), (7, 2), (5, 4)])
def test_oracle_inner_product_at_lengths_that_are_no_power_of_two(oracle, level, n_b):
    a, b = oracle.random_b128(0x1B0 + level, n_b >> (7 - level)), oracle.random_b128(0x1B8, n_b)
    rc, got = oracle.inner_product(a, level, b)
    want = 0
    for i, x in enumerate(oracle.arr_to_ints(b)):
        want ^= oracle.mul(x, py_limb(a, i, level))
    assert rc == 0 and got == want


def test_oracle_rejects_lengths_that_do_not_match(oracle):
    assert oracle.inner_product(oracle.arr(3), 5, oracle.arr(8))[0] != 0
    assert oracle.fold_right(oracle.arr(4), 7, oracle.arr(2), oracle.arr(4)) != 0
    assert oracle.fold_left(oracle.arr(4), 2, oracle.arr(2), oracle.arr(2)) != 0


@pytest.mark.parametrize("op,level,vec_len,n_out", [("right", 0, 512, 4), ("right", 3, 64, 4), ("right", 4, 8, 8), ("left", 5, 16, 8), ("right", 6, 8, 4),
                                                    ("right", 7, 4, 4), ("left", 3, 16, 16)])
def test_the_one_hot_expectation_is_the_oracle_s(oracle, op, level, vec_len, n_out):
    c = F.FoldCase("x", op, level, vec_len, n_out, None, frozenset())
    mat = oracle.random_b128(0x0E07 + level, F.mat_len(c))
    vec, j = F.one_hot(vec_len)
    assert 0 < j < vec_len and vec[j, 0] == 1 and int(vec.sum()) == 1
    out = oracle.arr(n_out)
    assert (oracle.fold_left if op == "left" else oracle.fold_right)(mat, level, vec, out) == 0
    want = F.one_hot_expected(mat, level, c, j, n_out)
    assert np.array_equal(out, want) and want.any()
