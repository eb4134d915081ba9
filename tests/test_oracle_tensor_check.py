"""Pins tests/tensor_check_ref.py (CPU only): the tables tests/test_gpu_tensor_check.py hands to the device check fail the plain
definition exactly where they are meant to -- one comparison for an isolated probe, several for a defining entry -- and the index sets
are the ones the kernel's layout calls for.  If the algebra behind isolate() were wrong for some class of indices, this is where it
would show, before a GPU is involved."""
import numpy as np
import pytest

import tensor_check_ref as T


@pytest.fixture(scope="module")
def tables(oracle):
    return {K: T.expansion(oracle.random_scalars(0x7C0000 + K, K)) for K in (9, 10, 11, 12, 13, 14)}


def test_a_genuine_expansion_and_its_multiples_have_the_structure(oracle, tables):
    for K, t in tables.items():
        assert T.failing(t) == []
        assert T.failing(T.scale(t, T.KAPPA)) == []
        assert T.failing(T.scale(t, (1 << 128) - 1)) == []
    # ... and failing() is the definition, not a restatement of isolate(): random data fails (nearly) everywhere but at the defining entries
    r = oracle.random_b128(0x7C1000, 1 << 9)
    assert T.failing(r) == [i for i in range(1, 1 << 9) if i & (i - 1)]


def test_every_entry_of_the_smallest_table_is_isolated(tables):
    t = tables[9]
    for p in range(1, 512):
        if p & (p - 1):
            assert T.failing(T.isolate(t, p)) == [p], p


@pytest.mark.parametrize("K", [10, 11, 12, 13, 14])
def test_the_structured_entries_are_isolated(tables, K):
    t = tables[K]
    probes = T.probe_indices(K)
    assert probes == sorted(set(probes))
    for p in probes:
        assert 1 <= p < 1 << K and p & (p - 1)
        assert T.failing(T.isolate(t, p)) == [p], T.describe(K, p)
    # every range is there with its first lanes, its last entry, and entries in each of the four slots a lane keeps in flight
    for k in range(8, K):
        mine = [p for p in probes if p.bit_length() - 1 == k]
        assert (1 << k) + 1 in mine and (2 << k) - 1 in mine
        assert {((p - (1 << k)) >> 8) & 3 for p in mine} ==set(range(min(4, 1 << (k - 8))))
    assert all(p in probes for p in T.HEAD)


def test_the_layout_restated():
    """One workgroup per 4096 entries, between 1 and 512 per range; 1024 entries per workgroup and trip."""
    assert [T.range_workgroups(k) for k in (8, 9, 11, 12, 13, 14, 16, 21, 22, 30)] == [1, 1, 1, 1, 2, 4, 16, 512, 512, 512]
    assert [T.range_trips(k) for k in (8, 9, 10, 11, 12, 13, 16, 21, 22, 23)] == [1, 1, 1, 2, 4, 4, 4, 4, 8, 16]
    for k in range(8, 24):  # the workgroups of a range cover it exactly (from range 10 on; ranges 8 and 9 are shorter than one trip)
        assert T.range_workgroups(k) * T.range_trips(k) * 1024 == max(1 << k, 1024)
    # the largest size probed has ranges dealt to 2, 4, 8 and 16 workgroups, and the probes reach the last workgroup's last trip
    p17 = T.probe_indices(17)
    assert {T.range_workgroups(k) for k in range(8, 17)} == {1, 2, 4, 8, 16}
    for k in range(10, 17):
        n_wg, trips = T.range_workgroups(k), T.range_trips(k)
        assert (1 << k) + (n_wg - 1) * 1024 + (trips - 1) * n_wg * 1024 + 3 * 256 + 255 == (2 << k) - 1 and (2 << k) - 1 in p17
    assert len(p17) < 600
    # where() takes an index apart the way probe_indices() put it together
    assert T.where((1 << 16) + 15 * 1024 + 3 * 16 * 1024 + 2 * 256 + 63) == (16, 15, 3, 2, 63)
    assert T.where((1 << 13) + 1024 + 256 + 64) == (13, 1, 0, 1, 64)
    assert T.where(511) == (8, 0, 0, 0, 255) and T.where(1023) == (9, 0, 0, 1, 255) and T.where(129) == (7, 0, 0, 0, 129)
    for K in (14, 17):
        seen = {T.where(p)[:3] for p in T.probe_indices(K)}
        for k in range(8, K):
            n_wg, trips = T.range_workgroups(k), T.range_trips(k)
            assert {(k, part, trip) for part in (0, n_wg - 1) for trip in (0, trips - 1)} <= seen


def test_a_narrowed_partition_leaves_out_a_probed_entry():
    """The partition as written compares every entry of [1, n) exactly once; each narrowing of it -- the head cut short, a range
    looked up one workgroup late, the last workgroup of a range doing another's part, the loop one stride short, one of the four
    slots dropped -- leaves out entries, and at least one of them is probed by tests/test_gpu_tensor_check.py at that size (the
    K = 9 sweep probes everything; from K = 10 on, probe_indices)."""
    for K in (8, 9, 10, 11, 12, 13, 14, 17):
        assert sorted(T.visits(K)) == list(range(1, 1 << K)), K
    caught = {}
    for K in (9, 10, 11, 12, 13, 14, 17):
        probed = set(range(1, 1 << K)) if K == 9 else set(T.probe_indices(K))
        for how in T.NARROWINGS:
            left_out = set(range(1, 1 << K)) - set(T.visits(K, how))
            if left_out:
                assert left_out & probed, (K, how, "skips %d entries, none of them probed" % len(left_out))
                caught.setdefault(how, []).append(K)
    # every narrowing bites at some size -- the head at all of them, several workgroups per range from K = 14
    assert caught["head"] == [9, 10, 11, 12, 13, 14, 17] and caught["part"] == [14, 17] and set(caught) == set(T.NARROWINGS), caught


def test_a_defining_entry_fails_in_several_places(tables):
    """p = 2^k0 altered: rho_k0 changes, so the range k0 fails (where it has more than its defining entry), and so does every
    2^k0 + 2^j above it.  Nothing below range k0 notices."""
    for K in (9, 13):
        t = tables[K]
        for k0 in range(K):
            bad = T.failing(T.alter(t, 1 << k0))
            assert bad is not None and len(bad) > 1, (K, k0)
            assert min(bad) >= 1 << k0
            assert 1 << k0 not in bad
            assert set(bad) == set(range((1 << k0) + 1, 2 << k0)) | {(1 << k0) + (1 << j) for j in range(k0 + 1, K)}
        bad = T.failing(T.alter(t, 0))
        assert bad == [i for i in range(1, 1 << K) if i & (i - 1)]  # (a power of two is compared with t[0] * rho: true by definition)


def test_one_flipped_bit_in_the_top_range_fails_there_alone(tables):
    t = tables[13]
    p = (1 << 12) + 2741
    for bit in (0, 31, 32, 63, 64, 95, 96, 127):
        f = T.flip(t, p, bit)
        assert np.count_nonzero(f != t) == 1
        assert T.failing(f) == [p]


def test_coordinates_zero_and_one_have_no_ratios(oracle):
    for pos in (0, 7, 8, 10):
        for v in (0, 1):
            c = oracle.random_scalars(0x7C2000 + pos, 11)
            c[pos] = v
            assert T.failing(T.expansion(c)) is None
