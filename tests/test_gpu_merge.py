"""bn_merge_multilins (csrc/kernels_merge.hip, abi_merge.cpp): merge_multilins of multilinears resident on the device, every case bit
for bit against piop_ref.merge_multilins on oracle.random_b128 data, tiled 2^log_repeats times.  The destination has a guard region
behind it and all of it is pre-filled with a non-zero pattern: a missing zero fill and a write past the end both show.  Shapes are
derived from T = BN_MERGE_TILE_LOG2: a multilinear of at least 2 T variables is a tiled job, a smaller one a small job."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4096
PATTERN = 0xA5A5A5A55A5A5A5A_0123456789ABCDEF
ARENA = (5 << 20) + (1 << 16)


def _t():
    from binius_amd._ffi import BN_MERGE_TILE_LOG2

    return BN_MERGE_TILE_LOG2


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    with binius_amd.Context(0, ARENA) as h:
        yield h


_DATA = {}


def data(oracle, seed, n_vars):
    """random multilinear (seed, n_vars), computed once and never modified"""
    key = (seed, n_vars)
    if key not in _DATA:
        _DATA[key] = oracle.random_b128(0x3E26E000 + 131 * seed + n_vars, 1 << n_vars)
        _DATA[key].setflags(write=False)
    return _DATA[key]


def upload(hal, alloc, arr):
    d = alloc.alloc(arr.shape[0])
    hal.copy_h2d(arr, d)
    return d


def run_case(hal, oracle, n_varss, total_vars=None, log_repeats=0, same_twice=False, launches=1):
    """Upload, merge, read back message + guard; compare with the oracle, the sources and the counters."""
    from oracle import piop_ref

    T = _t()
    mls = [data(oracle, 0 if same_twice else i, v) for i, v in enumerate(n_varss)]
    min_total = piop_ref.CommitMeta.with_vars(n_varss).total_vars
    total_vars = min_total if total_vars is None else total_vars
    assert total_vars >= min_total
    alloc = hal.dev_alloc()
    if same_twice:
        assert len(set(n_varss)) == 1
        one = upload(hal, alloc, mls[0])
        d_mls = [one] * len(n_varss)
    else:
        d_mls = [upload(hal, alloc, x) for x in mls]
    msg_len = 1 << (total_vars + log_repeats)
    region = alloc.alloc(msg_len + GUARD)
    hal.fill(region, PATTERN)
    before = hal.merge_counters()
    hal.merge_multilins(d_mls, region.slice(0, msg_len), total_vars, log_repeats)
    after = hal.merge_counters()
    got = hal.copy_d2h(region)
    want = np.concatenate([piop_ref.merge_multilins([np.array(x) for x in mls], total_vars)] * (1 << log_repeats))
    assert np.array_equal(got[:msg_len], want), "message differs from the oracle at element %d" % int(np.nonzero((got[:msg_len] != want).any(axis=1))[0][0])
    guard = got[msg_len:]
    assert (guard[:, 0] == (PATTERN & ((1 << 64) - 1))).all() and (guard[:, 1] == (PATTERN >> 64)).all(), "a write past the end of the message"
    for d, x in zip(d_mls, mls):
        assert np.array_equal(hal.copy_d2h(d), x), "a source was modified"
    tail = sum(1 << v for v in n_varss) < (1 << total_vars)
    n_tiled = sum(1 for v in n_varss if v >= 2 * T)
    delta = {k: after[k] - before[k] for k in after}
    assert delta == {"calls": 1, "launches": launches, "jobs": len(n_varss) + (1 if tail else 0), "jobs_tiled": n_tiled, "jobs_small": len(n_varss) - n_tiled}, delta


def single_sizes():
    T = _t()
    return sorted({0, 1, 2, T - 1, T, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 2, 2 * T + 3, 20})


@pytest.mark.parametrize("n_vars", single_sizes())
def test_single_multilinear(hal, oracle, n_vars):
    """Both sides of every form boundary, an odd and an even number of mid bits, one size with many units."""
    run_case(hal, oracle, [n_vars])


def mixes():
    n = 2 * _t() + 2
    return {
        "tiny": [0, 0, 1, 3],
        "tail": [4, 4, 6, 7],
        "exact": [5, 5, 6, 7],
        "tiled+small": [n - 3, n - 3, n - 1, n],
        "keccak-count": [5] * 3 + [8] * 100,
    }


@pytest.mark.parametrize("name", list(mixes()))
def test_mixes(hal, oracle, name):
    run_case(hal, oracle, mixes()[name])


def test_tail_longer_than_the_data(hal, oracle):
    """total_vars one above the minimum: more than half of every repeat is the zero job's."""
    run_case(hal, oracle, [4, 4, 6, 7], total_vars=9)
    run_case(hal, oracle, [2 * _t() + 1], total_vars=2 * _t() + 2)


def test_same_source_twice(hal, oracle):
    run_case(hal, oracle, [2 * _t(), 2 * _t()], same_twice=True)
    run_case(hal, oracle, [3, 3], same_twice=True)


def test_more_jobs_than_one_launch_holds(hal, oracle):
    """4100 one-element multilinears and the tail are 4101 jobs; the table of a launch holds 4096: the call is split, not rejected."""
    run_case(hal, oracle, [0] * 4100, same_twice=True, launches=2)


def test_no_multilinears_is_a_zero_fill(hal, oracle):
    run_case(hal, oracle, [], total_vars=0)
    run_case(hal, oracle, [], total_vars=13, log_repeats=1)


@pytest.mark.parametrize("log_repeats", [0, 1, 2])
@pytest.mark.parametrize("name", ["tail", "tiled+small"])
def test_repeats(hal, oracle, name, log_repeats):
    run_case(hal, oracle, mixes()[name], log_repeats=log_repeats)


def _deferred_fold_case(oracle, state):
    import deferred_states as ds
    from oracle import piop_ref

    T = _t()
    for k in (3, 2 * T):
        other = data(oracle, 8, k + 1)
        box = {}

        def stage(pv, st):
            box["other"] = st.take(1 << (k + 1), "other")
            box["other"].host[:] = other
            box["msg"] = st.take(1 << (k + 2), "message")
            box["msg"].host[:] = (PATTERN & ((1 << 64) - 1), PATTERN >> 64)

        hal = ds.make_context(state, ds.region_elems(3, k + 1) + 4096)
        try:
            st = ds.reach(hal, oracle, state, seed=0x3E26 + k, stage=stage, log_n=k + 1)
            e0 = st.live[0]
            lo = np.array(e0.host)  # (the model: evals_0 folded with evals_1 by oracle.extrapolate_line)
            assert e0.n == 1 << k and not np.array_equal(lo, st.inputs[0].host[: 1 << k])
            hal.merge_multilins([e0.dev, box["other"].dev], box["msg"].dev, k + 2)
            got = hal.copy_d2h(box["msg"].dev)
            box["msg"].host[:] = piop_ref.merge_multilins([lo, np.array(other)], k + 2)
            assert np.array_equal(got, box["msg"].host)
            st.continuation()
            st.check_bytes()
        finally:
            hal.close()


def test_deferred_fold_is_visible(oracle):
    """On the context's own stream bn_extrapolate_line_batch is left deferred -- pending in the single-claim state (S1) or parked as
    a claim-group fold (S2), reached and proven by tests/deferred_states.py; the merge that follows reads the folded array."""
    for state in ("S1", "S2"):
        _deferred_fold_case(oracle, state)


def test_validation(hal, oracle):
    """Every rejection is BN_ERR_INPUT_VALIDATION, made before any launch: the counters and the destination stay as they were."""
    import binius_amd
    from binius_amd import BnError, DevSlice
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION

    alloc = hal.dev_alloc()
    a3, a4, b4 = (upload(hal, alloc, data(oracle, i, v)) for i, v in enumerate((3, 4, 4)))
    region = alloc.alloc(64 + GUARD)
    hal.fill(region, PATTERN)
    msg = region.slice(0, 64)
    before = hal.merge_counters()

    def rejected(multilins, message, total_vars, log_repeats=0, starts=None):
        with pytest.raises(BnError) as ei:
            hal.merge_multilins(multilins, message, total_vars, log_repeats)
        assert ei.value.code == BN_ERR_INPUT_VALIDATION
        text = binius_amd.lib().bn_last_error().decode()
        assert text.startswith("input validation: ")
        if starts:
            assert text[len("input validation: ") :].startswith(starts), text

    rejected([a3, a4], None, 6)  # null message
    rejected([a3, None], msg, 6)  # null multilinear
    rejected([a4, a3], msg, 6, starts="CommittedsNotSorted")
    rejected([a3, DevSlice(a4.ptr, 1 << 48)], DevSlice(msg.ptr, 1 << 47), 47)  # n_vars >= 48
    rejected([a3], DevSlice(msg.ptr, 1 << 47), 40, 8)  # total_vars + log_repeats >= 48
    rejected([a4, b4], msg.slice(0, 16), 4)  # more than 2^total_vars elements
    rejected([a4, b4], msg.slice(0, 32), 4, 1)  # (repeats do not make room)
    inside = msg.slice(8, 16)
    rejected([inside], msg, 6)  # a source inside the destination
    rejected([a3], DevSlice(a3.ptr + 16 * 4, 64), 6)  # a destination that starts inside a source
    rejected([a3], DevSlice(msg.ptr + 8, 64), 6)  # misaligned
    assert hal.merge_counters() == before
    got = hal.copy_d2h(region)
    assert (got[:, 0] == (PATTERN & ((1 << 64) - 1))).all() and (got[:, 1] == (PATTERN >> 64)).all()
    # and the same arguments in order are accepted
    hal.merge_multilins([a3, a4], msg, 6)
    assert hal.merge_counters()["calls"] == before["calls"] + 1
