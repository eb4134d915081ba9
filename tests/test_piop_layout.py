"""The host arithmetic of the device-side commit (no GPU): bnh_piop_message_layout against the oracle's CommitMeta and the offsets
that piop_ref.merge_multilins implies, bnh_piop_commit_elems against the sizes of piop_ref.fri_commit's outputs, and the new
symbols of both libraries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [[4, 4, 6, 7], [4, 4, 6, 6, 6, 7], [5, 5, 6, 7], [0], []]


@pytest.mark.parametrize("n_varss", SHAPES, ids=lambda s: "-".join(map(str, s)) or "empty")
def test_message_layout_vs_oracle(n_varss):
    """A distinct marker value per multilinear (its index + 1 in every element): where the oracle's merge puts it is the offset."""
    from binius_amd._host import piop_message_layout
    from oracle import piop_ref

    offsets, total_vars = piop_message_layout(n_varss)
    meta = piop_ref.CommitMeta.with_vars(n_varss)
    assert total_vars == meta.total_vars
    mls = [np.full((1 << v, 2), i + 1, dtype=np.uint64) for i, v in enumerate(n_varss)]
    msg = piop_ref.merge_multilins(mls, meta.total_vars)
    assert len(offsets) == len(n_varss)
    for i, v in enumerate(n_varss):
        where = np.nonzero(msg[:, 0] == i + 1)[0]
        assert where.shape[0] == 1 << v and where[0] == offsets[i] and where[-1] == offsets[i] + (1 << v) - 1
    assert sum(1 << v for v in n_varss) <= 1 << total_vars
    if n_varss == [5, 5, 6, 7]:
        assert sum(1 << v for v in n_varss) == 1 << total_vars  # (no tail)


def test_message_layout_rejects():
    from binius_amd import BnError
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION
    from binius_amd._host import piop_message_layout

    with pytest.raises(BnError) as ei:
        piop_message_layout([4, 3])
    assert ei.value.code == BN_ERR_INPUT_VALIDATION and "CommittedsNotSorted" in str(ei.value)
    with pytest.raises(BnError) as ei:
        piop_message_layout([4, 48])
    assert ei.value.code == BN_ERR_INPUT_VALIDATION


@pytest.mark.parametrize("log_dim,log_inv_rate,log_batch,arities", [(9, 1, 3, [4, 4]), (9, 2, 0, [3, 2]), (8, 1, 2, []), (1, 0, 0, [])])
def test_commit_elems(log_dim, log_inv_rate, log_batch, arities):
    """The codeword is 2^(log_dim + log_batch + log_inv_rate) elements; the tree has one leaf per coset of 2^arity_0 elements (the
    whole message without arities) and 2 * (2 * leaves - 1) elements: two per node."""
    from binius_amd._host import FRIParams, piop_commit_elems

    code, tree = piop_commit_elems(FRIParams(log_dim, log_inv_rate, log_batch, arities, 3))
    assert code == 1 << (log_dim + log_batch + log_inv_rate)
    leaves = code >> (arities[0] if arities else log_dim + log_batch)
    assert tree == 2 * (2 * leaves - 1)


def test_commit_elems_rejects_a_bad_arity_sequence():
    from binius_amd import BnError
    from binius_amd._host import FRIParams, piop_commit_elems

    with pytest.raises(BnError):
        piop_commit_elems(FRIParams(4, 1, 0, [2, 2], 3))


def test_new_symbols_are_exported():
    from binius_amd import _ffi
    from binius_amd._host import host_lib

    L = _ffi.lib()
    for name in ("bn_merge_multilins", "bn_merge_counters"):
        assert hasattr(L, name) and name in _ffi.ABI_SYMBOLS
    H = host_lib()
    for name in ("bnh_piop_message_layout", "bnh_piop_commit_elems", "bnh_piop_commit", "bnh_piop_prove_committed", "bnh_piop_commit_last_ms", "bnh_piop_prove"):
        assert isinstance(getattr(H, name), C._CFuncPtr)
    header = open(os.path.join(ROOT, "include", "binius_amd.h")).read()
    t = int(re.search(r"#define BN_MERGE_TILE_LOG2 (\d+)", header).group(1))
    assert t in (5, 6) and t == _ffi.BN_MERGE_TILE_LOG2
