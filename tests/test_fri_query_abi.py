"""CPU-side checks of the FRI query phase's boundary: bn_fri_query_proof_elems (a pure host function) against the layout computed in
Python from the protocol for every shape of the device tests, its rejections, the Python FRIParams arithmetic against the restated
one, the bn_fri_oracle struct on both sides of the FFI, and the new entry points of the host library.  No device."""
import ctypes
import os

import pytest

import fri_verify_ref as fv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g

    g.build()
    import binius_amd._ffi as f

    return f


def host_params(p):
    from binius_amd._host import FRIParams

    return FRIParams(p.log_dim, p.log_inv_rate, p.log_batch_size, list(p.fold_arities), p.n_test_queries)


@pytest.mark.parametrize("p", [p for p, _ in fv.SHAPES], ids=fv.SHAPE_IDS)
def test_proof_elems_equal_the_layout_of_the_protocol(ffi, p):
    hp = host_params(p)
    assert hp.index_bits() == p.index_bits() and hp.optimal_layer_depths() == p.optimal_layer_depths() and hp.terminate_elems() == p.terminate_len()
    oracles = [(None, None) + o for o in hp.query_oracles()]
    assert len(oracles) == p.n_oracles()
    assert ffi.fri_query_proof_elems(oracles, p.terminate_len(), p.n_test_queries) == p.layout()
    assert hp.advice_elems() == p.layout()
    # no query: the header alone; no oracle: the terminate codeword alone
    header = p.layout()[0]
    assert ffi.fri_query_proof_elems(oracles, p.terminate_len(), 0) == (header, p.layout()[1], header)
    assert ffi.fri_query_proof_elems([], p.terminate_len(), 7) == (p.terminate_len(), 0, p.terminate_len())


def test_layout_of_a_hand_computed_case(ffi):
    """log_len 9, arities (3, 2, 1), three queries: depths min(2, .) = 2, 2, 2 over trees of 6, 4 and 3 levels"""
    p = fv.SHAPES[0][0]
    assert p.optimal_layer_depths() == [2, 2, 2] and p.terminate_len() == 1 << 3
    assert p.layout() == (8 + 3 * 8, (8 + 2 * 4) + (4 + 2 * 2) + (2 + 2 * 1), 32 + 3 * 28)


def test_proof_elems_rejections(ffi):
    def rejected(oracles, terminate_elems=8, n_queries=3, text=None):
        with pytest.raises(ffi.BnError) as e:
            ffi.fri_query_proof_elems(oracles, terminate_elems, n_queries)
        assert e.value.code == ffi.BN_ERR_INPUT_VALIDATION
        if text:
            assert text in str(e.value)

    ok = (None, None, 6, 3, 2, 0)
    assert ffi.fri_query_proof_elems([ok] * ffi.FRI_QUERY_MAX_ORACLES, 8, 1)[1] == 32 * (8 + 2 * 4)
    rejected([ok] * (ffi.FRI_QUERY_MAX_ORACLES + 1), text="BN_FRI_QUERY_MAX_ORACLES")
    rejected([(None, None, 6, 3, 7, 0)], text="IncorrectLayerDepth")
    rejected([(None, None, 40, 8, 2, 0)], text="out of range")
    rejected([ok], terminate_elems=(1 << 26) + 1, text="too many elements")
    rejected([ok], n_queries=1 << 22, text="too many elements")  # 2^22 records of 16 elements
    rejected([(None, None, 27, 3, 27, 0)], text="too many elements")  # a layer of 2^27 digests


def test_fri_oracle_struct_matches_on_both_sides_of_the_ffi(ffi):
    from test_rust_shim_ffi import parse_header, parse_rust

    h, r = parse_header()[1], parse_rust()[1]
    assert h["bn_fri_oracle"] == r["bn_fri_oracle"]
    assert [n for n, _ in h["bn_fri_oracle"]] == [n for n, _ in ffi.FriOracle._fields_]
    assert ctypes.sizeof(ffi.FriOracle) == 32
    hdr = open(os.path.join(ROOT, "include", "binius_amd.h")).read()
    assert "#define BN_FRI_QUERY_MAX_ORACLES %d" % ffi.FRI_QUERY_MAX_ORACLES in hdr


def test_host_library_exports_the_query_phase(ffi):
    from binius_amd._host import host_lib

    L = host_lib()
    for name in ("bnh_fri_prove", "bnh_piop_prove_committed_open", "bnh_fri_commit_fold", "bnh_piop_prove_committed"):
        assert hasattr(L, name), name
    assert len(L.bnh_piop_prove_committed_open.argtypes) == len(L.bnh_piop_prove_committed.argtypes) + 4
    assert len(L.bnh_fri_prove.argtypes) == len(L.bnh_fri_commit_fold.argtypes) + 3  # terminate_out gone, four arguments added
