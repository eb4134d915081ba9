"""The live-transcript seam without a GPU (include/binius_amd_host.h, "Against a live transcript"): every new symbol is exported by
the built library, declared in the Rust shim's ffi.rs with the header's argument count, and bound by binius_amd._host; the
library's array-backed transcript (bnh_transcript_replay_*) is driven through its own function pointers; a `_live` entry point given a
null table, or a table without a callback it needs, is BN_ERR_INPUT_VALIDATION before it looks at anything else."""
import ctypes as C
import os
import re

import pytest

import transcript_ref as T
from test_rust_shim_ffi import _strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = ["bnh_batch_sumcheck_prove_live", "bnh_eqind_sumcheck_prove_live", "bnh_zerocheck_batch_prove_tower_live", "bnh_gkr_gpa_prove_live", "bnh_gkr_exp_prove_live",
        "bnh_flush_prodcheck_prove_live", "bnh_evalcheck_bivariate_prove_lc_live", "bnh_ring_switch_prove_live", "bnh_fri_prove_live",
        "bnh_piop_prove_committed_open_live"]
REPLAY = ["bnh_transcript_replay_new", "bnh_transcript_replay_table", "bnh_transcript_replay_written", "bnh_transcript_replay_events", "bnh_transcript_replay_free"]


def n_args(text, name, rust):
    m = re.search((r"fn %s\s*\((.*?)\)\s*(?:->\s*[^;]+)?;" if rust else r"\b%s\s*\(([^;{]*?)\)\s*;") % name, text, flags=re.S)
    assert m, "%s is not declared" % name
    return len([a for a in m.group(1).split(",") if a.strip()])


def param_names(text, name):
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S)
    assert m, "%s is not declared" % name
    return [re.findall(r"\w+", a)[-1] for a in m.group(1).split(",") if a.strip()]


SAMPLE_NAMES = {"batch_coeff", "batch_coeffs", "challenges", "zerocheck_challenges", "univariate_challenge", "sumcheck_challenges", "reduction_batch_coeff",
                "reduction_challenges", "gpa_challenges", "mixing_challenge", "permutation_challenges", "gpa_batch_coeffs", "gpa_sumcheck_challenges", "red_batch_coeffs",
                "red_challenges", "mixing_challenges", "n_mixing_challenges", "row_batch_challenges", "n_row_batch_challenges", "query_indices", "n_batch_coeffs",
                "n_challenges"}


def test_live_forms_drop_exactly_the_sample_arguments_name_by_name():
    """The positions in binius_amd._host.LIVE_FORMS against the header's parameter names: what is dropped from an array form is its
    sample arguments and nothing else, and the array form without them, with `transcript` inserted, is the _live form's parameter
    list in order."""
    from binius_amd._host import LIVE_FORMS

    header = _strip_comments(open(os.path.join(ROOT, "include", "binius_amd_host.h")).read())
    for array, (live, drop, at, splice) in LIVE_FORMS.items():
        names = param_names(header, array)
        if splice:
            names[splice[0]:splice[0]] = ["n_terms", "term_levels", "d_term_columns", "term_coeffs", "ml_offsets"][: len(splice[1])]
        assert {names[i] for i in drop} == SAMPLE_NAMES & set(names), "%s: the dropped positions are not its sample arguments" % array
        kept = [n for i, n in enumerate(names) if i not in drop]
        kept.insert(at, "transcript")
        assert kept == param_names(header, live), "%s -> %s: the parameter lists do not line up" % (array, live)


def test_every_new_symbol_is_exported_declared_and_bound():
    from binius_amd._host import LIVE_FORMS, host_lib

    L = host_lib()
    header = _strip_comments(open(os.path.join(ROOT, "include", "binius_amd_host.h")).read())
    rust = _strip_comments(open(os.path.join(ROOT, "crates", "binius_mi355x", "src", "ffi.rs")).read())
    assert sorted({v[0] for v in LIVE_FORMS.values()}) == sorted(LIVE)
    for name in LIVE + REPLAY:
        assert hasattr(L, name), "%s is not exported" % name
        assert n_args(header, name, False) == n_args(rust, name, True), "%s: ffi.rs and the header disagree on the number of arguments" % name
        assert len(getattr(L, name).argtypes) == n_args(header, name, False), "%s: the Python binding and the header disagree" % name
    # the table and the constants on both sides
    assert re.search(r"pub struct bnh_transcript\s*\{\s*pub user:.*?pub write:.*?pub sample:.*?pub sample_bits:", rust, flags=re.S)
    for const, val in (("BN_ERR_CALLBACK", 5), ("BNH_TR_MESSAGE", 0), ("BNH_TR_DECOMMITMENT", 1)):
        assert re.search(r"pub const %s: \w+ = %d;" % (const, val), rust), const
        assert re.search(r"\b%s = %d\b" % (const, val), open(os.path.join(ROOT, "include", "binius_amd.h" if const.startswith("BN_") else "binius_amd_host.h")).read()), const
    # a _live form is its array form without the sample arguments, plus the table
    for array, (live, drop, _at, splice) in LIVE_FORMS.items():
        extra = len(splice[1]) if splice else 0
        assert n_args(header, live, False) == n_args(header, array, False) + extra - len(drop) + 1, array


def test_replay_transcript_through_its_own_function_pointers():
    from binius_amd._host import F128, ReplayTranscript, from_f128

    samples = [3, 1 << 127, (0xABCD << 64) | 0x1234, 7, 9]
    r = ReplayTranscript(samples, [0xFFFF, 5, 1 << 40])
    user, write, sample, sample_bits = r.callbacks()
    out = (F128 * 3)()
    assert write(user, T.MESSAGE, b"commit", 6) == 0
    assert sample(user, out, 2) == 0 and [from_f128(out[i]) for i in range(2)] == samples[:2]
    assert write(user, T.MESSAGE, b"ab", 2) == 0 and write(user, T.MESSAGE, b"cde", 3) == 0  # two calls, one segment
    assert sample(user, out, 1) == 0 and from_f128(out[0]) == samples[2]
    assert sample(user, out, 1) == 0 and from_f128(out[0]) == samples[3]                      # two calls, one draw event
    assert write(user, T.DECOMMITMENT, b"terminate", 9) == 0
    bits = (C.c_uint64 * 2)()
    assert sample_bits(user, 4, 2, bits) == 0 and list(bits) == [0xF, 5]
    assert write(user, T.DECOMMITMENT, b"openings", 8) == 0
    assert sample(user, out, 2) != 0, "two samples asked for, one left"
    assert sample(user, out, 1) == 0 and from_f128(out[0]) == samples[4]
    assert sample(user, out, 1) != 0, "the samples have run out"
    assert sample_bits(user, 41, 1, bits) == 0 and bits[0] == 1 << 40
    assert sample_bits(user, 4, 1, bits) != 0, "the bit samples have run out"
    assert write(user, 2, b"x", 1) != 0, "an unknown channel"
    assert r.written(T.MESSAGE) == b"commitabcde" and r.written(T.DECOMMITMENT) == b"terminateopenings"
    assert r.events() == [("write_message", 6), ("sample", 2), ("write_message", 5), ("sample", 2), ("write_decommitment", 9), ("sample_bits", 2),
                          ("write_decommitment", 8), ("sample", 1), ("sample_bits", 1)]
    r.close()


def test_python_challenger_depends_on_every_message_byte():
    a, b = T.Hasher(), T.Hasher()
    assert a.sample() == b.sample() and a.sample() != T.Hasher().sample(), "the draw counter separates equal states"
    a.observe(b"round 0")
    b.observe(b"round 1")
    assert a.sample() != b.sample()
    assert T.Hasher().sample_bits(5) < 32
    sched = [("w", T.MESSAGE, 4), ("s", "x", 2), ("w", T.DECOMMITMENT, 3), ("w", T.MESSAGE, 2), ("b", 1), ("s", "y", 1)]
    assert T.merged(sched) == [("w", T.MESSAGE, 4), ("s", 2), ("w", T.DECOMMITMENT, 3), ("w", T.MESSAGE, 2), ("b", 1), ("s", 1)]
    roles, idx = T.replay(sched, b"abcdef", bits=7)
    again, _ = T.replay(sched, b"abcdeg", bits=7)
    assert roles["x"] == again["x"] and roles["y"] != again["y"] and len(idx) == 1 and idx[0] < 128
    assert T.roles_of(sched, [1, 2, 3]) == {"x": [1, 2], "y": [3]}


@pytest.mark.parametrize("name", LIVE)
def test_live_entry_points_reject_a_null_table(name):
    """A null table is rejected before anything else is read: every other argument is null too."""
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION
    from binius_amd._host import host_lib

    L = host_lib()
    fn = getattr(L, name)
    args = [None if t is not C.c_uint32 and t is not C.c_uint64 else 0 for t in fn.argtypes]
    assert fn(*args) == BN_ERR_INPUT_VALIDATION
    assert "transcript" in L.bnh_last_error().decode()


def test_a_table_without_a_callback_the_entry_point_needs_is_rejected():
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION
    from binius_amd._host import BnhTranscript, ReplayTranscript, host_lib

    L = host_lib()
    r = ReplayTranscript([1, 2, 3], [1])
    full = C.cast(r.table(), C.POINTER(BnhTranscript)).contents
    fn = L.bnh_fri_prove_live
    where = [i for i, t in enumerate(fn.argtypes) if t is C.c_void_p][3]  # ctx, d_message, d_scratch, transcript
    assert len(fn.argtypes) == 16 and where == 10
    for missing, n_test_queries, rejected in (("write", 0, True), ("sample", 0, True), ("sample_bits", 2, True), ("sample_bits", 0, False)):
        table = BnhTranscript(full.user, full.write, full.sample, full.sample_bits)
        setattr(table, missing, type(getattr(table, missing))())
        args = [None if t is not C.c_uint32 and t is not C.c_uint64 else 0 for t in fn.argtypes]
        args[6], args[where] = n_test_queries, C.addressof(table)
        assert fn(*args) == BN_ERR_INPUT_VALIDATION  # (the null context, if the table passed)
        assert ("transcript" in L.bnh_last_error().decode()) == rejected, missing
    r.close()
