"""ctypes binding of libbinius_amd_host.so -- the compiled C++ host mirror
(binius_amd/host/{compute_layer,sumcheck}.hpp): a whole BivariateSumcheckProver run behind one C
call, i.e. the prover loop driven at compiled-host speed over the same C ABI."""
import ctypes as C
import os
import threading

from ._ffi import BN_ERR_CALLBACK, BN_ERR_INPUT_VALIDATION, F128, BnError, _f128_array, from_f128, lib, to_f128

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libbinius_amd_host.so")
_lib = None

REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(F128))

# bnh_transcript (include/binius_amd_host.h): the caller's Fiat-Shamir transcript as three callbacks
TR_MESSAGE, TR_DECOMMITMENT = 0, 1
TR_EVENT_KINDS = ("write_message", "write_decommitment", "sample", "sample_bits")
TR_WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64)
TR_SAMPLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(F128), C.c_uint32)
TR_SAMPLE_BITS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64))


class BnhTranscript(C.Structure):
    _fields_ = [("user", C.c_void_p), ("write", TR_WRITE_FN), ("sample", TR_SAMPLE_FN), ("sample_bits", TR_SAMPLE_BITS_FN)]


# array entry point -> (its _live form, the positions of its sample arguments, where the transcript stands once they are gone,
# arguments to splice in first as (position, values): the entry point whose _live form is the superset's).  The positions are checked
# against the parameter NAMES of include/binius_amd_host.h by tests/test_transcript_abi.py: dropping the named sample arguments of
# the array form and inserting `transcript` must give the _live form's parameter list, name by name.
_EVALCHECK_NO_TERMS = (5, (0, None, None, None, None))
LIVE_FORMS = {
    "bnh_batch_sumcheck_prove": ("bnh_batch_sumcheck_prove_live", (8, 9), 8, None),
    "bnh_eqind_sumcheck_prove": ("bnh_eqind_sumcheck_prove_live", (14, 15), 14, None),
    "bnh_zerocheck_batch_prove_tower": ("bnh_zerocheck_batch_prove_tower_live", (13, 14, 15, 16, 17, 18), 13, None),
    "bnh_gkr_gpa_prove": ("bnh_gkr_gpa_prove_live", (8, 9, 10), 8, None),
    "bnh_gkr_exp_prove": ("bnh_gkr_exp_prove_live", (14, 15), 14, None),
    "bnh_flush_prodcheck_prove": ("bnh_flush_prodcheck_prove_live", (18, 19, 23, 24, 25, 26, 27), 21, None),
    "bnh_evalcheck_bivariate_prove": ("bnh_evalcheck_bivariate_prove_lc_live", (16, 17), 16, _EVALCHECK_NO_TERMS),
    "bnh_evalcheck_bivariate_prove_lc": ("bnh_evalcheck_bivariate_prove_lc_live", (16, 17), 16, None),
    "bnh_ring_switch_prove": ("bnh_ring_switch_prove_live", (12, 13, 14, 15), 12, None),
    "bnh_fri_prove": ("bnh_fri_prove_live", (10, 12), 10, None),
    "bnh_piop_prove_committed_open": ("bnh_piop_prove_committed_open_live", (20, 21, 22, 23, 34), 20, None),
}
# bnh_zerocheck_batch_prove has no _live form of its own (the tower form is the superset, with its own scratch formula): a plan made
# with tower=False is refused inside proving() rather than redirected
NO_LIVE_FORM = {"bnh_zerocheck_batch_prove": "bnh_zerocheck_batch_prove has no _live form: make the ZerocheckBatchPlan with tower=True (and the tower scratch size)"}


class _LiveState(threading.local):
    """the transcripts of the proving() scopes in progress on THIS thread (innermost last)"""

    def __init__(self):
        self.stack = []


_live = _LiveState()


class _LiveEntries:
    """host_lib() as a plan's run() sees it inside Transcript.prove(): every array entry point that has a _live form calls that form
    with the sample arguments dropped and the transcript's table in their place; everything else is the library's."""

    def __init__(self, L, table):
        self._L, self._table = L, table

    def __getattr__(self, name):
        if name in NO_LIVE_FORM:
            raise BnError(BN_ERR_INPUT_VALIDATION, NO_LIVE_FORM[name])
        if name not in LIVE_FORMS:
            return getattr(self._L, name)
        live, drop, at, splice = LIVE_FORMS[name]
        fn, table = getattr(self._L, live), self._table

        def call(*args):
            args = list(args)
            if splice is not None:
                args[splice[0]:splice[0]] = list(splice[1])
            args = [a for i, a in enumerate(args) if i not in drop]
            args.insert(at, table)
            return fn(*args)

        return call


class _TranscriptBase:
    def table(self):
        """the `const bnh_transcript *` to hand to a _live entry point"""
        raise NotImplementedError

    def proving(self):
        """Context manager: inside it, every plan of this module whose entry point has a _live form (LIVE_FORMS) runs against this
        transcript.  The plan's own sample arrays are not read (hand it placeholders of the right lengths); its output arrays are
        filled as its array form fills them.  A Python exception raised inside a callback ends the proof (the callback returns
        non-zero, the entry point BN_ERR_CALLBACK) and is re-raised on the way out, after the call has come back: it never unwinds
        through the library."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            _live.stack.append(_LiveEntries(_plain_host_lib(), self.table()))
            try:
                yield self
            except BnError as e:
                pending = self._take_exception()
                if e.code == BN_ERR_CALLBACK and pending is not None:
                    raise pending from None
                raise
            finally:
                _live.stack.pop()

        return scope()

    def prove(self, plan):
        """plan.run() inside proving()"""
        with self.proving():
            return plan.run()

    def _take_exception(self):
        return None


class TranscriptAbort(Exception):
    """raised inside a Transcript callback: the callback returns non-zero and nothing is re-raised -- the entry point's
    BN_ERR_CALLBACK surfaces as BnError"""


class Transcript(_TranscriptBase):
    """A Fiat-Shamir transcript in Python behind the bnh_transcript table.  Subclasses implement
        write(channel, data)        data: bytes in transcript byte order; channel TR_MESSAGE is observed, TR_DECOMMITMENT is not
        sample(n) -> n ints         n x transcript.sample() of B128
        sample_bits(bits, n) -> n ints
    The callbacks run on the calling thread inside the entry point and must not call the library on the same context."""

    def __init__(self):
        self._exc = None

        def guard(body):
            def cb(*args):
                try:
                    body(*args)
                    return 0
                except TranscriptAbort:
                    return 1
                except BaseException as e:  # noqa: BLE001 -- nothing may unwind through the C++ frames above this callback
                    self._exc = e
                    return 1
            return cb

        def on_write(_user, channel, data, n):
            self.write(int(channel), C.string_at(data, n))

        def on_sample(_user, out, n):
            vals = list(self.sample(int(n)))
            assert len(vals) == n
            for i, v in enumerate(vals):
                out[i] = to_f128(v)

        def on_sample_bits(_user, bits, n, out):
            vals = list(self.sample_bits(int(bits), int(n)))
            assert len(vals) == n
            for i, v in enumerate(vals):
                out[i] = int(v)

        self._fns = (TR_WRITE_FN(guard(on_write)), TR_SAMPLE_FN(guard(on_sample)), TR_SAMPLE_BITS_FN(guard(on_sample_bits)))
        self._table = BnhTranscript(None, *self._fns)

    def table(self):
        return C.addressof(self._table)

    def _take_exception(self):
        e, self._exc = self._exc, None
        return e

    def write(self, channel, data):
        raise NotImplementedError

    def sample(self, n):
        raise NotImplementedError

    def sample_bits(self, bits, n):
        raise NotImplementedError


class ReplayTranscript(_TranscriptBase):
    """The library's array-backed transcript (bnh_transcript_replay_*): serves `samples` and `bit_samples` in order, fails when they
    run out, records every write.  Host code only; needs no context."""

    def __init__(self, samples, bit_samples=()):
        samples, bit_samples = list(samples), list(bit_samples)
        bits = (C.c_uint64 * max(1, len(bit_samples)))(*bit_samples)
        self._h = C.c_void_p()
        _host_check(host_lib().bnh_transcript_replay_new(_f128_array(samples), len(samples), bits, len(bit_samples), C.byref(self._h)))

    def table(self):
        return host_lib().bnh_transcript_replay_table(self._h)

    def callbacks(self):
        """the table itself: (user, write, sample, sample_bits) as ctypes callables"""
        t = C.cast(self.table(), C.POINTER(BnhTranscript)).contents
        return t.user, t.write, t.sample, t.sample_bits

    def written(self, channel):
        n = C.c_uint64()
        host_lib().bnh_transcript_replay_written(self._h, channel, None, 0, C.byref(n))  # (the length; fails when it is not zero)
        buf = (C.c_uint8 * max(1, n.value))()
        _host_check(host_lib().bnh_transcript_replay_written(self._h, channel, buf, n.value, C.byref(n)))
        return bytes(buf[: n.value])

    def events(self):
        """[(kind, count)]: kind in TR_EVENT_KINDS, count in bytes (writes) or samples (draws); neighbours of one kind merged"""
        n = C.c_uint64()
        host_lib().bnh_transcript_replay_events(self._h, None, None, 0, C.byref(n))
        kinds, counts = (C.c_uint32 * max(1, n.value))(), (C.c_uint64 * max(1, n.value))()
        _host_check(host_lib().bnh_transcript_replay_events(self._h, kinds, counts, n.value, C.byref(n)))
        return [(TR_EVENT_KINDS[kinds[i]], int(counts[i])) for i in range(n.value)]

    def close(self):
        if self._h:
            host_lib().bnh_transcript_replay_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


def host_lib():
    """the library -- or, inside Transcript.proving(), its entry points redirected to their _live forms"""
    return _live.stack[-1] if _live.stack else _plain_host_lib()


def _plain_host_lib():
    global _lib
    if _lib is None:
        lib()  # libbinius_amd.so first (dependency, resolved through rpath as well)
        if not os.path.exists(_SO):
            raise ImportError("binius_amd: %s is missing -- run __graft_entry__.build()" % _SO)
        L = C.CDLL(_SO)
        L.bnh_last_error.restype = C.c_char_p
        L.bnh_bivariate_sumcheck_prove.restype = C.c_int
        L.bnh_bivariate_sumcheck_prove.argtypes = [
            C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_uint32,
            C.POINTER(C.c_uint32), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128),
            REDUCE_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
        ]
        L.bnh_shm_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.bnh_shm_close.argtypes = [C.c_void_p]
        L.bnh_shm_allgather.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint64)]
        L.bnh_bivariate_mlecheck_prove.restype = C.c_int
        L.bnh_bivariate_mlecheck_prove.argtypes = [
            C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(F128), C.c_void_p, C.c_uint64,
            C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128),
        ]
        L.bnh_mlecheck_new.restype = C.c_int
        L.bnh_mlecheck_new.argtypes = [
            C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(F128), C.c_void_p, C.c_uint64,
            C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(F128), C.POINTER(C.c_void_p),
        ]
        L.bnh_mlecheck_execute.argtypes = [C.c_void_p, C.POINTER(F128), C.POINTER(F128)]
        L.bnh_mlecheck_fold.argtypes = [C.c_void_p, C.POINTER(F128)]
        L.bnh_mlecheck_finish.argtypes = [C.c_void_p, C.POINTER(F128)]
        L.bnh_mlecheck_free.argtypes = [C.c_void_p]
        L.bnh_mlecheck_free.restype = None
        L.bnh_mlecheck_last_mode.restype = C.c_int
        L.bnh_fri_commit_fold.restype = C.c_int
        L.bnh_fri_commit_fold.argtypes = [
            C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
            C.c_uint64, C.POINTER(F128), C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
        ]
        L.bnh_fri_prove.restype = C.c_int
        L.bnh_fri_prove.argtypes = [
            C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
            C.c_uint64, C.POINTER(F128), C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double),
        ]
        L.bnh_fri_query_phase_bench.restype = C.c_int
        L.bnh_fri_query_phase_bench.argtypes = [
            C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
            C.c_uint64, C.POINTER(F128), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
            C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
        ]
        L.bnh_batch_sumcheck_prove.restype = C.c_int
        L.bnh_batch_sumcheck_prove.argtypes = [
            C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(F128), C.c_void_p, C.c_uint64,
            C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128),
        ]
        L.bnh_piop_prove.restype = C.c_int
        L.bnh_piop_prove.argtypes = [
            C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p),
            C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(F128), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
            C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(F128), C.c_uint32, C.POINTER(F128), C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32,
            C.POINTER(C.c_uint32), C.POINTER(F128), C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double),
        ]
        U32P_, VPP_, FP_ = C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(F128)
        L.bnh_piop_message_layout.restype = C.c_int
        L.bnh_piop_message_layout.argtypes = [C.c_uint32, U32P_, C.POINTER(C.c_uint64), U32P_]
        L.bnh_piop_commit_elems.restype = C.c_int
        L.bnh_piop_commit_elems.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, U32P_, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.bnh_piop_commit.restype = C.c_int
        L.bnh_piop_commit.argtypes = [C.c_void_p, C.c_uint32, U32P_, VPP_, C.c_uint32, C.c_uint32, C.c_uint32, U32P_, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_double)]
        L.bnh_piop_commit_last_ms.restype = C.c_double
        L.bnh_piop_commit_last_ms.argtypes = []
        L.bnh_piop_prove_committed.restype = C.c_int
        L.bnh_piop_prove_committed.argtypes = [
            C.c_void_p, C.c_uint32, U32P_, VPP_, C.c_uint32, U32P_, VPP_, C.c_uint32, U32P_, FP_, C.c_uint32, C.c_uint32, C.c_uint32, U32P_, C.c_uint32, C.c_uint32,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, FP_, C.c_uint32, FP_, C.c_uint32, U32P_, C.c_uint32, U32P_, FP_, C.c_uint64, C.POINTER(C.c_uint64),
            C.c_void_p, C.c_uint32, U32P_, C.POINTER(C.c_double),
        ]
        L.bnh_piop_prove_committed_open.restype = C.c_int
        L.bnh_piop_prove_committed_open.argtypes = L.bnh_piop_prove_committed.argtypes + [C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.bnh_eqind_sumcheck_prove.restype = C.c_int
        L.bnh_eqind_sumcheck_prove.argtypes = [
            C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32),
            C.POINTER(C.c_uint32), C.POINTER(F128), C.POINTER(F128), C.c_void_p, C.c_uint64, C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128),
        ]
        L.bnh_gkr_gpa_prove.restype = C.c_int
        L.bnh_gkr_gpa_prove.argtypes = [
            C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64,
            C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128), C.POINTER(F128),
            C.POINTER(C.c_double),
        ]
        U32P, VPP, FP = C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(F128)
        L.bnh_gkr_exp_prove.restype = C.c_int
        L.bnh_gkr_exp_prove.argtypes = [
            C.c_void_p, C.c_uint32, U32P, U32P, VPP, FP, VPP, VPP, C.c_uint32, U32P, FP, FP, C.c_void_p, C.c_uint64, FP, FP,
            U32P, U32P, U32P, FP, U32P, U32P, FP, U32P, U32P, FP, FP, C.POINTER(C.c_double),
        ]
        U64P, DP = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
        L.bnh_flush_prodcheck_prove.restype = C.c_int
        L.bnh_flush_prodcheck_prove.argtypes = [
            C.c_void_p, C.c_uint32, U32P, U32P, U32P, U32P, VPP, U32P, U32P, U32P, VPP, U32P, FP, C.c_uint32, U32P, VPP, U32P, U32P, FP, FP, C.c_uint32,
            C.c_void_p, C.c_uint64, FP, FP, FP, FP, FP, U64P, FP, FP, FP, FP, FP, U32P, U32P, U32P, FP, FP, U32P, U32P, DP,
        ]
        L.bnh_evalcheck_bivariate_prove.restype = C.c_int
        L.bnh_evalcheck_bivariate_prove.argtypes = [C.c_void_p, C.c_uint32, U32P, U32P, VPP, FP, C.c_uint32, U32P, FP, C.c_void_p, C.c_uint64, FP, FP, FP, FP]
        L.bnh_evalcheck_bivariate_prove_lc.restype = C.c_int
        L.bnh_evalcheck_bivariate_prove_lc.argtypes = [C.c_void_p, C.c_uint32, U32P, U32P, VPP, C.c_uint32, U32P, VPP, FP, FP, FP, C.c_uint32, U32P, FP, C.c_void_p,
                                                       C.c_uint64, FP, FP, FP, FP]
        L.bnh_evalcheck_evaluate_scratch_elems.restype = C.c_uint64
        L.bnh_evalcheck_evaluate_scratch_elems.argtypes = [C.c_uint32, U32P, C.c_uint32]
        L.bnh_evalcheck_evaluate.restype = C.c_int
        L.bnh_evalcheck_evaluate.argtypes = [C.c_void_p, C.c_uint32, U32P, VPP, FP, C.c_uint32, C.c_void_p, C.c_uint64, FP, DP]
        L.bnh_ring_switch_scratch_elems.restype = C.c_uint64
        L.bnh_ring_switch_scratch_elems.argtypes = [C.c_uint32, U32P, C.c_uint32, U32P]
        L.bnh_ring_switch_prove.restype = C.c_int
        L.bnh_ring_switch_prove.argtypes = [C.c_void_p, C.c_uint32, VPP, U32P, FP, C.c_uint32, C.c_uint32, U32P, C.c_uint32, U32P, C.c_uint32, U32P, FP, C.c_uint32, FP,
                                            C.c_uint32, C.c_void_p, C.c_uint64, FP, FP, VPP, DP]
        L.bnh_zerocheck_batch_scratch_elems.restype = C.c_uint64
        L.bnh_zerocheck_batch_scratch_elems.argtypes = [C.c_uint32, C.c_uint32, U32P, U32P]
        L.bnh_zerocheck_batch_prove.restype = C.c_int
        L.bnh_zerocheck_batch_prove.argtypes = [
            C.c_void_p, C.c_uint32, C.c_uint32, U32P, U32P, VPP, U32P, U32P, C.c_void_p, U32P, C.c_void_p, U32P, U32P, FP, FP, FP, FP, FP, FP, C.c_void_p, C.c_uint64,
            FP, FP, FP, FP, FP, FP, FP, FP, DP, U64P,
        ]
        L.bnh_zerocheck_batch_scratch_elems_tower.restype = C.c_uint64
        L.bnh_zerocheck_batch_scratch_elems_tower.argtypes = [C.c_uint32, C.c_uint32, U32P, U32P, U32P]
        L.bnh_zerocheck_batch_prove_tower.restype = C.c_int
        L.bnh_zerocheck_batch_prove_tower.argtypes = L.bnh_zerocheck_batch_prove.argtypes
        L.bnh_witness_derive_scratch_elems.restype = C.c_uint64
        L.bnh_witness_derive_scratch_elems.argtypes = [C.c_uint32, U32P, U64P, U32P, FP, C.c_uint32, FP]
        L.bnh_witness_derive.restype = C.c_int
        L.bnh_witness_derive.argtypes = [C.c_void_p, C.c_uint32, U32P, U64P, VPP, U32P, FP, C.c_uint32, FP, C.c_void_p, C.c_uint64, VPP, U32P, U32P, U32P, U32P]
        L.bnh_witness_build_scratch_elems.restype = C.c_uint64
        L.bnh_witness_build_scratch_elems.argtypes = L.bnh_witness_derive_scratch_elems.argtypes
        L.bnh_witness_build.restype = C.c_int
        L.bnh_witness_build.argtypes = L.bnh_witness_derive.argtypes
        from ._ffi import Step

        expr_args = [C.POINTER(Step), U32P, U32P, U32P, C.c_uint32]
        L.bnh_witness_compute_scratch_elems.restype = C.c_uint64
        L.bnh_witness_compute_scratch_elems.argtypes = L.bnh_witness_derive_scratch_elems.argtypes + expr_args
        L.bnh_witness_compute.restype = C.c_int
        L.bnh_witness_compute.argtypes = L.bnh_witness_derive.argtypes + expr_args
        L.bnh_witness_compute_batched.restype = C.c_int
        L.bnh_witness_compute_batched.argtypes = L.bnh_witness_compute.argtypes
        # the _live forms: the array form's arguments without the samples, the transcript's table where LIVE_FORMS says
        for name, (live, drop, at, _splice) in LIVE_FORMS.items():
            if name == "bnh_evalcheck_bivariate_prove":
                continue  # (its _live form is the superset's, declared from it)
            types = [t for i, t in enumerate(getattr(L, name).argtypes) if i not in drop]
            types.insert(at, C.c_void_p)
            getattr(L, live).restype = C.c_int
            getattr(L, live).argtypes = types
        L.bnh_transcript_replay_new.restype = C.c_int
        L.bnh_transcript_replay_new.argtypes = [FP, C.c_uint64, U64P, C.c_uint64, C.POINTER(C.c_void_p)]
        L.bnh_transcript_replay_table.restype = C.c_void_p
        L.bnh_transcript_replay_table.argtypes = [C.c_void_p]
        L.bnh_transcript_replay_written.restype = C.c_int
        L.bnh_transcript_replay_written.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, U64P]
        L.bnh_transcript_replay_events.restype = C.c_int
        L.bnh_transcript_replay_events.argtypes = [C.c_void_p, U32P, U64P, C.c_uint64, U64P]
        L.bnh_transcript_replay_free.restype = None
        L.bnh_transcript_replay_free.argtypes = [C.c_void_p]
        L.bnh_rccl_open.argtypes = [C.c_char_p]
        L.bnh_rccl_unique_id.argtypes = [C.c_void_p]
        L.bnh_rccl_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.bnh_rccl_destroy.argtypes = [C.c_void_p]
        _lib = L
    return _lib


class SumcheckPlan:
    """Pre-marshalled arguments of one prove so repeated runs have no per-call Python work."""

    def __init__(self, hal, n_vars, multilins, scratch, comps, sums, batch_coeff, challenges, reduce=None, d_partial=0,
                 rccl_comm=None, world=1, d_gathered=0, shm=None, tail_rounds=False, peer=False):
        """tail_rounds (shm or RCCL exchange): `challenges` holds n_vars + log2(world) values and the run
        also does the residual rounds; round_coeffs() then has n_vars + log2(world) entries.
        peer: the ranks' partial round evaluations are XORed on the devices inside the kernels' finalize step (the
        context must hold a connected PeerExchange); `shm` then only rebuilds the residual instance."""
        self.peer = bool(peer)
        self.hal = hal
        self.n_vars = n_vars
        self.m = len(multilins)
        self.ptrs = (C.c_void_p * self.m)(*[s.ptr for s in multilins])
        self.scratch = scratch
        flat = [i for pair in comps for i in pair]
        self.n_comps = len(comps)
        self.comps = (C.c_uint32 * max(1, len(flat)))(*flat)
        self.sums = _f128_array(list(sums))
        self.bc = to_f128(batch_coeff)
        self.ch = _f128_array(list(challenges))
        self.tail_rounds = bool(tail_rounds and (shm is not None or rccl_comm is not None) and world > 1)
        self.n_rounds = n_vars + ((world.bit_length() - 1) if self.tail_rounds else 0)
        assert len(challenges) >= self.n_rounds
        self.coeffs = (F128 * (3 * self.n_rounds))()
        self.final = (F128 * self.m)()
        self.reduce = REDUCE_FN(reduce) if reduce is not None else C.cast(None, REDUCE_FN)
        self.d_partial = d_partial
        self.rccl_comm, self.world, self.d_gathered = rccl_comm, world, d_gathered
        self.shm = shm

    def run(self):
        rc = host_lib().bnh_bivariate_sumcheck_prove(
            self.hal._h, self.n_vars, self.m, self.ptrs, self.scratch.ptr, self.scratch.len, self.n_comps, self.comps,
            self.sums, C.byref(self.bc), self.ch, self.coeffs, self.final, self.reduce, None, self.d_partial,
            self.rccl_comm, self.world, self.d_gathered, self.shm, (1 if self.tail_rounds else 0) | (2 if self.peer else 0),
        )
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def round_coeffs(self):
        return [[from_f128(self.coeffs[3 * r + i]) for i in range(3)] for r in range(self.n_rounds)]

    def final_evals(self):
        return [from_f128(self.final[j]) for j in range(self.m)]


class MlecheckPlan:
    """One BivariateMLEcheckProver run of the compiled host mirror (bnh_bivariate_mlecheck_prove)."""

    def __init__(self, hal, n_vars, multilins, eq_ind, eq_ind_challenges, scratch, comps, sums, batch_coeff, challenges):
        self.hal, self.n_vars, self.m = hal, n_vars, len(multilins)
        self.ptrs = (C.c_void_p * self.m)(*[s.ptr for s in multilins])
        self.eq_ind, self.scratch = eq_ind, scratch
        self.eqc = _f128_array(list(eq_ind_challenges))
        flat = [i for pair in comps for i in pair]
        self.n_comps = len(comps)
        self.comps = (C.c_uint32 * max(1, len(flat)))(*flat)
        self.sums = _f128_array(list(sums))
        self.bc = to_f128(batch_coeff)
        self.ch = _f128_array(list(challenges))
        self.coeffs = (F128 * (4 * n_vars))()
        self.final = (F128 * (self.m + 1))()

    def run(self):
        rc = host_lib().bnh_bivariate_mlecheck_prove(
            self.hal._h, self.n_vars, self.m, self.ptrs, self.eq_ind.ptr, self.eqc, self.scratch.ptr, self.scratch.len,
            self.n_comps, self.comps, self.sums, C.byref(self.bc), self.ch, self.coeffs, self.final,
        )
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def last_mode(self):
        """1: WeightedMLEcheckProver ran; 0: the literal BivariateMLEcheckProver mirror."""
        return host_lib().bnh_mlecheck_last_mode()

    def round_coeffs(self):
        return [[from_f128(self.coeffs[4 * r + i]) for i in range(4)] for r in range(self.n_vars)]

    def final_evals(self):
        return [from_f128(self.final[j]) for j in range(self.m + 1)]


class MlecheckProver:
    """The MLE-check prover behind its handle (bnh_mlecheck_*): SumcheckProver::{execute, fold, finish} one call each,
    challenges supplied round by round."""

    def __init__(self, hal, n_vars, multilins, eq_ind, eq_ind_challenges, scratch, comps, sums):
        self.m = len(multilins)
        ptrs = (C.c_void_p * self.m)(*[s.ptr for s in multilins])
        flat = [i for pair in comps for i in pair]
        cc = (C.c_uint32 * max(1, len(flat)))(*flat)
        self._h = C.c_void_p()
        self._keep = (multilins, eq_ind, scratch)
        rc = host_lib().bnh_mlecheck_new(hal._h, n_vars, self.m, ptrs, eq_ind.ptr, _f128_array(list(eq_ind_challenges)), scratch.ptr, scratch.len,
                                         len(comps), cc, _f128_array(list(sums)), C.byref(self._h))
        self._check(rc)
        self.mode = host_lib().bnh_mlecheck_last_mode()

    @staticmethod
    def _check(rc):
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def execute(self, batch_coeff):
        bc, out = to_f128(batch_coeff), (F128 * 4)()
        self._check(host_lib().bnh_mlecheck_execute(self._h, C.byref(bc), out))
        return [from_f128(out[i]) for i in range(4)]

    def fold(self, challenge):
        z = to_f128(challenge)
        self._check(host_lib().bnh_mlecheck_fold(self._h, C.byref(z)))

    def finish(self):
        out = (F128 * (self.m + 1))()
        self._check(host_lib().bnh_mlecheck_finish(self._h, out))
        return [from_f128(out[j]) for j in range(self.m + 1)]

    def close(self):
        if self._h:
            host_lib().bnh_mlecheck_free(self._h)
            self._h = C.c_void_p()


class FRIParams:
    """Parameters of a FRI instance as bnh_fri_commit_fold takes them (the arithmetic of FRIParams,
    crates/core/src/protocols/fri/common.rs:84-190; validation happens in the C++ mirror, binius_amd/host/fri.hpp)."""

    def __init__(self, log_dim, log_inv_rate, log_batch_size, fold_arities, n_test_queries):
        self.log_dim, self.log_inv_rate, self.log_batch_size = log_dim, log_inv_rate, log_batch_size
        self.fold_arities, self.n_test_queries = list(fold_arities), n_test_queries

    def rs_log_len(self):
        return self.log_dim + self.log_inv_rate

    def n_fold_rounds(self):
        return self.log_dim + self.log_batch_size

    def n_final_challenges(self):
        return self.n_fold_rounds() - sum(self.fold_arities)

    def log_len(self):
        return self.rs_log_len() + self.log_batch_size

    def index_bits(self):
        return self.log_len() - self.fold_arities[0] if self.fold_arities else 0

    def optimal_layer_depths(self):
        """vcs_optimal_layers_depths_iter (common.rs:174-190) with optimal_verify_layer (merkle_tree/scheme.rs:47-49)"""
        cap, log_n_cosets, out = max(0, self.n_test_queries - 1).bit_length(), self.log_len(), []
        for arity in self.fold_arities:
            log_n_cosets -= arity
            out.append(min(cap, log_n_cosets))
        return out

    def query_oracles(self):
        """(log_n_cosets, log_coset_size, layer_depth, index_shift) of every oracle a query opens, as bn_fri_oracle takes them"""
        out, log_n_cosets, shift = [], self.log_len(), 0
        for i, (arity, depth) in enumerate(zip(self.fold_arities, self.optimal_layer_depths())):
            log_n_cosets -= arity
            shift += arity if i else 0
            out.append((log_n_cosets, arity, depth, shift))
        return out

    def terminate_elems(self):
        return 1 << (self.log_inv_rate + self.n_final_challenges())

    def advice_elems(self):
        """(header, per-query record, total) of the decommitment of finish_proof in field elements (bn_fri_query_proof_elems)"""
        from ._ffi import fri_query_proof_elems

        return fri_query_proof_elems([(None, None) + o for o in self.query_oracles()], self.terminate_elems(), self.n_test_queries)


class FriPlan:
    """FRI commit phase + every fold round + finalize through the compiled C++ mirror (bnh_fri_commit_fold,
    binius_amd/host/fri.hpp).  `scratch` takes the codeword, the folded codewords and the Merkle trees."""

    def __init__(self, hal, params, message, scratch, challenges):
        import numpy as np

        self.hal, self.p, self.message, self.scratch = hal, params, message, scratch
        self.arities = (C.c_uint32 * max(1, len(params.fold_arities)))(*params.fold_arities)
        self.ch = _f128_array(list(challenges))
        self.roots = np.zeros((len(params.fold_arities) + 1, 32), dtype=np.uint8)
        self.terminate = np.zeros((1 << (params.log_inv_rate + params.n_final_challenges()), 2), dtype=np.uint64)
        self.phase_ms = (C.c_double * 2)()

    def run(self):
        p = self.p
        rc = host_lib().bnh_fri_commit_fold(
            self.hal._h, p.log_dim, p.log_inv_rate, p.log_batch_size, self.arities, len(p.fold_arities), p.n_test_queries,
            self.message.ptr, self.scratch.ptr, self.scratch.len, self.ch, self.roots.ctypes.data, self.terminate.ctypes.data, self.phase_ms,
        )
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())
        return self.phase_ms[0], self.phase_ms[1]


class FriProvePlan(FriPlan):
    """FriPlan with the query phase (bnh_fri_prove): FRIFolder::finish_proof in place of finalize.  query_indices: n_test_queries
    indices below 2^index_bits, handed in like the challenges.  After run(), `advice` is the decommitment as a (total, 2) uint64 array
    in transcript order and `terminate` its first terminate_elems rows; phase_ms: commit, fold, query phase."""

    def __init__(self, hal, params, message, scratch, challenges, query_indices, max_advice_elems=None):
        import numpy as np

        FriPlan.__init__(self, hal, params, message, scratch, challenges)
        self.indices = np.ascontiguousarray(np.asarray(list(query_indices), dtype=np.uint64))
        self.max_advice = params.advice_elems()[2] if max_advice_elems is None else max_advice_elems
        self._advice = np.zeros((max(1, self.max_advice), 2), dtype=np.uint64)
        self.n_advice = C.c_uint64()
        self.phase_ms = (C.c_double * 3)()

    def run(self):
        p = self.p
        _host_check(host_lib().bnh_fri_prove(
            self.hal._h, p.log_dim, p.log_inv_rate, p.log_batch_size, self.arities, len(p.fold_arities), p.n_test_queries, self.message.ptr,
            self.scratch.ptr, self.scratch.len, self.ch, self.roots.ctypes.data, self.indices.ctypes.data_as(C.POINTER(C.c_uint64)),
            self._advice.ctypes.data, self.max_advice, C.byref(self.n_advice), self.phase_ms))
        self.advice = self._advice[: self.n_advice.value]
        self.terminate = self.advice[: p.terminate_elems()]
        return tuple(self.phase_ms)


def fri_query_phase_bench(hal, params, message, scratch, challenges, query_indices, warmup, runs):
    """bnh_fri_query_phase_bench: (new_ms[runs], old_ms[runs], advice elements, same bytes) -- FRIFolder::finish_proof against the
    per-opening route on the same resident codewords and trees, alternating, wall clock between synchronisations."""
    import numpy as np

    ar = (C.c_uint32 * max(1, len(params.fold_arities)))(*params.fold_arities)
    idx = np.ascontiguousarray(np.asarray(list(query_indices), dtype=np.uint64))
    new_ms, old_ms = (C.c_double * max(1, runs))(), (C.c_double * max(1, runs))()
    n_adv, same = C.c_uint64(), C.c_uint32()
    _host_check(host_lib().bnh_fri_query_phase_bench(
        hal._h, params.log_dim, params.log_inv_rate, params.log_batch_size, ar, len(params.fold_arities), params.n_test_queries, message.ptr, scratch.ptr,
        scratch.len, _f128_array(list(challenges)), idx.ctypes.data_as(C.POINTER(C.c_uint64)), warmup, runs, new_ms, old_ms, C.byref(n_adv), C.byref(same)))
    return list(new_ms)[:runs], list(old_ms)[:runs], n_adv.value, bool(same.value)


class BatchSumcheckPlan:
    """p BivariateSumcheckProvers front-loaded on ONE layer (bnh_batch_sumcheck_prove = SumcheckBatchProver::run,
    protocols/sumcheck/prove/front_loaded.rs:33-203): per round execute() on every live prover, one challenge, fold() on
    every live prover.  provers: list of (n_vars, multilins, comps, sums), ascending by n_vars."""

    def __init__(self, hal, provers, scratch, batch_coeffs, challenges):
        self.hal, self.scratch = hal, scratch
        self.n = len(provers)
        desc, ptrs, flat, sums = [], [], [], []
        for n_vars, mls, comps, sm in provers:
            desc += [n_vars, len(mls), len(comps)]
            ptrs += [x.ptr for x in mls]
            flat += [i for pair in comps for i in pair]
            sums += list(sm)
        self._keep = provers
        self.desc = (C.c_uint32 * max(1, len(desc)))(*desc)
        self.ptrs = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        self.comps = (C.c_uint32 * max(1, len(flat)))(*flat)
        self.sums = _f128_array(sums if sums else [0])
        self.bcs = _f128_array(list(batch_coeffs))
        self.rounds = max([pv[0] for pv in provers]) if provers else 0
        assert len(challenges) >= self.rounds
        self.ch = _f128_array(list(challenges) if challenges else [0])
        self.proofs = (F128 * max(1, 2 * self.rounds))()
        self.total_m = len(ptrs)
        self.final = (F128 * max(1, self.total_m))()
        self.m_by_prover = [len(pv[1]) for pv in provers]

    def run(self):
        rc = host_lib().bnh_batch_sumcheck_prove(self.hal._h, self.n, self.desc, self.ptrs, self.comps, self.sums, self.scratch.ptr, self.scratch.len,
                                                 self.bcs, self.ch, self.proofs, self.final)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def round_proofs(self):
        return [[from_f128(self.proofs[2 * r]), from_f128(self.proofs[2 * r + 1])] for r in range(self.rounds)]

    def final_evals(self):
        out, at = [], 0
        for m in self.m_by_prover:
            out.append([from_f128(self.final[at + j]) for j in range(m)])
            at += m
        return out


class PiopPlan:
    """piop::prove through the compiled C++ mirror (bnh_piop_prove, binius_amd/host/piop.hpp): commit_interleaved of the merged
    message, one BivariateSumcheckProver per size, the front-loaded batch interleaved with the FRI folder
    (crates/core/src/piop/prove.rs:148-395).  committed / transparents: lists of (n_vars, device slice), ascending by n_vars;
    claims: list of (n_vars, committed index, transparent index, sum); params: FRIParams with log_dim + log_batch_size =
    total_vars; message: device slice of 2^total_vars elements (merge_multilins of the committed multilinears)."""

    KINDS = ("round_proof", "multilinear_evals", "fri_commitment", "fri_terminate")

    def __init__(self, hal, committed, transparents, claims, params, message, scratch, batch_coeffs, challenges):
        import numpy as np

        self.hal, self.p, self.message, self.scratch = hal, params, message, scratch
        self._keep = (committed, transparents)
        self.nc, self.nt = len(committed), len(transparents)
        self.c_nv = (C.c_uint32 * max(1, self.nc))(*[v for v, _ in committed])
        self.c_ptr = (C.c_void_p * max(1, self.nc))(*[s.ptr for _, s in committed])
        self.t_nv = (C.c_uint32 * max(1, self.nt))(*[v for v, _ in transparents])
        self.t_ptr = (C.c_void_p * max(1, self.nt))(*[s.ptr for _, s in transparents])
        flat = [x for c in claims for x in c[:3]]
        self.n_claims = len(claims)
        self.claims = (C.c_uint32 * max(1, len(flat)))(*flat)
        self.sums = _f128_array([c[3] for c in claims] if claims else [0])
        self.arities = (C.c_uint32 * max(1, len(params.fold_arities)))(*params.fold_arities)
        self.bcs, self.n_bcs = _f128_array(list(batch_coeffs) if batch_coeffs else [0]), len(batch_coeffs)
        self.ch, self.n_ch = _f128_array(list(challenges)), len(challenges)
        rounds = params.n_fold_rounds()
        self.max_items = 2 * rounds + self.nc + len(params.fold_arities) + 8
        self.max_scalars = 2 * rounds + self.nc + self.nt + (1 << (params.log_inv_rate + params.n_final_challenges())) + 8
        self.max_digests = len(params.fold_arities) + 1
        self.items = (C.c_uint32 * (2 * self.max_items))()
        self.scalars = (F128 * self.max_scalars)()
        self.digests = np.zeros((self.max_digests, 32), dtype=np.uint8)
        self.commitment = np.zeros(32, dtype=np.uint8)
        self.n_items, self.n_scalars, self.n_digests = C.c_uint32(), C.c_uint64(), C.c_uint32()
        self.phase_ms = (C.c_double * 2)()

    def run(self):
        p = self.p
        rc = host_lib().bnh_piop_prove(
            self.hal._h, self.nc, self.c_nv, self.c_ptr, self.nt, self.t_nv, self.t_ptr, self.n_claims, self.claims, self.sums,
            p.log_dim, p.log_inv_rate, p.log_batch_size, self.arities, len(p.fold_arities), p.n_test_queries, self.message.ptr,
            self.scratch.ptr, self.scratch.len, self.bcs, self.n_bcs, self.ch, self.n_ch, self.commitment.ctypes.data, self.items, self.max_items,
            C.byref(self.n_items), self.scalars, self.max_scalars, C.byref(self.n_scalars), self.digests.ctypes.data, self.max_digests,
            C.byref(self.n_digests), self.phase_ms,
        )
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())
        return self.phase_ms[0], self.phase_ms[1]

    def transcript(self):
        """[(kind, payload)] in writing order: lists of ints for scalar items, 32 bytes for a FRI commitment."""
        out, at_s, at_d = [], 0, 0
        for i in range(self.n_items.value):
            kind, cnt = self.KINDS[self.items[2 * i]], self.items[2 * i + 1]
            if kind == "fri_commitment":
                out.append((kind, bytes(self.digests[at_d])))
                at_d += 1
            else:
                out.append((kind, [from_f128(self.scalars[at_s + j]) for j in range(cnt)]))
                at_s += cnt
        return out


def _host_check(rc):
    if rc != 0:
        raise BnError(rc, host_lib().bnh_last_error().decode())


def piop_message_layout(n_varss):
    """bnh_piop_message_layout: (offsets, total_vars) -- where each committed multilinear (ascending by n_vars) starts in the message
    of merge_multilins, and CommitMeta::total_vars.  Host arithmetic; needs no context."""
    n = len(n_varss)
    nv = (C.c_uint32 * max(1, n))(*n_varss)
    offs, total = (C.c_uint64 * max(1, n))(), C.c_uint32()
    _host_check(host_lib().bnh_piop_message_layout(n, nv, offs, C.byref(total)))
    return [int(offs[i]) for i in range(n)], total.value


def piop_commit_elems(params):
    """bnh_piop_commit_elems: (codeword elements, tree elements) a PiopCommit with these FRIParams needs."""
    ar = (C.c_uint32 * max(1, len(params.fold_arities)))(*params.fold_arities)
    code, tree = C.c_uint64(), C.c_uint64()
    _host_check(host_lib().bnh_piop_commit_elems(params.log_dim, params.log_inv_rate, params.log_batch_size, ar, len(params.fold_arities), C.byref(code), C.byref(tree)))
    return code.value, tree.value


class PiopCommit:
    """piop::commit on the device (bnh_piop_commit; piop/prove.rs:120-165): merge_multilins of the committed multilinears straight
    into the codeword with every repeat, the batched NTT, the Merkle tree.  committed: list of (n_vars, device slice), ascending;
    codeword / tree: device slices of piop_commit_elems(params) elements, which hold the codeword and the flattened tree after
    run(); commitment: the 32-byte root; phase_ms: merge, encode, Merkle."""

    def __init__(self, hal, committed, params, codeword, tree):
        import numpy as np

        self.hal, self.p, self.codeword, self.tree = hal, params, codeword, tree
        self._keep = committed
        self.nc = len(committed)
        self.c_nv = (C.c_uint32 * max(1, self.nc))(*[v for v, _ in committed])
        self.c_ptr = (C.c_void_p * max(1, self.nc))(*[s.ptr for _, s in committed])
        self.arities = (C.c_uint32 * max(1, len(params.fold_arities)))(*params.fold_arities)
        self._commitment = np.zeros(32, dtype=np.uint8)
        self.phase_ms = (C.c_double * 3)()

    def run(self, phases=True):
        """phases=False: no phase_ms (and none of the synchronisations between the phases that taking them costs)"""
        p = self.p
        _host_check(host_lib().bnh_piop_commit(
            self.hal._h, self.nc, self.c_nv, self.c_ptr, p.log_dim, p.log_inv_rate, p.log_batch_size, self.arities, len(p.fold_arities), p.n_test_queries,
            self.codeword.ptr, self.codeword.len, self.tree.ptr, self.tree.len, self._commitment.ctypes.data, self.phase_ms if phases else None))
        self.total_ms = host_lib().bnh_piop_commit_last_ms()  # between the synchronisations around the commit, as PiopPlan's commit phase
        return tuple(self.phase_ms)

    @property
    def commitment(self):
        return bytes(self._commitment)


class PiopCommittedPlan(PiopPlan):
    """piop::prove from the codeword and tree of a PiopCommit (bnh_piop_prove_committed): PiopPlan without the message and without
    the commit.  It only reads the codeword and the tree: any number of plans may run from one commit.  transcript() as PiopPlan's;
    phase_ms[0]: the prove."""

    def __init__(self, hal, committed, transparents, claims, params, codeword, tree, scratch, batch_coeffs, challenges):
        PiopPlan.__init__(self, hal, committed, transparents, claims, params, None, scratch, batch_coeffs, challenges)
        self.codeword, self.tree = codeword, tree
        self.commitment = None
        self.phase_ms = (C.c_double * 1)()

    def run(self):
        p = self.p
        _host_check(host_lib().bnh_piop_prove_committed(
            self.hal._h, self.nc, self.c_nv, self.c_ptr, self.nt, self.t_nv, self.t_ptr, self.n_claims, self.claims, self.sums,
            p.log_dim, p.log_inv_rate, p.log_batch_size, self.arities, len(p.fold_arities), p.n_test_queries, self.codeword.ptr, self.tree.ptr,
            self.scratch.ptr, self.scratch.len, self.bcs, self.n_bcs, self.ch, self.n_ch, self.items, self.max_items,
            C.byref(self.n_items), self.scalars, self.max_scalars, C.byref(self.n_scalars), self.digests.ctypes.data, self.max_digests,
            C.byref(self.n_digests), self.phase_ms))
        return self.phase_ms[0]


class PiopCommittedOpenPlan(PiopCommittedPlan):
    """PiopCommittedPlan with the FRI query phase (bnh_piop_prove_committed_open): the same transcript items, and `advice`, the
    decommitment of FRIFolder::finish_proof for the given query indices, as a (total, 2) uint64 array."""

    def __init__(self, hal, committed, transparents, claims, params, codeword, tree, scratch, batch_coeffs, challenges, query_indices, max_advice_elems=None):
        import numpy as np

        PiopCommittedPlan.__init__(self, hal, committed, transparents, claims, params, codeword, tree, scratch, batch_coeffs, challenges)
        self.indices = np.ascontiguousarray(np.asarray(list(query_indices), dtype=np.uint64))
        self.max_advice = params.advice_elems()[2] if max_advice_elems is None else max_advice_elems
        self._advice = np.zeros((max(1, self.max_advice), 2), dtype=np.uint64)
        self.n_advice = C.c_uint64()

    def run(self):
        p = self.p
        _host_check(host_lib().bnh_piop_prove_committed_open(
            self.hal._h, self.nc, self.c_nv, self.c_ptr, self.nt, self.t_nv, self.t_ptr, self.n_claims, self.claims, self.sums,
            p.log_dim, p.log_inv_rate, p.log_batch_size, self.arities, len(p.fold_arities), p.n_test_queries, self.codeword.ptr, self.tree.ptr,
            self.scratch.ptr, self.scratch.len, self.bcs, self.n_bcs, self.ch, self.n_ch, self.items, self.max_items,
            C.byref(self.n_items), self.scalars, self.max_scalars, C.byref(self.n_scalars), self.digests.ctypes.data, self.max_digests,
            C.byref(self.n_digests), self.phase_ms, self.indices.ctypes.data_as(C.POINTER(C.c_uint64)), self._advice.ctypes.data, self.max_advice,
            C.byref(self.n_advice)))
        self.advice = self._advice[: self.n_advice.value]
        return self.phase_ms[0]


class EqIndPlan:
    """EqIndSumcheckProver over the old HAL (bnh_eqind_sumcheck_prove = binius_amd/host/eq_ind.hpp;
    crates/core/src/protocols/sumcheck/prove/eq_ind.rs:378-644): the zerocheck of a constraint set, one composition (degree 1 .. 8: `degrees`, default all 2)
    per constraint over ALL multilinears, High-to-Low.  multilins: device slices of 2^n_vars elements, FOLDED IN PLACE by run();
    compositions: list of (steps, steps_of_the_leading_form) in compile_expr's notation; sums: one claimed sum per composition;
    eq_scratch: device slice of >= 2^(n_vars - 1) elements."""

    def __init__(self, hal, n_vars, multilins, compositions, sums, eq_ind_challenges, eq_scratch, batch_coeff, challenges, degrees=None):
        from ._ffi import make_steps

        self.degrees = (C.c_uint32 * max(1, len(compositions)))(*(degrees if degrees is not None else [2] * len(compositions)))
        self.hal, self.n_vars, self.m = hal, n_vars, len(multilins)
        self._keep = (multilins, eq_scratch)
        self.ptrs = (C.c_void_p * max(1, self.m))(*[x.ptr for x in multilins])
        self.n_comps = len(compositions)
        flat = [st for c, _ in compositions for st in c]
        flat_inf = [st for _, ci in compositions for st in ci]
        self.steps, self.steps_inf = make_steps(flat) if flat else None, make_steps(flat_inf) if flat_inf else None
        self.n_steps = (C.c_uint32 * max(1, self.n_comps))(*[len(c) for c, _ in compositions])
        self.n_steps_inf = (C.c_uint32 * max(1, self.n_comps))(*[len(ci) for _, ci in compositions])
        self.sums = _f128_array(list(sums) if sums else [0])
        assert len(eq_ind_challenges) == n_vars and len(challenges) >= n_vars
        self.eqc, self.ch = _f128_array(list(eq_ind_challenges)), _f128_array(list(challenges))
        self.bc = to_f128(batch_coeff)
        self.eq_scratch = eq_scratch
        self.per_round = 2 + max([2] + [int(d) for d in (degrees or [])])  # the round polynomials' coefficients: the largest degree (>= 2) + 2
        self.coeffs = (F128 * (self.per_round * n_vars))()
        self.final = (F128 * (self.m + 1))()

    def run(self):
        rc = host_lib().bnh_eqind_sumcheck_prove(
            self.hal._h, self.n_vars, self.m, self.ptrs, self.n_comps, C.cast(self.steps, C.c_void_p), self.n_steps, C.cast(self.steps_inf, C.c_void_p),
            self.n_steps_inf, self.degrees, self.sums, self.eqc, self.eq_scratch.ptr, self.eq_scratch.len, C.byref(self.bc), self.ch, self.coeffs, self.final)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def round_coeffs(self):
        return [[from_f128(self.coeffs[self.per_round * r + i]) for i in range(self.per_round)] for r in range(self.n_vars)]

    def final_evals(self):
        return [from_f128(self.final[j]) for j in range(self.m + 1)]


class GkrGpaPlan:
    """gkr_gpa::batch_prove (bnh_gkr_gpa_prove = binius_amd/host/gkr_gpa.hpp; crates/core/src/protocols/gkr_gpa/prove.rs:33-296): the GKR
    grand-product argument over a batch of witnesses.  n_vars: one per claim; inputs: device slices of up to 2^n_vars elements
    (None = empty; the absent tail counts as ONE; only read); arenas: device slices of 2^n_vars elements (None for n_vars = 0),
    CONSUMED by run(); scratch: device slice of at least scratch_elems(n_vars) elements; batch_coeffs / gpa_challenges: one per step
    j < max(n_vars); sumcheck_challenges: list per step j of its j challenges."""

    @staticmethod
    def scratch_elems(n_vars):
        m = max(list(n_vars) + [0])
        return sum(1 << n for n in n_vars if n >= 1) + ((1 << (m - 1)) if m >= 1 else 0)

    def __init__(self, hal, n_vars, inputs, arenas, scratch, batch_coeffs, sumcheck_challenges, gpa_challenges):
        self.hal, self.n_vars, self.k = hal, list(n_vars), len(n_vars)
        self.max_n = m = max(self.n_vars + [0])
        self._keep = (inputs, arenas, scratch)
        k1 = max(1, self.k)
        self.nv = (C.c_uint32 * k1)(*self.n_vars)
        self.ins = (C.c_void_p * k1)(*[(x.ptr if x is not None else None) for x in inputs])
        self.lens = (C.c_uint64 * k1)(*[(x.len if x is not None else 0) for x in inputs])
        self.ars = (C.c_void_p * k1)(*[(a.ptr if a is not None else None) for a in arenas])
        self.scratch = scratch
        assert len(batch_coeffs) >= m and len(gpa_challenges) >= m and len(sumcheck_challenges) >= m
        assert all(len(sumcheck_challenges[j]) == j for j in range(m))
        flat = [z for j in range(m) for z in sumcheck_challenges[j]]
        self.bc, self.sc, self.gc = _f128_array(list(batch_coeffs[:m]) or [0]), _f128_array(flat or [0]), _f128_array(list(gpa_challenges[:m]) or [0])
        # claims in the sorted order (n_vars descending, stable): the active ones of step j are those with n_vars > j
        self.active = [sum(1 for n in self.n_vars if n > j) for j in range(m)]
        self.products = (F128 * k1)()
        self.proofs = (F128 * max(1, 3 * m * (m - 1) // 2))()
        self.evals = (F128 * max(1, sum(2 * a + 1 for a in self.active)))()
        self.points = (F128 * max(1, sum(self.n_vars)))()
        self.finals = (F128 * k1)()
        self.step_ms = (C.c_double * max(1, m))()

    def run(self):
        rc = host_lib().bnh_gkr_gpa_prove(self.hal._h, self.k, self.nv, self.ins, self.lens, self.ars, self.scratch.ptr, self.scratch.len, self.bc, self.sc, self.gc,
                                          self.products, self.proofs, self.evals, self.points, self.finals, self.step_ms)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def output(self):
        """The proof in the shape of tests/gkr_gpa_ref.py gpa_prove."""
        proofs, evals, at_p, at_e = [], [], 0, 0
        for j in range(self.max_n):
            proofs.append([[from_f128(self.proofs[at_p + 3 * r + i]) for i in range(3)] for r in range(j)])
            at_p += 3 * j
            cnt = 2 * self.active[j] + 1
            evals.append([from_f128(self.evals[at_e + i]) for i in range(cnt)])
            at_e += cnt
        points, at = [], 0
        for n in self.n_vars:
            points.append([from_f128(self.points[at + i]) for i in range(n)])
            at += n
        return {"products": [from_f128(self.products[t]) for t in range(self.k)], "round_proofs": proofs, "layer_evals": evals, "final_points": points,
                "final_evals": [from_f128(self.finals[t]) for t in range(self.k)]}

    def step_times_ms(self):
        return [self.step_ms[j] for j in range(self.max_n)]


class FlushProdcheckPlan:
    """The product-check phase of the constraint-system prover (bnh_flush_prodcheck_prove = binius_amd/host/flush.hpp;
    crates/core/src/constraint_system/prove.rs:276-428): flush witnesses on the device, the grand-product argument over every flush and
    non-zero oracle, and the reduction of the composite flush claims to claims on their selectors and inner columns.
    flushes: dicts {"channel", "n_vars", "selectors": [(oracle id, device slice)], "entries": [("oracle", id, device slice, tower level) |
    ("const", base)]} in the caller's order (sorted by channel); nonzero: [(id, device slice, tower level, n_vars)]; all columns only read.
    gpa_*: the samples GkrGpaPlan takes, sized by the largest n_vars of all witnesses; red_batch_coeffs[g] / red_challenges[g]: one
    coefficient and n_vars challenges per MLE-check, in the order of groups(flushes)."""

    @staticmethod
    def groups(flushes):
        """[(n_vars, [flush indices], sorted de-duplicated ids)]: the composite flushes grouped by n_vars (= by evaluation point) in order
        of first appearance."""
        out = []
        for f, fl in enumerate(flushes):
            if not fl["selectors"]:
                continue
            g = next((g for g in out if g[0] == fl["n_vars"]), None)
            if g is None:
                g = (fl["n_vars"], [], set())
                out.append(g)
            g[1].append(f)
            g[2].update([s[0] for s in fl["selectors"]] + [e[1] for e in fl["entries"] if e[0] == "oracle"])
        return [(n, fs, sorted(ids)) for n, fs, ids in out]

    @staticmethod
    def scratch_elems(flushes, nonzero):
        nv = [fl["n_vars"] for fl in flushes] + [z[3] for z in nonzero]
        red = max([(len(ids) << n) + ((1 << (n - 1)) if n >= 1 else 0) for n, _, ids in FlushProdcheckPlan.groups(flushes)] + [0])
        return 1 + sum((1 << n) + ((1 << n) if n >= 1 else 0) for n in nv) + GkrGpaPlan.scratch_elems(nv) + red

    def __init__(self, hal, flushes, nonzero, mixing_challenge, permutation_challenges, scratch, gpa_batch_coeffs, gpa_sumcheck_challenges, gpa_challenges,
                 red_batch_coeffs, red_challenges):
        self.hal, self.flushes, self.nonzero, self.scratch = hal, flushes, nonzero, scratch
        self.nf, self.nz = len(flushes), len(nonzero)
        self.n_vars = [fl["n_vars"] for fl in flushes] + [z[3] for z in nonzero]
        self.max_n = m = max(self.n_vars + [0])
        self.grp = self.groups(flushes)
        u32 = lambda v: (C.c_uint32 * max(1, len(v)))(*v)
        vps = lambda v: (C.c_void_p * max(1, len(v)))(*[(x.ptr if x is not None else None) for x in v])
        sels = [s for fl in flushes for s in fl["selectors"]]
        ents = [e for fl in flushes for e in fl["entries"]]
        self.a_ch, self.a_nv, self.a_ns = u32([fl["channel"] for fl in flushes]), u32([fl["n_vars"] for fl in flushes]), u32([len(fl["selectors"]) for fl in flushes])
        self.a_sid, self.a_sp = u32([s[0] for s in sels]), vps([s[1] for s in sels])
        self.a_ne = u32([len(fl["entries"]) for fl in flushes])
        self.a_ek = u32([0 if e[0] == "oracle" else 1 for e in ents])
        self.a_eid = u32([e[1] if e[0] == "oracle" else 0 for e in ents])
        self.a_ep = vps([e[2] if e[0] == "oracle" else None for e in ents])
        self.a_el = u32([e[3] if e[0] == "oracle" else 0 for e in ents])
        self.a_ec = _f128_array([e[1] if e[0] == "const" else 0 for e in ents] or [0])
        self.z_id, self.z_p, self.z_l, self.z_n = u32([z[0] for z in nonzero]), vps([z[1] for z in nonzero]), u32([z[2] for z in nonzero]), u32([z[3] for z in nonzero])
        self.mix, self.perm, self.n_channels = _f128_array([mixing_challenge]), _f128_array(list(permutation_challenges) or [0]), len(permutation_challenges)
        assert len(gpa_batch_coeffs) >= m and len(gpa_challenges) >= m and len(gpa_sumcheck_challenges) >= m
        flat = [z for j in range(m) for z in gpa_sumcheck_challenges[j]]
        self.bc, self.sc, self.gc = _f128_array(list(gpa_batch_coeffs[:m]) or [0]), _f128_array(flat or [0]), _f128_array(list(gpa_challenges[:m]) or [0])
        assert len(red_batch_coeffs) >= len(self.grp) and all(len(red_challenges[g]) == self.grp[g][0] for g in range(len(self.grp)))
        self.rbc = _f128_array(list(red_batch_coeffs[: len(self.grp)]) or [0])
        self.rch = _f128_array([z for g in range(len(self.grp)) for z in red_challenges[g]] or [0])
        k1 = max(1, self.nf + self.nz)
        self.active = [sum(1 for n in self.n_vars if n > j) for j in range(m)]
        self.prefix = (C.c_uint64 * max(1, self.nf))()
        self.products, self.finals = (F128 * k1)(), (F128 * k1)()
        self.proofs = (F128 * max(1, 3 * m * (m - 1) // 2))()
        self.evals = (F128 * max(1, sum(2 * a + 1 for a in self.active)))()
        self.points = (F128 * max(1, sum(self.n_vars)))()
        g1 = max(1, len(self.grp))
        self.n_checks, self.n_linear = C.c_uint32(0), C.c_uint32(0)
        self.desc, self.ids = (C.c_uint32 * (3 * g1))(), (C.c_uint32 * max(1, sum(len(g[2]) for g in self.grp)))()
        self.c_proofs = (F128 * max(1, sum(9 * g[0] for g in self.grp)))()
        self.c_evals = (F128 * max(1, sum(len(g[2]) + 1 for g in self.grp)))()
        self.linear = (C.c_uint32 * max(1, self.nf))()
        self.phase_ms = (C.c_double * 4)()

    def run(self):
        rc = host_lib().bnh_flush_prodcheck_prove(
            self.hal._h, self.nf, self.a_ch, self.a_nv, self.a_ns, self.a_sid, self.a_sp, self.a_ne, self.a_ek, self.a_eid, self.a_ep, self.a_el, self.a_ec,
            self.nz, self.z_id, self.z_p, self.z_l, self.z_n, self.mix, self.perm, self.n_channels, self.scratch.ptr, self.scratch.len, self.bc, self.sc, self.gc,
            self.rbc, self.rch, self.prefix, self.products, self.proofs, self.evals, self.points, self.finals, C.byref(self.n_checks), self.desc, self.ids,
            self.c_proofs, self.c_evals, C.byref(self.n_linear), self.linear, self.phase_ms)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def output(self):
        """The proof in the shape of tests/flush_ref.py flush_prodcheck_prove."""
        m, k = self.max_n, self.nf + self.nz
        proofs, evals, at_p, at_e = [], [], 0, 0
        for j in range(m):
            proofs.append([[from_f128(self.proofs[at_p + 3 * r + i]) for i in range(3)] for r in range(j)])
            at_p += 3 * j
            cnt = 2 * self.active[j] + 1
            evals.append([from_f128(self.evals[at_e + i]) for i in range(cnt)])
            at_e += cnt
        points, at = [], 0
        for n in self.n_vars:
            points.append([from_f128(self.points[at + i]) for i in range(n)])
            at += n
        gpa = {"products": [from_f128(self.products[t]) for t in range(k)], "round_proofs": proofs, "layer_evals": evals, "final_points": points,
               "final_evals": [from_f128(self.finals[t]) for t in range(k)]}
        checks, at_i, at_c, at_v = [], 0, 0, 0
        for g in range(self.n_checks.value):
            n, n_ml, per = self.desc[3 * g], self.desc[3 * g + 1], self.desc[3 * g + 2]
            ids = [int(self.ids[at_i + i]) for i in range(n_ml)]
            rounds = [[from_f128(self.c_proofs[at_c + per * r + i]) for i in range(per)] for r in range(n)]
            fin = [from_f128(self.c_evals[at_v + i]) for i in range(n_ml + 1)]
            at_i, at_c, at_v = at_i + n_ml, at_c + per * n, at_v + n_ml + 1
            checks.append({"n_vars": int(n), "ids": ids, "round_proofs": rounds, "final_evals": fin})
        return {"prefix_lens": [int(self.prefix[f]) for f in range(self.nf)], "gpa": gpa, "checks": checks,
                "linear_flushes": [int(self.linear[i]) for i in range(self.n_linear.value)]}

    def phase_times_ms(self):
        return dict(zip(("witnesses", "gpa", "reductions", "total"), [self.phase_ms[i] for i in range(4)]))


class GkrExpPlan:
    """gkr_exp::batch_prove (bnh_gkr_exp_prove = binius_amd/host/gkr_exp.hpp; crates/core/src/protocols/gkr_exp/batch_prove.rs:46-315): the
    GKR exponentiation argument over a batch of claims sorted by n_vars descending.  Per claim: n_vars; bit_columns: device slices e_0 ..
    e_{w-1} (packed B1 multilinears, only read); bases: an int (static) or a device slice of 2^n_vars elements (dynamic, only read);
    arenas: device slices of w * 2^n_vars elements, filled and then CONSUMED by run(); eval_points / evals: the claims; scratch: a device
    slice of at least scratch_elems(n_vars, dynamic) elements; batch_coeffs[L][g], challenges[L][r]: the samples per layer (g-th sumcheck
    prover, round r).  n_witnesses: how many witnesses the caller believes it passes (default: as many as claims)."""

    @staticmethod
    def scratch_elems(n_vars, dynamic):
        return sum(((2 if d else 1) << n) + ((1 << (n - 1)) if n >= 1 else 0) for n, d in zip(n_vars, dynamic))

    def __init__(self, hal, n_vars, bit_columns, bases, arenas, eval_points, evals, scratch, batch_coeffs, challenges, n_witnesses=None):
        self.hal, self.n_vars, self.k = hal, list(n_vars), len(n_vars)
        self.n_witnesses = self.k if n_witnesses is None else n_witnesses
        self._keep = (bit_columns, bases, arenas, scratch)
        k1 = max(1, self.k)
        self.widths = [len(b) for b in bit_columns]
        self.M, self.N = max(self.widths + [0]), max(1, max(self.n_vars + [0]))
        max_n = max(self.n_vars + [0])
        self.nv = (C.c_uint32 * k1)(*self.n_vars)
        self.wd = (C.c_uint32 * k1)(*self.widths)
        self.kd = (C.c_uint32 * k1)(*[0 if isinstance(b, int) else 1 for b in bases])
        flat = [c.ptr for cols in bit_columns for c in cols]
        self.cols = (C.c_void_p * max(1, len(flat)))(*flat)
        self.sb = _f128_array([b if isinstance(b, int) else 0 for b in bases] or [0])
        self.db = (C.c_void_p * k1)(*[(None if isinstance(b, int) else b.ptr) for b in bases])
        self.ars = (C.c_void_p * k1)(*[(a.ptr if a is not None else None) for a in arenas])
        self.pts = _f128_array([z for p in eval_points for z in p] or [0])
        self.evs = _f128_array(list(evals) or [0])
        self.scratch = scratch
        M, N, K = max(1, self.M), self.N, k1
        bc = [0] * (M * K)
        for L, row in enumerate(batch_coeffs[: self.M]):
            bc[L * K : L * K + min(K, len(row))] = list(row)[:K]
        ch = [0] * (M * N)
        for L, row in enumerate(challenges[: self.M]):
            ch[L * max_n : L * max_n + min(max_n, len(row))] = list(row)[:max_n]
        self.bc, self.ch = _f128_array(bc), _f128_array(ch)
        self.n_layers = C.c_uint32(0)
        self.rounds, self.coeff_cnt, self.proofs = (C.c_uint32 * M)(), (C.c_uint32 * (M * N))(), (F128 * (5 * M * N))()
        self.n_provers, self.eval_cnt, self.ml_evals = (C.c_uint32 * M)(), (C.c_uint32 * (M * K))(), (F128 * (4 * M * K))()
        self.n_lc, self.lc_nv = (C.c_uint32 * M)(), (C.c_uint32 * (2 * M * K))()
        self.lc_pts, self.lc_evs = (F128 * (2 * M * K * N))(), (F128 * (2 * M * K))()
        self.layer_ms = (C.c_double * M)()

    def run(self):
        rc = host_lib().bnh_gkr_exp_prove(self.hal._h, self.n_witnesses, self.wd, self.kd, self.cols, self.sb, self.db, self.ars, self.k, self.nv, self.pts,
                                          self.evs, self.scratch.ptr if self.scratch is not None else None, self.scratch.len if self.scratch is not None else 0,
                                          self.bc, self.ch, C.byref(self.n_layers), self.rounds, self.coeff_cnt, self.proofs, self.n_provers, self.eval_cnt,
                                          self.ml_evals, self.n_lc, self.lc_nv, self.lc_pts, self.lc_evs, self.layer_ms)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def output(self):
        """The proof in the shape of tests/gkr_exp_ref.py exp_prove."""
        K, N = max(1, self.k), self.N
        proofs, evals, claims, at_c, at_e, at_p, at_v = [], [], [], 0, 0, 0, 0
        for L in range(self.n_layers.value):
            rounds = []
            for r in range(self.rounds[L]):
                cnt = self.coeff_cnt[L * N + r]
                rounds.append([from_f128(self.proofs[at_c + i]) for i in range(cnt)])
                at_c += cnt
            proofs.append(rounds)
            per = []
            for g in range(self.n_provers[L]):
                cnt = self.eval_cnt[L * K + g]
                per.append([from_f128(self.ml_evals[at_e + i]) for i in range(cnt)])
                at_e += cnt
            evals.append(per)
            lcs = []
            for i in range(self.n_lc[L]):
                n = self.lc_nv[L * 2 * K + i]
                lcs.append(([from_f128(self.lc_pts[at_p + j]) for j in range(n)], from_f128(self.lc_evs[at_v])))
                at_p += n
                at_v += 1
            claims.append(lcs)
        return {"round_proofs": proofs, "multilinear_evals": evals, "layer_claims": claims}

    def layer_times_ms(self):
        return [self.layer_ms[L] for L in range(self.n_layers.value)]


class EvalcheckPlan:
    """One round of evalcheck's bivariate sumchecks (bnh_evalcheck_bivariate_prove = binius_amd/host/evalcheck.hpp; one call of
    prove_bivariate_sumchecks_with_switchover, evalcheck/subclaims.rs:549-586, with the witness construction in front of it).
    provers: list of (b, multilins, comps, sums) ascending by b; a multilinear is one of
      ("proj", column DevSlice, tower_level, n_vars, suffix_off, suffix_len)   the inner column at the suffix pool[suffix_off : + suffix_len]
      ("shift", block_size, shift_offset, variant, r_off, r_len)               variant: 0 circular left, 1 logical left, 2 logical right
      ("basis", k, iota)
      ("lincomb", terms, offset, n_vars, suffix_off, suffix_len)               offset + sum of coeff * column over terms = [(column DevSlice,
                                                                               tower_level, coeff), ...], projected from its constituents
                                                                               (bnh_evalcheck_bivariate_prove_lc; never materialised)
    pool: the shared list of point coordinates; scratch: a device slice of at least scratch_elems(provers) elements.
    A projection's final evaluation v is the new claim (r' || suffix, v) on its inner column, r' the reversed challenges; a lincomb's is
    that claim on the linear-combination oracle itself.  Equal term lists share one range of the call's term list, so an identical
    (terms, offset, suffix) is projected once."""

    KINDS = {"proj": 0, "shift": 1, "basis": 2, "lincomb": 3}

    @staticmethod
    def _term_key(terms):
        return tuple((t[0].ptr if t[0] is not None else None, int(t[1]), int(t[2])) for t in terms)

    @staticmethod
    def scratch_elems(provers):
        suffixes, projections, lincombs, total = set(), set(), set(), 0
        for b, mls, _comps, _sums in provers:
            for ml in mls:
                if ml[0] == "proj":
                    s = (ml[4], ml[5])
                    if s not in suffixes:
                        suffixes.add(s)
                        total += 1 << ml[5]
                    if (ml[1].ptr, ml[2], s) not in projections:
                        projections.add((ml[1].ptr, ml[2], s))
                        total += 1 << b
                elif ml[0] == "lincomb":
                    s = (ml[4], ml[5])
                    if s not in suffixes:
                        suffixes.add(s)
                        total += 1 << ml[5]
                    key = (EvalcheckPlan._term_key(ml[1]), int(ml[2]), s, int(ml[3]))
                    if key not in lincombs:
                        lincombs.add(key)
                        total += 1 << b
                else:
                    total += 1 << b
            if b >= 1:
                total += len(mls) << (b - 1)
        return total

    def __init__(self, hal, provers, pool, scratch, batch_coeffs, challenges):
        self.hal, self.scratch, self._keep = hal, scratch, provers
        self.n = len(provers)
        desc, mld, cols, flat, sums = [], [], [], [], []
        ranges, terms, offsets = {}, [], []
        for b, mls, comps, sm in provers:
            desc += [b, len(mls), len(comps)]
            for ml in mls:
                offsets.append(int(ml[2]) if ml[0] == "lincomb" else 0)
                if ml[0] == "lincomb":
                    key = self._term_key(ml[1])
                    if key not in ranges:
                        ranges[key] = len(terms)
                        terms += list(key)
                    mld += [self.KINDS["lincomb"], int(ml[3]), int(ml[4]), int(ml[5]), ranges[key], len(key)]
                    cols.append(None)
                    continue
                words = [self.KINDS[ml[0]]] + [int(x) for x in (ml[2:] if ml[0] == "proj" else ml[1:])]
                mld += words + [0] * (6 - len(words))
                cols.append(ml[1].ptr if ml[0] == "proj" and ml[1] is not None else None)
            flat += [i for pair in comps for i in pair]
            sums += list(sm)
        self.desc = (C.c_uint32 * max(1, len(desc)))(*desc)
        self.mld = (C.c_uint32 * max(1, len(mld)))(*mld)
        self.cols = (C.c_void_p * max(1, len(cols)))(*cols)
        self.has_lincomb = bool(ranges)
        self.n_terms = len(terms)
        self.term_levels = (C.c_uint32 * max(1, len(terms)))(*[t[1] for t in terms])
        self.term_cols = (C.c_void_p * max(1, len(terms)))(*[t[0] for t in terms])
        self.term_coeffs = _f128_array([t[2] for t in terms] or [0])
        self.offsets = _f128_array(offsets or [0])
        self.pool, self.pool_len = _f128_array(list(pool) or [0]), len(pool)
        self.comps = (C.c_uint32 * max(1, len(flat)))(*flat)
        self.sums = _f128_array(sums if sums else [0])
        self.bcs = _f128_array(list(batch_coeffs) or [0])
        self.rounds = max([pv[0] for pv in provers]) if provers else 0
        assert len(challenges) >= self.rounds
        self.ch = _f128_array(list(challenges) if challenges else [0])
        self.proofs = (F128 * max(1, 2 * self.rounds))()
        self.m_by_prover = [len(pv[1]) for pv in provers]
        self.final = (F128 * max(1, sum(self.m_by_prover)))()

    def run(self):
        tail = (self.pool, self.pool_len, self.comps, self.sums, self.scratch.ptr if self.scratch is not None else None,
                self.scratch.len if self.scratch is not None else 0, self.bcs, self.ch, self.proofs, self.final)
        if self.has_lincomb:
            rc = host_lib().bnh_evalcheck_bivariate_prove_lc(self.hal._h, self.n, self.desc, self.mld, self.cols, self.n_terms, self.term_levels, self.term_cols,
                                                             self.term_coeffs, self.offsets, *tail)
        else:
            rc = host_lib().bnh_evalcheck_bivariate_prove(self.hal._h, self.n, self.desc, self.mld, self.cols, *tail)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def round_proofs(self):
        return [[from_f128(self.proofs[2 * r]), from_f128(self.proofs[2 * r + 1])] for r in range(self.rounds)]

    def final_evals(self):
        out, at = [], 0
        for m in self.m_by_prover:
            out.append([from_f128(self.final[at + j]) for j in range(m)])
            at += m
        return out


class EvalcheckEvaluatePlan:
    """The evaluations in front of an evalcheck round (bnh_evalcheck_evaluate = evalcheck_evaluate_claims of binius_amd/host/evalcheck.hpp;
    the first step of EvalcheckProver::prove, evalcheck/prove.rs:191-275).  claims: (column DevSlice, tower_level, n_vars, point_off,
    point_len) per claim, the point pool[point_off : + point_len] with point_len == n_vars; pool: the shared list of point coordinates;
    scratch: a device slice of at least scratch_elems(claims) elements.  Every point is split at min(point_len // 2, LO_SPLIT), distinct
    prefix and suffix slices are expanded once, a repeated claim is evaluated once, one bn_mle_evaluate_batch serves all."""

    LO_SPLIT = 8  # BNH_EVALCHECK_LO_SPLIT
    PHASES = ("expand", "evaluate")

    @classmethod
    def scratch_elems(cls, claims, lo_split=None):
        """2^len per distinct prefix slice and per distinct suffix slice of the pool."""
        split = cls.LO_SPLIT if lo_split is None else lo_split
        prefixes, suffixes, total = set(), set(), 0
        for _col, _level, _n_vars, off, ln in claims:
            lo = min(ln // 2, split)
            if (off, lo) not in prefixes:
                prefixes.add((off, lo))
                total += 1 << lo
            if (off + lo, ln - lo) not in suffixes:
                suffixes.add((off + lo, ln - lo))
                total += 1 << (ln - lo)
        return total

    def __init__(self, hal, claims, pool, scratch):
        self.hal, self.scratch, self._keep = hal, scratch, claims
        self.n = len(claims)
        self.desc = (C.c_uint32 * max(1, 4 * self.n))(*[int(w) for c in claims for w in c[1:5]])
        self.cols = (C.c_void_p * max(1, self.n))(*[(c[0].ptr if c[0] is not None else None) for c in claims])
        self.pool, self.pool_len = _f128_array(list(pool) or [0]), len(pool)
        self.out = (F128 * max(1, self.n))()
        self.phase_ms = (C.c_double * 2)()

    def run(self):
        rc = host_lib().bnh_evalcheck_evaluate(self.hal._h, self.n, self.desc, self.cols, self.pool, self.pool_len,
                                               self.scratch.ptr if self.scratch is not None else None, self.scratch.len if self.scratch is not None else 0,
                                               self.out, self.phase_ms)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def evals(self):
        return [from_f128(self.out[i]) for i in range(self.n)]

    def phase_times_ms(self):
        return {name: self.phase_ms[i] for i, name in enumerate(self.PHASES)}


class RingSwitchPlan:
    """The ring-switching reduction (bnh_ring_switch_prove = binius_amd/host/ring_switch.hpp; ring_switch::prove, ring_switch/prove.rs:42-144).
    columns: (DevSlice, tower_level, n_vars) per committed column; pool: the shared list of point coordinates; suffixes: (off, len, kappa)
    per suffix descriptor; prefix_kappas: kappa per prefix descriptor; claims: (committed_idx, suffix_desc_idx, prefix_desc_idx) in the
    reference's claim order; mixing_challenges: ceil(log2 n_claims) of them, row_batch_challenges: max kappa of them; scratch: a device
    slice of at least scratch_elems(suffixes, claims) elements.  The PIOP sumcheck claim of claim i is (suffix length, committed_idx,
    transparent i, row_batched_evals()[i])."""

    PHASES = ("partial_evals", "tensor_algebra", "eq_inds")

    @staticmethod
    def scratch_elems(suffixes, claims):
        """2^len per distinct suffix (slice of the pool), 2^kappa per distinct (column, suffix), 2^len per claim."""
        tables, pairs, total = set(), set(), 0
        for col, si, _pi in claims:
            off, ln, kappa = suffixes[si]
            if (off, ln) not in tables:
                tables.add((off, ln))
                total += 1 << ln
            if (col, off, ln) not in pairs:
                pairs.add((col, off, ln))
                total += 1 << kappa
            total += 1 << ln
        return total

    def __init__(self, hal, columns, pool, suffixes, prefix_kappas, claims, scratch, mixing_challenges, row_batch_challenges):
        self.hal, self.scratch, self._keep = hal, scratch, columns
        self.n_columns, self.n_suffixes, self.n_prefixes, self.n_claims = len(columns), len(suffixes), len(prefix_kappas), len(claims)
        self.cols = (C.c_void_p * max(1, self.n_columns))(*[(c[0].ptr if c[0] is not None else None) for c in columns])
        self.col_desc = (C.c_uint32 * max(1, 2 * self.n_columns))(*[int(w) for c in columns for w in c[1:3]])
        self.pool, self.pool_len = _f128_array(list(pool) or [0]), len(pool)
        self.suffix_desc = (C.c_uint32 * max(1, 3 * self.n_suffixes))(*[int(w) for s in suffixes for w in s])
        self.prefix_kappas = (C.c_uint32 * max(1, self.n_prefixes))(*[int(k) for k in prefix_kappas])
        self.claim_desc = (C.c_uint32 * max(1, 3 * self.n_claims))(*[int(w) for c in claims for w in c])
        self.mixing, self.n_mixing = _f128_array(list(mixing_challenges) or [0]), len(mixing_challenges)
        self.row, self.n_row = _f128_array(list(row_batch_challenges) or [0]), len(row_batch_challenges)
        self.mixed_counts = [1 << int(k) for k in prefix_kappas]
        self.mixed = (F128 * max(1, sum(self.mixed_counts)))()
        self.evals = (F128 * max(1, self.n_claims))()
        self.transparent_ptrs = (C.c_void_p * max(1, self.n_claims))()
        self.transparent_lens = [1 << int(suffixes[c[1]][1]) for c in claims] if all(c[1] < len(suffixes) for c in claims) else [0] * len(claims)
        self.phase_ms = (C.c_double * 3)()

    def run(self):
        rc = host_lib().bnh_ring_switch_prove(self.hal._h, self.n_columns, self.cols, self.col_desc, self.pool, self.pool_len, self.n_suffixes, self.suffix_desc,
                                              self.n_prefixes, self.prefix_kappas, self.n_claims, self.claim_desc, self.mixing, self.n_mixing, self.row, self.n_row,
                                              self.scratch.ptr if self.scratch is not None else None, self.scratch.len if self.scratch is not None else 0,
                                              self.mixed, self.evals, self.transparent_ptrs, self.phase_ms)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())

    def mixed_tensor_elems(self):
        """Per prefix descriptor its 2^kappa vertical elements."""
        out, at = [], 0
        for n in self.mixed_counts:
            out.append([from_f128(self.mixed[at + j]) for j in range(n)])
            at += n
        return out

    def row_batched_evals(self):
        return [from_f128(self.evals[i]) for i in range(self.n_claims)]

    def transparents(self):
        """The transparent of every claim as a DevSlice inside the scratch, in claim order."""
        from ._ffi import DevSlice

        return [DevSlice(self.transparent_ptrs[i], self.transparent_lens[i]) for i in range(self.n_claims)]

    def phase_times_ms(self):
        return {name: self.phase_ms[i] for i, name in enumerate(self.PHASES)}


class ShmExchange:
    """Intra-node exchange of a few 64-bit words per round through POSIX shared memory (host_capi.cpp
    bnh_shm_*): rank 0 creates the segment, the name travels over the torch.distributed group."""

    def __init__(self, dist, rank, world):
        import uuid

        L = host_lib()
        box = ["/bn_amd_%s" % uuid.uuid4().hex[:16] if rank == 0 else None]
        if dist is not None:
            dist.broadcast_object_list(box, src=0)
        self.name = box[0]
        self.world, self.rank = world, rank
        self.handle = C.c_void_p()
        if rank == 0:
            self._open(L, 1)
        if dist is not None:
            dist.barrier()  # the segment exists (and is zeroed) before anyone else maps it
        if rank != 0:
            self._open(L, 0)
        if dist is not None:
            dist.barrier()

    def _open(self, L, create):
        rc = L.bnh_shm_open(self.name.encode(), self.world, self.rank, create, C.byref(self.handle))
        if rc != 0:
            raise BnError(rc, L.bnh_last_error().decode())

    def allgather_words(self, words):
        """words: list of < 8 ints (64-bit).  Returns [rank][i]."""
        n = len(words)
        src = (C.c_uint64 * n)(*words)
        dst = (C.c_uint64 * (n * self.world))()
        rc = host_lib().bnh_shm_allgather(self.handle, src, n, dst)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())
        return [[int(dst[w * n + i]) for i in range(n)] for w in range(self.world)]

    def all_gather_scalars(self, vals):
        """128-bit scalars (<= 3): returns [rank][i] like TorchComm.all_gather_scalars."""
        words = []
        for v in vals:
            words += [v & ((1 << 64) - 1), v >> 64]
        per = self.allgather_words(words)
        return [[r[2 * i] | (r[2 * i + 1] << 64) for i in range(len(vals))] for r in per]

    def xor_scalars(self, vals):
        out = [0] * len(vals)
        for r in self.all_gather_scalars(vals):
            for i, v in enumerate(r):
                out[i] ^= v
        return out

    def close(self):
        if self.handle:
            host_lib().bnh_shm_close(self.handle)
            self.handle = C.c_void_p()


class PeerExchange:
    """Device-resident exchange of the round evaluations (include/binius_amd.h bn_peer_*, csrc/finalize.hpp): every rank
    owns a mailbox in fine-grained device memory, hipIpc-mapped into all ranks of the node (peers on the same device on a
    one-GPU box, xGMI peers on a node); the handles travel over the torch.distributed group.  Once connected, a
    SumcheckPlan(..., peer=True) on this context has its local rounds reduced across the ranks inside the kernels."""

    def __init__(self, hal, dist, rank, world):
        from ._ffi import _check

        self.hal, self.world, self.rank = hal, world, rank
        self.created = False
        buf = C.create_string_buffer(64)
        _check(lib().bn_peer_create(hal._h, world, rank, buf))
        self.created = True
        try:
            handles = [None] * world
            dist.all_gather_object(handles, bytes(buf.raw))
            _check(lib().bn_peer_connect(hal._h, b"".join(handles)))
            ok = 1
        except Exception:  # noqa: BLE001 -- every rank has to learn that one of them failed
            ok = 0
        flags = [None] * world
        dist.all_gather_object(flags, ok)
        if not all(flags):
            self.close()
            raise BnError(3, "peer exchange: rank(s) %s could not map the peers' mailboxes" % [i for i, f in enumerate(flags) if not f])
        dist.barrier()  # nobody writes into a mailbox that its owner has not mapped and zeroed

    def rounds(self):
        from ._ffi import _check

        st = (C.c_uint64 * 2)()
        _check(lib().bn_peer_stats(self.hal._h, st))
        return int(st[0])

    def close(self):
        if self.created:
            lib().bn_peer_destroy(self.hal._h)
            self.created = False


class RcclComm:
    """An RCCL communicator owned by the C++ host library (one per process / GPU), bootstrapped over
    an existing torch.distributed group: rank 0 creates the unique id, everyone joins."""

    def __init__(self, dist, rank, world):
        import torch

        L = host_lib()
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if not os.path.exists(path):
            path = "librccl.so"
        rc = L.bnh_rccl_open(path.encode())
        if rc != 0:
            raise BnError(rc, L.bnh_last_error().decode())
        uid = C.create_string_buffer(128)
        if rank == 0:
            rc = L.bnh_rccl_unique_id(uid)
            if rc != 0:
                raise BnError(rc, L.bnh_last_error().decode())
        box = [bytes(uid.raw)]
        dist.broadcast_object_list(box, src=0)
        uid = C.create_string_buffer(box[0], 128)
        self.handle = C.c_void_p()
        rc = L.bnh_rccl_init(uid, world, rank, C.byref(self.handle))
        if rc != 0:
            raise BnError(rc, L.bnh_last_error().decode())

    def destroy(self):
        if self.handle:
            host_lib().bnh_rccl_destroy(self.handle)
            self.handle = None


class ZerocheckBatchPlan:
    """batch_zerocheck::batch_prove (bnh_zerocheck_batch_prove = binius_amd/host/zerocheck.hpp; crates/core/src/protocols/sumcheck/prove/
    batch_zerocheck.rs:166-293): the batched univariate-skip zerocheck for the domain field B8, the transcript's samples handed in.
    tables: in ascending n_vars, each (n_vars, columns, compositions) with columns = [(DevSlice of the packed column, tower_level 0 or 3)]
    (only read) and compositions = [(steps, steps_of_the_leading_form, degree)] in compile_expr's notation, constants in B8; k =
    skip_rounds; zerocheck_challenges and sumcheck_challenges: max_n - k each; batch_coeffs: one per table; reduction_challenges: k;
    scratch: a device slice of at least scratch_elems(tables, k) elements.  run() returns the proof as a dict: message, round_coeffs (all
    coefficients, padded to max(2, largest degree) + 2), final_evals (per table, the indicator's last), reduction_round_coeffs,
    reduction_final_evals, skipped_challenges, unskipped_challenges, concat_multilinear_evals; phase_ms / phase_calls afterwards.
    tower=True is bnh_zerocheck_batch_prove_tower: every arm of constraint_system/prove.rs:483-490 -- columns at tower_level 0 or 3 .. 7
    (little-endian values of 2^(level - 3) bytes), constants anywhere in B128, a table's arm chosen from its levels; the fold phase's call
    count then includes one bn_fold_right per column above level 3.  With the default the old entry point is called."""

    PHASES = ("univariate", "fold", "multilinear", "projection", "reduction")

    @staticmethod
    def scratch_elems(tables, k, tower=False):
        n = len(tables)
        nv = (C.c_uint32 * max(1, n))(*[t[0] for t in tables])
        nc = (C.c_uint32 * max(1, n))(*[len(t[1]) for t in tables])
        if tower:  # (the formula depends on the levels: a padded column takes what its level needs)
            levels = [c[1] for t in tables for c in t[1]]
            return int(host_lib().bnh_zerocheck_batch_scratch_elems_tower(n, k, nv, nc, (C.c_uint32 * max(1, len(levels)))(*levels)))
        return int(host_lib().bnh_zerocheck_batch_scratch_elems(n, k, nv, nc))

    def __init__(self, hal, tables, k, zerocheck_challenges, batch_coeffs, univariate_challenge, sumcheck_challenges, reduction_batch_coeff,
                 reduction_challenges, scratch, tower=False):
        from ._ffi import make_steps

        self.hal, self.k, self.n, self.tower = hal, k, len(tables), bool(tower)
        self._keep = (tables, scratch)
        self.n_cols = [len(t[1]) for t in tables]
        self.nv = (C.c_uint32 * max(1, self.n))(*[t[0] for t in tables])
        self.nc = (C.c_uint32 * max(1, self.n))(*self.n_cols)
        cols = [c for t in tables for c in t[1]]
        self.ptrs = (C.c_void_p * max(1, len(cols)))(*[(c[0].ptr if c[0] is not None else None) for c in cols])
        self.levels = (C.c_uint32 * max(1, len(cols)))(*[c[1] for c in cols])
        comps = [c for t in tables for c in t[2]]
        self.ncomp = (C.c_uint32 * max(1, self.n))(*[len(t[2]) for t in tables])
        flat, flat_inf = [st for c in comps for st in c[0]], [st for c in comps for st in c[1]]
        self.steps, self.steps_inf = make_steps(flat) if flat else None, make_steps(flat_inf) if flat_inf else None
        self.n_steps = (C.c_uint32 * max(1, len(comps)))(*[len(c[0]) for c in comps])
        self.n_steps_inf = (C.c_uint32 * max(1, len(comps)))(*[len(c[1]) for c in comps])
        self.degrees = (C.c_uint32 * max(1, len(comps)))(*[c[2] for c in comps])
        max_n = max([t[0] for t in tables] + [0])
        self.rounds = max(0, max_n - k)
        d_top = max([c[2] for c in comps] + [0])
        self.msg_len = max(0, (d_top << k) - (1 << k)) if 0 <= k <= 8 and d_top <= 256 else 0
        self.per_round = max(2, min(d_top, 256)) + 2
        self.zc, self.sc = _f128_array(list(zerocheck_challenges) or [0]), _f128_array(list(sumcheck_challenges) or [0])
        self.bc, self.rc = _f128_array(list(batch_coeffs) or [0]), _f128_array(list(reduction_challenges) or [0])
        self.lens = (len(zerocheck_challenges), len(sumcheck_challenges), len(batch_coeffs), len(reduction_challenges))
        self.z, self.rb = to_f128(univariate_challenge), to_f128(reduction_batch_coeff)
        self.scratch = scratch
        total = sum(self.n_cols)
        self.message = (F128 * max(1, self.msg_len))()
        self.coeffs = (F128 * max(1, self.per_round * self.rounds))()
        self.final = (F128 * (total + self.n + 1))()
        self.red_coeffs = (F128 * max(1, 3 * max(0, min(k, 8))))()
        self.red_final = (F128 * (total + 1))()
        self.skipped, self.unskipped = (F128 * max(1, min(k, 8)))(), (F128 * max(1, self.rounds))()
        self.concat = (F128 * max(1, total))()
        self.phase_ms, self.phase_calls = (C.c_double * 5)(), (C.c_uint64 * 5)()

    def run(self):
        if self.lens != (self.rounds, self.rounds, self.n, self.k):
            raise BnError(BN_ERR_INPUT_VALIDATION, "input validation: zerocheck: max_n - k zerocheck and sumcheck challenges, one coefficient per table, k reduction challenges")
        prove = host_lib().bnh_zerocheck_batch_prove_tower if self.tower else host_lib().bnh_zerocheck_batch_prove
        rc = prove(
            self.hal._h, self.n, self.k, self.nv, self.nc, self.ptrs, self.levels, self.ncomp, C.cast(self.steps, C.c_void_p), self.n_steps,
            C.cast(self.steps_inf, C.c_void_p), self.n_steps_inf, self.degrees, self.zc, self.bc, C.byref(self.z), self.sc, C.byref(self.rb), self.rc,
            self.scratch.ptr if self.scratch is not None else None, self.scratch.len if self.scratch is not None else 0, self.message, self.coeffs, self.final,
            self.red_coeffs, self.red_final, self.skipped, self.unskipped, self.concat, self.phase_ms, self.phase_calls)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())
        ints = lambda a, n: [from_f128(a[i]) for i in range(n)]  # noqa: E731
        finals, at = [], 0
        for m in self.n_cols:
            finals.append(ints(self.final, at + m + 1)[at:])
            at += m + 1
        total = sum(self.n_cols)
        return {
            "message": ints(self.message, self.msg_len),
            "round_coeffs": [ints(self.coeffs, self.per_round * (r + 1))[self.per_round * r:] for r in range(self.rounds)],
            "final_evals": finals,
            "reduction_round_coeffs": [ints(self.red_coeffs, 3 * (r + 1))[3 * r:] for r in range(self.k)],
            "reduction_final_evals": ints(self.red_final, total + 1),
            "skipped_challenges": ints(self.skipped, self.k), "unskipped_challenges": ints(self.unskipped, self.rounds),
            "concat_multilinear_evals": ints(self.concat, total),
        }

    def phases(self):
        return {name: (float(self.phase_ms[i]), int(self.phase_calls[i])) for i, name in enumerate(self.PHASES)}


class WitnessPlan:
    """The virtual columns of a constraint system derived on the device (bnh_witness_derive = binius_amd/host/witness.hpp): the
    witness-side reading of a MultilinearOracleSet (multilinear.rs of core's oracle module).  columns, in oracle-id order, each one of
      ("given", DevSlice, tower_level, n_vars)
      ("shifted", inner, block_size, shift_offset, variant)       variant: "circular_left" / "logical_left" / "logical_right" or 0 / 1 / 2
      ("repeating", inner, log_count)
      ("zero_padded", inner, n_pad_vars, start_index, nonzero_index)
      ("packed", inner, log_degree)                               an alias: the inner's pointer, no launch
      ("lincomb", [(inner, coeff), ...], offset, n_vars)          coefficients and offset as ints
    with inner an index smaller than the column's own.  scratch: a device slice of at least scratch_elems(columns) elements.  run()
    returns [(DevSlice, tower_level, n_vars)] per column; n_waves and n_launches afterwards."""

    KINDS = {"given": 0, "shifted": 1, "repeating": 2, "zero_padded": 3, "packed": 4, "lincomb": 5}
    VARIANTS = {"circular_left": 0, "logical_left": 1, "logical_right": 2}

    @classmethod
    def _marshal(cls, columns):
        desc, args, given, terms, coeffs, offsets = [], [], [], [], [], []
        for c in columns:
            kind = cls.KINDS.get(c[0], c[0])
            d, arg, ptr, off = [0, 0, 0], 0, None, 0
            if kind == 0:
                ptr, d = (c[1].ptr if c[1] is not None else None), [c[2], c[3], 0]
            elif kind == 1:
                d, arg = [c[1], c[2], cls.VARIANTS.get(c[4], c[4])], c[3]
            elif kind in (2, 4):
                d = [c[1], c[2], 0]
            elif kind == 3:
                d, arg = [c[1], c[2], c[3]], c[4]
            elif kind == 5:
                d, off = [len(terms), len(c[1]), c[3]], c[2]
                terms += [t[0] for t in c[1]]
                coeffs += [t[1] for t in c[1]]
            desc += [kind] + [int(x) for x in d]
            args.append(int(arg))
            given.append(ptr)
            offsets.append(off)
        n = len(columns)
        return (n, (C.c_uint32 * max(1, 4 * n))(*desc), (C.c_uint64 * max(1, n))(*args), (C.c_void_p * max(1, n))(*given),
                (C.c_uint32 * max(1, len(terms)))(*terms), _f128_array(coeffs or [0]), len(terms), _f128_array(offsets or [0]))

    @classmethod
    def scratch_elems(cls, columns):
        n, desc, args, _given, terms, coeffs, n_terms, offsets = cls._marshal(columns)
        return int(host_lib().bnh_witness_derive_scratch_elems(n, desc, args, terms, coeffs, n_terms, offsets))

    def __init__(self, hal, columns, scratch):
        self.hal, self.scratch, self._keep = hal, scratch, columns
        self.n, self.desc, self.args, self.given, self.terms, self.coeffs, self.n_terms, self.offsets = self._marshal(columns)
        self.ptrs = (C.c_void_p * max(1, self.n))()
        self.levels, self.n_vars = (C.c_uint32 * max(1, self.n))(), (C.c_uint32 * max(1, self.n))()
        self._waves, self._launches = C.c_uint32(0), C.c_uint32(0)

    def run(self):
        from ._ffi import DevSlice

        rc = host_lib().bnh_witness_derive(self.hal._h, self.n, self.desc, self.args, self.given, self.terms, self.coeffs, self.n_terms, self.offsets,
                                           self.scratch.ptr if self.scratch is not None else None, self.scratch.len if self.scratch is not None else 0,
                                           self.ptrs, self.levels, self.n_vars, C.byref(self._waves), C.byref(self._launches))
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())
        return [(DevSlice(self.ptrs[i], max(1, (1 << (self.n_vars[i] + self.levels[i])) >> 7)), int(self.levels[i]), int(self.n_vars[i])) for i in range(self.n)]

    @property
    def n_waves(self):
        return int(self._waves.value)

    @property
    def n_launches(self):
        return int(self._launches.value)


class WitnessBuild:
    """WitnessPlan with the columns that a few integers, one field element or a 0/1 projection determine generated on the device as
    well (bnh_witness_build = witness_build of binius_amd/host/witness.hpp, over bn_generate_columns_batch).  columns: WitnessPlan's, and
      ("projected_bits", inner, start_index, query_size, query_bits)   add_projected / add_selected at query values ZERO / ONE
      ("constant", tower_level, n_vars, value)
      ("step_down", n_vars, index) / ("step_up", n_vars, index) / ("select_row", n_vars, index)     B1 columns
      ("incrementing", tower_level, n_vars)
      ("powers", tower_level, n_vars, base)
    A generated column without an inner is wave 0; every wave with generated columns makes one more launch.  run(), n_waves and
    n_launches as WitnessPlan's."""

    KINDS = dict(WitnessPlan.KINDS, projected_bits=6, constant=7, step_down=8, step_up=9, select_row=10, incrementing=11, powers=12)
    VARIANTS = WitnessPlan.VARIANTS
    _SCRATCH, _RUN = "bnh_witness_build_scratch_elems", "bnh_witness_build"

    @classmethod
    def _marshal(cls, columns):
        """WitnessPlan's marshalling of the kinds 0 .. 5 (their rows are taken from it), the further kinds encoded here."""
        old = [c if cls.KINDS.get(c[0], c[0]) <= 5 else ("packed", 0, 0) for c in columns]
        n, desc, args, given, terms, coeffs, n_terms, offsets = WitnessPlan._marshal(old)
        for i, c in enumerate(columns):
            kind = cls.KINDS.get(c[0], c[0])
            if kind <= 5:
                continue
            d, arg, value = [0, 0, 0], 0, 0
            if kind == 6:
                d, arg = [c[1], c[2], c[3]], c[4]
            elif kind == 7:
                d, value = [c[1], c[2], 0], c[3]
            elif kind in (8, 9, 10):
                d, arg = [0, c[1], 0], c[2]
            elif kind == 11:
                d = [c[1], c[2], 0]
            elif kind == 12:
                d, value = [c[1], c[2], 0], c[3]
            desc[4 * i : 4 * i + 4] = [kind] + [int(x) for x in d]
            args[i] = int(arg)
            offsets[i].lo, offsets[i].hi = int(value) & ((1 << 64) - 1), int(value) >> 64
        return n, desc, args, given, terms, coeffs, n_terms, offsets

    @classmethod
    def scratch_elems(cls, columns):
        n, desc, args, _given, terms, coeffs, n_terms, offsets = cls._marshal(columns)
        return int(getattr(host_lib(), cls._SCRATCH)(n, desc, args, terms, coeffs, n_terms, offsets))

    def __init__(self, hal, columns, scratch):
        self.hal, self.scratch, self._keep = hal, scratch, columns
        self.n, self.desc, self.args, self.given, self.terms, self.coeffs, self.n_terms, self.offsets = self._marshal(columns)
        self.ptrs = (C.c_void_p * max(1, self.n))()
        self.levels, self.n_vars = (C.c_uint32 * max(1, self.n))(), (C.c_uint32 * max(1, self.n))()
        self._waves, self._launches = C.c_uint32(0), C.c_uint32(0)

    def run(self):
        from ._ffi import DevSlice

        rc = getattr(host_lib(), self._RUN)(self.hal._h, self.n, self.desc, self.args, self.given, self.terms, self.coeffs, self.n_terms, self.offsets,
                                            self.scratch.ptr if self.scratch is not None else None, self.scratch.len if self.scratch is not None else 0,
                                            self.ptrs, self.levels, self.n_vars, C.byref(self._waves), C.byref(self._launches))
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())
        return [(DevSlice(self.ptrs[i], max(1, (1 << (self.n_vars[i] + self.levels[i])) >> 7)), int(self.levels[i]), int(self.n_vars[i])) for i in range(self.n)]

    @property
    def n_waves(self):
        return int(self._waves.value)

    @property
    def n_launches(self):
        return int(self._launches.value)


class WitnessCompute(WitnessBuild):
    """WitnessBuild with the columns of m3's add_computed computed on the device as well (bnh_witness_compute = witness_compute of
    binius_amd/host/witness.hpp): each is one bn_compute_composite with a tower-typed expression.  columns: WitnessBuild's, and
      ("computed", steps, [inputs], n_vars, tower_level)   steps as Context.compile_expr takes them; variable v is column inputs[v]
    ("lincomb", ...) is unchanged, but a combination that is neither in XOR form nor a B128 one now runs as the expression sum of
    coeff * term + offset at its own level instead of being rejected.  run(), n_waves and n_launches as WitnessPlan's."""

    KINDS = dict(WitnessBuild.KINDS, computed=13)
    _SCRATCH, _RUN = "bnh_witness_compute_scratch_elems", "bnh_witness_compute"

    @classmethod
    def _marshal_exprs(cls, columns):
        """(columns with every computed column replaced by a placeholder, its rows, the expression tables)"""
        from ._ffi import make_steps

        flat, step_off, inputs, input_off, rows = [], [0], [], [0], {}
        for i, c in enumerate(columns):
            if cls.KINDS.get(c[0], c[0]) != 13:
                continue
            rows[i] = [13, len(step_off) - 1, int(c[3]), int(c[4])]
            flat += list(c[1])
            inputs += [int(v) for v in c[2]]
            step_off.append(len(flat))
            input_off.append(len(inputs))
        U32 = C.c_uint32
        tables = (make_steps(flat), (U32 * len(step_off))(*step_off), (U32 * max(1, len(inputs)))(*inputs), (U32 * len(input_off))(*input_off), len(step_off) - 1)
        return [("packed", 0, 0) if i in rows else c for i, c in enumerate(columns)], rows, tables

    @classmethod
    def _marshal(cls, columns):
        plain, rows, _tables = cls._marshal_exprs(columns)
        out = WitnessBuild._marshal.__func__(cls, plain)
        for i, row in rows.items():
            out[1][4 * i : 4 * i + 4] = row
        return out

    @classmethod
    def scratch_elems(cls, columns):
        n, desc, args, _given, terms, coeffs, n_terms, offsets = cls._marshal(columns)
        return int(host_lib().bnh_witness_compute_scratch_elems(n, desc, args, terms, coeffs, n_terms, offsets, *cls._marshal_exprs(columns)[2]))

    def __init__(self, hal, columns, scratch):
        super().__init__(hal, columns, scratch)
        self.exprs = self._marshal_exprs(columns)[2]

    def run(self):
        from ._ffi import DevSlice

        rc = getattr(host_lib(), self._RUN)(self.hal._h, self.n, self.desc, self.args, self.given, self.terms, self.coeffs, self.n_terms, self.offsets,
                                            self.scratch.ptr if self.scratch is not None else None, self.scratch.len if self.scratch is not None else 0,
                                            self.ptrs, self.levels, self.n_vars, C.byref(self._waves), C.byref(self._launches), *self.exprs)
        if rc != 0:
            raise BnError(rc, host_lib().bnh_last_error().decode())
        return [(DevSlice(self.ptrs[i], max(1, (1 << (self.n_vars[i] + self.levels[i])) >> 7)), int(self.levels[i]), int(self.n_vars[i])) for i in range(self.n)]


class WitnessComputeBatched(WitnessCompute):
    """WitnessCompute with the expression columns of a wave in one launch (bnh_witness_compute_batched = witness_compute_batched of
    binius_amd/host/witness.hpp, over Context.expr_compile_tower_batch's op): the same columns, bytes and rejections; n_launches counts
    one per wave that has expression columns.  scratch_elems is WitnessCompute's."""

    _RUN = "bnh_witness_compute_batched"
