"""piop::commit apart from piop::prove (bnh_piop_commit + bnh_piop_prove_committed = PiopCommit + PiopCommittedPlan): the commitment,
the codeword and tree left in the caller's buffers and the whole transcript against the oracle's restatement, at the shapes of
tests/test_gpu_group.py::test_piop_prove_vs_oracle that still commit in rounds; two proves from ONE commit; bad arguments."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(12, 1, 3, [4, 4]), (9, 2, 0, [3, 2]), (10, 1, 2, [])]


class env:
    """environment switches that bn_ctx_create reads, for the contexts created inside the block"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_INST, _ORACLE = {}, {}


def instance(oracle, n, log_inv_rate, log_batch, arities):
    """committed multilinears of n-3, n-3, n-1 and n variables, two transparents per size, a claim for every pair of equal size"""
    from binius_amd._host import FRIParams
    from oracle import piop_ref

    key = (n, log_inv_rate, log_batch, tuple(arities))
    if key not in _INST:
        n_varss = [n - 3, n - 3, n - 1, n]
        meta = piop_ref.CommitMeta.with_vars(n_varss)
        p = FRIParams(meta.total_vars - log_batch, log_inv_rate, log_batch, arities, n_test_queries=3)
        seed = 0xC0317 + 977 * n
        committed = [oracle.random_b128(seed + 16 * i, 1 << v) for i, v in enumerate(n_varss)]
        t_sizes = [v for v in sorted(set(n_varss)) for _ in range(2)]
        transparents = [oracle.random_b128(seed + 0x1000 + 16 * j, 1 << v) for j, v in enumerate(t_sizes)]
        claims = []
        for i, c in enumerate(committed):
            for j, t in enumerate(transparents):
                if c.shape[0] == t.shape[0]:
                    rc, s = oracle.inner_product(c, 7, t)
                    assert rc == 0
                    claims.append((c.shape[0].bit_length() - 1, i, j, s))
        n_sizes = len(set(n_varss))
        streams = []
        for s in (0, 1):
            st = oracle.random_scalars(0x7A0 + n + 0x100 * s, n_sizes + meta.total_vars)
            streams.append((st[:n_sizes], st[n_sizes:]))
        for x in committed + transparents:
            x.setflags(write=False)
        _INST[key] = dict(n_varss=n_varss, t_sizes=t_sizes, meta=meta, p=p, committed=committed, transparents=transparents, claims=claims, streams=streams)
    return _INST[key]


def oracle_prove(inst, key, stream):
    from oracle import piop_ref

    if (key, stream) not in _ORACLE:
        bcs, chs = inst["streams"][stream]
        _ORACLE[(key, stream)] = piop_ref.piop_prove([np.array(x) for x in inst["committed"]], [np.array(x) for x in inst["transparents"]], inst["claims"],
                                                     inst["p"], bcs, chs)
    return _ORACLE[(key, stream)]


def upload(hal, alloc, arr):
    d = alloc.alloc(arr.shape[0])
    hal.copy_h2d(arr, d)
    return d


class Session:
    """a context with the instance uploaded and the commit's buffers allocated"""

    def __init__(self, inst):
        import binius_amd
        from binius_amd._host import piop_commit_elems

        self.inst = inst
        self.code_elems, self.tree_elems = piop_commit_elems(inst["p"])
        ml_elems = sum(x.shape[0] for x in inst["committed"]) + sum(x.shape[0] for x in inst["transparents"])
        self.scratch_elems = 3 * self.code_elems + ml_elems + (1 << 14)
        self.hal = binius_amd.Context(0, self.code_elems + self.tree_elems + 2 * ml_elems + self.scratch_elems + (1 << 12))
        alloc = self.hal.dev_alloc()
        self.d_c = [(v, upload(self.hal, alloc, x)) for v, x in zip(inst["n_varss"], inst["committed"])]
        self.d_t = [(v, upload(self.hal, alloc, x)) for v, x in zip(inst["t_sizes"], inst["transparents"])]
        self.codeword, self.tree = alloc.alloc(self.code_elems), alloc.alloc(self.tree_elems)
        self.scratch = alloc.alloc(self.scratch_elems)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.hal.close()

    def commit(self):
        from binius_amd._host import PiopCommit

        c = PiopCommit(self.hal, self.d_c, self.inst["p"], self.codeword, self.tree)
        c.run()
        return c

    def prove(self, stream):
        from binius_amd._host import PiopCommittedPlan

        bcs, chs = self.inst["streams"][stream]
        plan = PiopCommittedPlan(self.hal, self.d_c, self.d_t, self.inst["claims"], self.inst["p"], self.codeword, self.tree, self.scratch, bcs, chs)
        plan.run()
        return plan.transcript()


def assert_transcript(got, items):
    assert [k for k, _ in got] == [k for k, _ in items]
    for idx, ((k, a), (_, b)) in enumerate(zip(got, items)):
        assert a == b, "transcript item %d (%s) differs from the oracle" % (idx, k)


@pytest.mark.parametrize("group", [1, 0])
@pytest.mark.parametrize("n,log_inv_rate,log_batch,arities", SHAPES)
def test_commit_then_prove_vs_oracle(oracle, n, log_inv_rate, log_batch, arities, group):
    inst = instance(oracle, n, log_inv_rate, log_batch, arities)
    with env(BN_GROUP=group):
        with Session(inst) as s:
            c = s.commit()
            assert s.hal.merge_counters()["calls"] == 1 and s.hal.merge_counters()["launches"] == 1
            got = s.prove(0)
    commitment, items, _evals, _terminate = oracle_prove(inst, (n, log_inv_rate, log_batch, tuple(arities)), 0)
    assert c.commitment == commitment
    assert_transcript(got, items)


@pytest.mark.parametrize("n,log_inv_rate,log_batch,arities", SHAPES)
def test_codeword_and_tree_vs_oracle(oracle, n, log_inv_rate, log_batch, arities):
    """What is left in d_codeword and d_tree is piop_ref.fri_commit's codeword and node array (leaves first, root last)."""
    from oracle import piop_ref

    inst = instance(oracle, n, log_inv_rate, log_batch, arities)
    p = inst["p"]
    with Session(inst) as s:
        c = s.commit()
        code = s.hal.copy_d2h(s.codeword)
        nodes = np.ascontiguousarray(s.hal.copy_d2h(s.tree)).view(np.uint8).reshape(-1, 32)
    message = piop_ref.merge_multilins([np.array(x) for x in inst["committed"]], inst["meta"].total_vars)
    want_code, want_nodes = piop_ref.fri_commit(p, oracle.ntt_s_evals(5, p.rs_log_len()), p.rs_log_len(), message)
    assert np.array_equal(code, want_code)
    assert np.array_equal(nodes, want_nodes)
    assert c.commitment == bytes(want_nodes[-1])


def test_two_proves_from_one_commit(oracle):
    """Two PiopCommittedPlan runs from ONE commit with different challenge streams both match the oracle, and the codeword and the
    tree are byte for byte what the commit left: prove only reads them."""
    shape = SHAPES[0]
    inst = instance(oracle, *shape)
    key = (shape[0], shape[1], shape[2], tuple(shape[3]))
    with Session(inst) as s:
        c = s.commit()
        code0, tree0 = s.hal.copy_d2h(s.codeword), s.hal.copy_d2h(s.tree)
        got = [s.prove(0), s.prove(1)]
        assert s.hal.merge_counters()["calls"] == 1
        assert np.array_equal(s.hal.copy_d2h(s.codeword), code0) and np.array_equal(s.hal.copy_d2h(s.tree), tree0)
    for stream in (0, 1):
        commitment, items, _evals, _terminate = oracle_prove(inst, key, stream)
        assert c.commitment == commitment
        assert_transcript(got[stream], items)
    assert got[0] != got[1]


def test_bad_arguments(oracle):
    from binius_amd import BnError, DevSlice
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION
    from binius_amd._host import FRIParams, PiopCommit, piop_commit_elems

    inst = instance(oracle, *SHAPES[1])
    p = inst["p"]
    with Session(inst) as s:
        def rejected(committed, params, codeword, tree, text=None):
            with pytest.raises(BnError) as ei:
                PiopCommit(s.hal, committed, params, codeword, tree).run()
            assert ei.value.code == BN_ERR_INPUT_VALIDATION
            if text:
                assert text in str(ei.value)

        rejected(s.d_c, p, DevSlice(s.codeword.ptr, s.code_elems - 1), s.tree)
        rejected(s.d_c, p, DevSlice(s.codeword.ptr, 2 * s.code_elems), s.tree)
        rejected(s.d_c, p, s.codeword, DevSlice(s.tree.ptr, s.tree_elems - 2))
        rejected(s.d_c[::-1], p, s.codeword, s.tree, "CommittedsNotSorted")
        smaller = FRIParams(p.log_dim - 1, p.log_inv_rate, p.log_batch_size, p.fold_arities, p.n_test_queries)
        code, tree = piop_commit_elems(smaller)
        rejected(s.d_c, smaller, s.codeword.slice(0, code), s.tree.slice(0, tree), "total_vars")
        assert s.hal.merge_counters()["calls"] == 0
        assert s.commit().commitment == oracle_prove(inst, (SHAPES[1][0], SHAPES[1][1], SHAPES[1][2], tuple(SHAPES[1][3])), 0)[0]
