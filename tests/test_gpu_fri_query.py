"""The FRI query phase on the device (bn_fri_query_openings behind FRIFolder::finish_proof, bnh_fri_prove and
bnh_piop_prove_committed_open): every opening of a proof from ONE launch.  The checker is the oracle's codewords and
oracle.merkle_build trees (the Python prover of tests/fri_verify_ref.py) and the verifier restated there, never the code under test.
Shapes: the smallest at which each part of the kernel can go wrong (fri_verify_ref.SHAPES)."""
import numpy as np
import pytest

import fri_verify_ref as fv

pytestmark = pytest.mark.gpu

SHAPES = [p for p, _ in fv.SHAPES]


@pytest.fixture(scope="module")
def hal():
    import binius_amd

    ctx = binius_amd.Context(0, 1 << 20)
    yield ctx
    ctx.close()


def upload(hal, alloc, a):
    d = alloc.alloc(a.shape[0])
    hal.copy_h2d(a, d)
    return d


def host_params(p):
    from binius_amd._host import FRIParams

    return FRIParams(p.log_dim, p.log_inv_rate, p.log_batch_size, list(p.fold_arities), p.n_test_queries)


def moved(before, after):
    return {k: after[k] - before[k] for k in before}


@pytest.mark.parametrize("p", SHAPES, ids=fv.SHAPE_IDS)
def test_fri_prove_matches_the_python_prover_and_verifies(hal, oracle, p):
    """bnh_fri_prove: roots and advice byte-equal to the Python prover's on the same message, challenges and indices; the advice is
    accepted by the restated verifier; the query phase is exactly one launch."""
    from binius_amd._host import FriProvePlan

    message, chs, idx, pr = fv.case(oracle, p)
    alloc = hal.dev_alloc()
    d_msg = upload(hal, alloc, message)
    scratch = alloc.alloc(4 << (p.log_dim + p.log_batch_size + p.log_inv_rate))  # codewords and trees: small arities need more than twice the codeword
    plan = FriProvePlan(hal, host_params(p), d_msg, scratch, chs, idx)
    before = hal.fri_query_counters()
    plan.run()
    assert moved(before, hal.fri_query_counters()) == {"calls": 1, "launches": 1, "openings": p.n_test_queries * p.n_oracles()}
    roots = [bytes(r) for r in plan.roots]
    assert roots == pr.commitments
    assert plan.advice.shape[0] == p.layout()[2]
    assert np.array_equal(plan.advice, pr.advice)
    assert np.array_equal(plan.terminate, pr.codewords[-1])
    fv.verify(oracle, p, roots[0], roots[1:], chs, idx, plan.advice)


class Resident:
    """the oracle's codewords of a shape on the device, their trees built there (bn_merkle_build)"""

    def __init__(self, hal, oracle, p):
        self.hal, self.p = hal, p
        _message, _chs, self.idx, self.pr = fv.case(oracle, p)
        alloc = hal.dev_alloc()
        self.codewords = [upload(hal, alloc, c) for c in self.pr.codewords]
        self.trees = []
        coset_log = list(p.fold_arities) + [p.n_final_challenges()] if p.fold_arities else [p.log_dim + p.log_batch_size]
        for d_code, cl in zip(self.codewords, coset_log):
            nodes = alloc.alloc(2 * (2 * (d_code.len >> cl) - 1))
            hal.merkle_build(d_code, 1 << cl, nodes)
            self.trees.append(nodes)
        self.alloc = alloc
        self.oracles = [(self.codewords[i], self.trees[i]) + o for i, o in enumerate(host_params(p).query_oracles())]
        self.terminate = self.codewords[-1]

    def per_opening_route(self, indices):
        """What FRIFolder::finalize, vcs_optimal_layers and one FRIQueryProver::prove_query per index read back: a copy_d2h per
        terminate codeword, layer and coset, a bn_gather_d2h per branch (BinaryMerkleTree::branch)."""
        hal, p = self.hal, self.p
        parts = [hal.copy_d2h(self.terminate)]
        for _code, nodes, L, _arity, depth, _shift in self.oracles:
            start = (2 << L) - (2 << depth)
            parts.append(hal.copy_d2h(nodes.slice(2 * start, 2 * (start + (1 << depth)))))
        for index in indices:
            for code, nodes, L, arity, depth, shift in self.oracles:
                ci = index >> shift
                parts.append(hal.copy_d2h(code.slice(ci << arity, (ci + 1) << arity)))
                ids = [(((1 << j) - 1) << (L + 1 - j)) | ((ci >> j) ^ 1) for j in range(L - depth)]
                if ids:
                    parts.append(hal.gather_d2h(nodes, [2 * i for i in ids], 2).reshape(-1, 2))
        return np.concatenate(parts)


@pytest.mark.parametrize("p", SHAPES, ids=fv.SHAPE_IDS)
def test_openings_equal_the_per_opening_route(hal, oracle, p):
    r = Resident(hal, oracle, p)
    before = hal.fri_query_counters()
    got = hal.fri_query_openings(r.oracles, r.terminate, r.idx, p.index_bits())
    assert moved(before, hal.fri_query_counters()) == {"calls": 1, "launches": 1, "openings": p.n_test_queries * p.n_oracles()}
    assert np.array_equal(got, r.per_opening_route(r.idx))
    assert np.array_equal(got, r.pr.advice)


def test_header_alone_and_staging_growth(oracle):
    """No query and no oracle still copy the header; a block larger than the staging of the calls before it (64 KiB at first) grows
    the staging, and the calls after it are served from the grown buffer."""
    import binius_amd

    p = SHAPES[5]
    with binius_amd.Context(0, 1 << 18) as hal:
        r = Resident(hal, oracle, p)
        header = p.layout()[0]
        assert np.array_equal(hal.fri_query_openings(r.oracles, r.terminate, [], p.index_bits()), r.pr.advice[:header])
        assert np.array_equal(hal.fri_query_openings([], r.terminate, [0, 0], 0), r.pr.codewords[-1])
        assert hal.fri_query_counters() == {"calls": 2, "launches": 2, "openings": 0}
        top = (1 << p.index_bits()) - 1
        many = [0, top] + [int(w) & top for w in oracle.splitmix_words(0x9A0, 398)]
        assert 16 * (header + len(many) * p.layout()[1]) > 4 * (1 << 16)
        # (the layers stay at the depths of the committed proof: the descriptors say which layer, not the number of queries)
        want = fv.advice_block(p, r.pr.codewords, r.pr.trees, many)
        assert np.array_equal(hal.fri_query_openings(r.oracles, r.terminate, many, p.index_bits()), want)
        assert np.array_equal(hal.fri_query_openings(r.oracles, r.terminate, r.idx, p.index_bits()), r.pr.advice)
        assert hal.fri_query_counters() == {"calls": 4, "launches": 4, "openings": (len(many) + p.n_test_queries) * p.n_oracles()}


def _deferred_fold_case(oracle, state):
    import deferred_states as ds

    p = SHAPES[0]
    _message, _chs, idx, pr = fv.case(oracle, p)
    code = np.array(pr.codewords[0])
    log_n = code.shape[0].bit_length()  # the prover's first multilinear folds to the codeword
    diff = oracle.random_b128(0xD1FF, code.shape[0])
    box = {}

    def stage(pv, st):
        z = st.challenges[0]
        # lo + z (hi - lo) = code  <=>  lo = code + z * hi' with hi' = hi - lo chosen at random
        lo = np.array(code)
        lo ^= oracle.ints_to_arr([oracle.mul(z, d) for d in fv.ints(diff)])
        hi = lo ^ diff
        folded = lo.copy()
        assert oracle.extrapolate_line(folded, hi.copy(), z) == 0 and np.array_equal(folded, code)
        st.inputs[0].host[:] = np.concatenate([lo, hi])
        box["nodes"] = st.take(fv.units(pr.trees[0]).shape[0], "tree")
        box["nodes"].host[:] = fv.units(pr.trees[0])
        box["term"] = st.take(pr.codewords[-1].shape[0], "terminate")
        box["term"].host[:] = pr.codewords[-1]

    hal = ds.make_context(state, ds.region_elems(3, log_n) + 4096)
    try:
        st = ds.reach(hal, oracle, state, seed=0xF01D, stage=stage, log_n=log_n)
        e0 = st.live[0]
        assert np.array_equal(e0.host, code), "the model's fold is not the codeword"
        o = host_params(p).query_oracles()[0]
        got = hal.fri_query_openings([(e0.dev, box["nodes"].dev) + o], box["term"].dev, idx, p.index_bits())
        st.continuation()
        st.check_bytes()
    finally:
        hal.close()
    depth, arity, L = o[2], o[1], o[0]
    want = [pr.codewords[-1], fv.units(fv.tree_layer(pr.trees[0], depth))]
    for i in idx:
        want.append(code[i << arity : (i + 1) << arity])
        want.append(fv.units(np.stack(fv.tree_branch(pr.trees[0], i, depth))))
    assert L - depth > 0 and np.array_equal(got, np.concatenate(want))


def test_deferred_fold_on_the_codeword_is_visible(oracle):
    """On the context's own stream bn_extrapolate_line_batch is left deferred -- pending in the single-claim state (S1) or parked as
    a claim-group fold (S2), reached and proven by tests/deferred_states.py; the openings that follow read the folded codeword."""
    for state in ("S1", "S2"):
        _deferred_fold_case(oracle, state)


def test_rejections_launch_nothing_and_count_nowhere(hal, oracle):
    from binius_amd import BnError, DevSlice
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION, FRI_QUERY_MAX_ORACLES

    p = SHAPES[0]
    r = Resident(hal, oracle, p)
    before = hal.fri_query_counters()
    bits, total = p.index_bits(), p.layout()[2]

    def rejected(oracles, terminate, indices, index_bits, out_elems=None, text=None):
        with pytest.raises(BnError) as e:
            hal.fri_query_openings(oracles, terminate, indices, index_bits, out_elems=out_elems)
        assert e.value.code == BN_ERR_INPUT_VALIDATION, str(e.value)
        if text:
            assert text in str(e.value)
        assert hal.fri_query_counters() == before

    def with_oracle0(**kw):
        names = ("code", "nodes", "log_n_cosets", "log_coset_size", "layer_depth", "index_shift")
        o = dict(zip(names, r.oracles[0]))
        o.update(kw)
        return [tuple(o[n] for n in names)] + r.oracles[1:]

    rejected(with_oracle0(code=None), r.terminate, r.idx, bits, out_elems=total, text="null")
    rejected(with_oracle0(nodes=None), r.terminate, r.idx, bits, out_elems=total, text="null")
    rejected(r.oracles, DevSlice(0, r.terminate.len), r.idx, bits, out_elems=total, text="null")
    rejected(with_oracle0(code=DevSlice(r.oracles[0][0].ptr + 8, 8)), r.terminate, r.idx, bits, out_elems=total, text="aligned")
    rejected(r.oracles, DevSlice(r.terminate.ptr + 4, r.terminate.len), r.idx, bits, text="aligned")
    rejected(r.oracles, r.terminate, [0, 1 << bits, 1], bits, text="IndexOutOfRange")
    rejected(r.oracles, r.terminate, [0, (1 << 64) - 1, 1], bits, text="IndexOutOfRange")
    rejected(r.oracles, r.terminate, r.idx, bits + 1, text="index_shift")  # indices of bits + 1 bits would leave oracle 0
    rejected(with_oracle0(index_shift=bits + 1), r.terminate, r.idx, bits, text="index_shift")
    rejected(with_oracle0(layer_depth=r.oracles[0][2] + 1), r.terminate, r.idx, bits, out_elems=total, text="IncorrectLayerDepth")
    rejected(r.oracles, r.terminate, r.idx, bits, out_elems=total - 1, text="out_elems")
    rejected(r.oracles, r.terminate, r.idx, bits, out_elems=total + 1, text="out_elems")
    rejected([r.oracles[0]] * (FRI_QUERY_MAX_ORACLES + 1), r.terminate, r.idx, bits, out_elems=total, text="BN_FRI_QUERY_MAX_ORACLES")
    rejected(r.oracles, DevSlice(r.terminate.ptr, (1 << 26) + 1), r.idx, bits, out_elems=1, text="too many elements")
    # and the call that is accepted after all of them
    assert np.array_equal(hal.fri_query_openings(r.oracles, r.terminate, r.idx, bits), r.pr.advice)


def test_advice_buffer_too_small_is_rejected(hal, oracle):
    from binius_amd import BnError
    from binius_amd._ffi import BN_ERR_INPUT_VALIDATION
    from binius_amd._host import FriProvePlan

    p = SHAPES[0]
    message, chs, idx, _pr = fv.case(oracle, p)
    alloc = hal.dev_alloc()
    d_msg = upload(hal, alloc, message)
    scratch = alloc.alloc(4 << (p.log_dim + p.log_batch_size + p.log_inv_rate))  # codewords and trees: small arities need more than twice the codeword
    with pytest.raises(BnError) as e:
        FriProvePlan(hal, host_params(p), d_msg, scratch, chs, idx, max_advice_elems=p.layout()[2] - 1).run()
    assert e.value.code == BN_ERR_INPUT_VALIDATION
    with pytest.raises(BnError) as e:
        FriProvePlan(hal, host_params(p), d_msg, scratch, chs, idx[:-1] + [1 << p.index_bits()]).run()
    assert e.value.code == BN_ERR_INPUT_VALIDATION and "IndexOutOfRange" in str(e.value)


@pytest.mark.parametrize("n_varss", [[6, 6, 8, 9], [7]], ids=["vars_6_6_8_9", "vars_7"])
def test_piop_prove_committed_open(oracle, n_varss):
    """bnh_piop_prove_committed_open on the reference's own core/tests/piop.rs shape and on one committed multilinear: the item list
    of bnh_piop_prove_committed, an advice the restated FRI verifier accepts, and a final value equal to the piecewise evaluation of
    the committed evaluations (piop/verify.rs:343-358) -- the whole of piop::verify."""
    import binius_amd
    from binius_amd._host import PiopCommit, PiopCommittedOpenPlan, PiopCommittedPlan, piop_commit_elems
    from oracle import piop_ref
    from piop_verify import make_instance, optimal_params, piecewise, verify_transcript

    log_inv_rate = 1
    meta = piop_ref.CommitMeta.with_vars(n_varss)
    op = optimal_params(meta.total_vars, log_inv_rate)
    p = fv.Params(op.log_dim, op.log_inv_rate, op.log_batch_size, tuple(op.fold_arities), op.n_test_queries)
    hp = host_params(p)
    committed, transparents, claims = make_instance(oracle, n_varss, 1, 0x0FE2 + sum(n_varss))
    t_sizes = [t.shape[0].bit_length() - 1 for t in transparents]
    n_sizes = len(set(n_varss))
    stream = oracle.random_scalars(0x7A1 + len(n_varss), n_sizes + meta.total_vars)
    batch_coeffs, challenges = stream[:n_sizes], stream[n_sizes:]
    idx = fv.query_indices(oracle, p, seed=1)
    code_elems, tree_elems = piop_commit_elems(hp)
    ml_elems = sum(x.shape[0] for x in committed) + sum(x.shape[0] for x in transparents)
    with binius_amd.Context(0, code_elems + tree_elems + 2 * ml_elems + 4 * code_elems + (1 << 16)) as hal:
        alloc = hal.dev_alloc()
        d_c = [(v, upload(hal, alloc, x)) for v, x in zip(n_varss, committed)]
        d_t = [(v, upload(hal, alloc, x)) for v, x in zip(t_sizes, transparents)]
        codeword, tree = alloc.alloc(code_elems), alloc.alloc(tree_elems)
        scratch = alloc.alloc(3 * code_elems + ml_elems + (1 << 14))
        commit = PiopCommit(hal, d_c, hp, codeword, tree)
        commit.run()
        plain = PiopCommittedPlan(hal, d_c, d_t, claims, hp, codeword, tree, scratch, batch_coeffs, challenges)
        plain.run()
        want_items = plain.transcript()
        plan = PiopCommittedOpenPlan(hal, d_c, d_t, claims, hp, codeword, tree, scratch, batch_coeffs, challenges, idx)
        before = hal.fri_query_counters()
        plan.run()
        assert moved(before, hal.fri_query_counters()) == {"calls": 1, "launches": 1, "openings": p.n_test_queries * p.n_oracles()}
        items, advice = plan.transcript(), np.array(plan.advice)
    assert items == want_items
    verify_transcript(oracle, piop_ref, n_varss, committed, transparents, claims, op, batch_coeffs, challenges, items)
    assert advice.shape[0] == p.layout()[2]
    terminate = [pl for k, pl in items if k == "fri_terminate"][0]
    assert fv.ints(advice[: p.terminate_len()]) == terminate
    round_commitments = [pl for k, pl in items if k == "fri_commitment"]
    final = fv.verify(oracle, p, commit.commitment, round_commitments, challenges, idx, advice)
    # evaluate_piecewise_multilinear of the committed evaluations at the challenges (piop/verify.rs:343-358)
    piece_evals = []
    sizes = [v for v in range(meta.max_n_vars() + 1) if meta.n_multilins_by_vars[v]]
    for v, payload in zip(sizes, [pl for k, pl in items if k == "multilinear_evals"]):
        piece_evals += payload[: meta.n_multilins_by_vars[v]]
    piece_evals.reverse()
    assert final == piecewise(oracle, challenges, meta.n_multilins_by_vars, piece_evals)
