"""The verifier's side of FRI restated as test infrastructure, from the proof bytes alone, and a plain Python prover of the advice
block so that the CPU tests have something to verify.  Shared by tests/test_fri_verify_oracle.py, tests/test_fri_query_abi.py (CPU)
and tests/test_gpu_fri_query.py (device).

Restated:
  FRIVerifier::verify, verify_last_oracle, verify_query_internal        crates/core/src/protocols/fri/verify.rs:99-352
  verify_coset_opening                                                  crates/core/src/protocols/fri/verify.rs:370-394
  verify_vector / verify_layer / verify_opening, fold_digests_vector    crates/core/src/merkle_tree/scheme.rs:67-168
  fold_pair, fold_chunk, fold_interleaved_chunk                         crates/ntt/src/fri.rs:96-245
  vcs_optimal_layers_depths_iter, optimal_verify_layer                  fri/common.rs:174-190, merkle_tree/scheme.rs:47-49
over oracle.groestl256, oracle.groestl256_compress2, oracle.mul and oracle.ntt_get_subspace_eval, with F = BinaryField128b and
FA = BinaryField32b.  The Fiat-Shamir transcript is replaced by what it would have produced (challenges, query indices), as in the
other mirrors.  Every function takes the `oracle` module first, as tests/fri_cases.py does.

The advice block is a (n, 2) uint64 array of 16-byte units in transcript byte order: a field element is one unit (lo, hi), a
digest two.
"""
from collections import namedtuple

import numpy as np

TW_LEVEL = 5  # FA = BinaryField32b


class FriVerifyError(Exception):
    """VerificationError of fri/error.rs and merkle_tree/errors.rs; `kind` is the variant's name."""

    def __init__(self, kind, detail=""):
        super().__init__("%s %s" % (kind, detail))
        self.kind = kind


class Params(namedtuple("Params", "log_dim log_inv_rate log_batch_size fold_arities n_test_queries")):
    """FRIParams (fri/common.rs:25-171)"""

    def rs_log_len(self):
        return self.log_dim + self.log_inv_rate

    def log_len(self):
        return self.rs_log_len() + self.log_batch_size

    def n_fold_rounds(self):
        return self.log_dim + self.log_batch_size

    def n_oracles(self):
        return len(self.fold_arities)

    def index_bits(self):
        return self.log_len() - self.fold_arities[0] if self.fold_arities else 0

    def n_final_challenges(self):
        return self.n_fold_rounds() - sum(self.fold_arities)

    def terminate_len(self):
        return 1 << (self.n_final_challenges() + self.log_inv_rate)

    def optimal_layer_depths(self):
        cap = max(0, self.n_test_queries - 1).bit_length()  # log2_ceil
        log_n_cosets, out = self.log_len(), []
        for arity in self.fold_arities:
            log_n_cosets -= arity
            out.append(min(cap, log_n_cosets))
        return out

    def layout(self):
        """(header, per-query record, total) of the advice in 16-byte units, computed from the protocol alone"""
        header = self.terminate_len() + sum(2 << d for d in self.optimal_layer_depths())
        record, log_n_cosets = 0, self.log_len()
        for arity, depth in zip(self.fold_arities, self.optimal_layer_depths()):
            log_n_cosets -= arity
            record += (1 << arity) + 2 * (log_n_cosets - depth)
        return header, record, header + self.n_test_queries * record


# The shapes of the issue: the smallest at which each part of the opening kernel can go wrong
SHAPES = [
    (Params(6, 1, 2, (3, 2, 1), 3), "unequal arities, the index shift per oracle"),
    (Params(6, 2, 0, (2, 2), 1), "layer depth 0: full-height branches, layer = root"),
    (Params(5, 1, 2, (2, 2, 2), 64), "cap >= tree depth: empty branches, layer = leaves"),
    (Params(7, 1, 2, (7, 1), 5), "128-element coset: a wave loops over > 64 units"),
    (Params(4, 1, 2, (), 4), "no oracle: advice is the whole codeword, no openings"),
    (Params(10, 1, 4, (4, 4, 4), 40), "several workgroups, staging growth"),
]
SHAPE_IDS = ["d%d_r%d_b%d_a%s_q%d" % (p.log_dim, p.log_inv_rate, p.log_batch_size, "x".join(map(str, p.fold_arities)) or "none", p.n_test_queries) for p, _ in SHAPES]


def query_indices(oracle, p, seed=0):
    """0, 2^index_bits - 1, a repeated index, then seeded random ones: n_test_queries in all"""
    top = (1 << p.index_bits()) - 1
    rnd = [int(w) & top for w in oracle.splitmix_words(0x1D1CE5 + 31 * seed + p.log_dim, p.n_test_queries + 1)]
    fixed = [0, top, rnd[0], rnd[0]]
    return (fixed + rnd[1:])[: p.n_test_queries]


# ---------------------------------------------------------------------------------------------- field and digest helpers
def ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 2)
    return [int(a[i, 0]) | (int(a[i, 1]) << 64) for i in range(a.shape[0])]


def units(a):
    """any array of whole 16-byte units as (n, 2) uint64"""
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1, 2)


def digests(u):
    """(2 n, 2) uint64 units -> list of n 32-byte digests"""
    raw = np.ascontiguousarray(u, dtype=np.uint64).tobytes()
    return [raw[i : i + 32] for i in range(0, len(raw), 32)]


def hash_elems(oracle, u):
    """hash_serialize::<F, Groestl256> of field elements: 16 little-endian bytes each"""
    return oracle.groestl256(np.ascontiguousarray(u, dtype=np.uint64).tobytes())


def tensor_expand(oracle, coords):
    """tensor_product_full_query: entry i is the product over j of (coords[j] if bit j of i else 1 + coords[j])"""
    t = [1]
    for r in coords:
        hi = [oracle.mul(x, r) for x in t]
        t = [x ^ h for x, h in zip(t, hi)] + hi
    return t


# ---------------------------------------------------------------------------------------------- ntt/src/fri.rs:96-245
def fold_pair(oracle, s_evals, log_domain, rnd, index, u, v, r):
    t = oracle.ntt_get_subspace_eval(s_evals, log_domain, rnd, index)
    v ^= u
    u ^= oracle.mul(v, t)
    return u ^ oracle.mul(u ^ v, r)  # extrapolate_line_scalar(u, v, r)


def fold_chunk(oracle, s_evals, log_domain, log_len, chunk_index, values, challenges):
    values = list(values)
    log_size = len(challenges)
    assert len(values) == 1 << log_size and log_size <= log_len <= log_domain
    for r in challenges:
        for off in range(1 << (log_size - 1)):
            values[off] = fold_pair(oracle, s_evals, log_domain, log_len, (chunk_index << (log_size - 1)) | off, values[2 * off], values[2 * off + 1], r)
        log_len -= 1
        log_size -= 1
    return values[0]


def fold_interleaved_chunk(oracle, s_evals, log_domain, log_len, log_batch_size, chunk_index, values, tensor, fold_challenges):
    assert len(values) == 1 << (len(fold_challenges) + log_batch_size) and len(tensor) == 1 << log_batch_size
    if log_batch_size == 0:
        scratch = list(values)
    else:
        b = 1 << log_batch_size
        scratch = []
        for c in range(len(values) >> log_batch_size):
            acc = 0
            for a_i, b_i in zip(values[c * b : (c + 1) * b], tensor):
                acc ^= oracle.mul(a_i, b_i)
            scratch.append(acc)
    return fold_chunk(oracle, s_evals, log_domain, log_len, chunk_index, scratch, fold_challenges)


# ---------------------------------------------------------------------------------------------- merkle_tree/scheme.rs:67-168
def fold_digests(oracle, ds):
    ds = list(ds)
    if len(ds) & (len(ds) - 1) or not ds:
        raise FriVerifyError("PowerOfTwoLengthRequired")
    n = len(ds) // 2
    while n:
        for i in range(n):
            ds[i] = oracle.groestl256_compress2(ds[2 * i], ds[2 * i + 1])
        n //= 2
    return ds[0]


def verify_vector(oracle, root, data_units, batch_size):
    if data_units.shape[0] % batch_size:
        raise FriVerifyError("IncorrectBatchSize")
    leaves = [hash_elems(oracle, data_units[i : i + batch_size]) for i in range(0, data_units.shape[0], batch_size)]
    if fold_digests(oracle, leaves) != bytes(root):
        raise FriVerifyError("InvalidProof", "verify_vector")


def verify_layer(oracle, root, layer_depth, layer_digests):
    if 1 << layer_depth != len(layer_digests):
        raise FriVerifyError("IncorrectVectorLength")
    if fold_digests(oracle, layer_digests) != bytes(root):
        raise FriVerifyError("InvalidProof", "verify_layer")


def verify_opening(oracle, index, value_units, layer_depth, tree_depth, layer_digests, branch):
    if 1 << layer_depth != len(layer_digests):
        raise FriVerifyError("IncorrectVectorLength")
    if index >= 1 << tree_depth:
        raise FriVerifyError("IndexOutOfRange")
    assert len(branch) == tree_depth - layer_depth
    d = hash_elems(oracle, value_units)
    for node in branch:
        d = oracle.groestl256_compress2(d, node) if index & 1 == 0 else oracle.groestl256_compress2(node, d)
        index >>= 1
    if d != layer_digests[index]:
        raise FriVerifyError("InvalidProof", "verify_opening")


# ---------------------------------------------------------------------------------------------- fri/verify.rs
class _Reader:
    def __init__(self, advice):
        self.u, self.at = np.ascontiguousarray(advice, dtype=np.uint64).reshape(-1, 2), 0

    def take(self, n):
        if self.at + n > self.u.shape[0]:
            raise FriVerifyError("TranscriptError", "NotEnoughBytes")
        out = self.u[self.at : self.at + n]
        self.at += n
        return out


def verify(oracle, p, codeword_commitment, round_commitments, challenges, indices, advice):
    """FRIVerifier::new + verify (verify.rs:54-147) on the advice block alone; returns the final value.  challenges: the
    n_fold_rounds folding challenges (interleave challenges first); indices: what transcript.sample_bits(index_bits) returned."""
    assert len(round_commitments) == p.n_oracles() and len(challenges) == p.n_fold_rounds() and len(indices) == p.n_test_queries
    log_domain = p.rs_log_len()
    s_evals = oracle.ntt_s_evals(TW_LEVEL, log_domain)
    tensor = tensor_expand(oracle, challenges[: p.log_batch_size])
    fold_challenges = list(challenges[p.log_batch_size :])
    depths = p.optimal_layer_depths()
    rd = _Reader(advice)
    terminate_units = rd.take(p.terminate_len())
    terminate = ints(terminate_units)

    # ---- verify_last_oracle (:152-223)
    n_final = p.n_final_challenges()
    verify_vector(oracle, round_commitments[-1] if round_commitments else codeword_commitment, terminate_units, 1 << n_final)
    if p.n_oracles():
        final_challenges = fold_challenges[len(fold_challenges) - n_final :]
        rep = [fold_chunk(oracle, s_evals, log_domain, n_final + p.log_inv_rate, i, terminate[i << n_final : (i + 1) << n_final], final_challenges)
               for i in range(len(terminate) >> n_final)]
    else:
        fold_arity = p.log_dim + p.log_batch_size
        rep = [fold_interleaved_chunk(oracle, s_evals, log_domain, p.rs_log_len(), p.log_batch_size, i, terminate[i << fold_arity : (i + 1) << fold_arity], tensor,
                                      fold_challenges)
               for i in range(len(terminate) >> fold_arity)]
    final_value = rep[0]
    if any(x != final_value for x in rep[1:]):
        raise FriVerifyError("IncorrectDegree")

    # ---- the layers against the commitments (:117-129)
    layers = [digests(rd.take(2 << d)) for d in depths]
    for commitment, depth, layer in zip([codeword_commitment] + list(round_commitments), depths, layers):
        verify_layer(oracle, commitment, depth, layer)

    # ---- verify_query_internal per index (:254-352)
    for index in indices:
        if not p.fold_arities:
            continue
        arity0 = p.fold_arities[0]
        fold_round, log_n_cosets = 0, p.index_bits()
        log_coset_size = arity0 - p.log_batch_size
        vals = rd.take(1 << arity0)  # verify_coset_opening (:370-394)
        verify_opening(oracle, index, vals, depths[0], log_n_cosets, layers[0], digests(rd.take(2 * (log_n_cosets - depths[0]))))
        next_value = fold_interleaved_chunk(oracle, s_evals, log_domain, p.rs_log_len(), p.log_batch_size, index, ints(vals), tensor,
                                            fold_challenges[fold_round : fold_round + log_coset_size])
        fold_round += log_coset_size
        for i, arity in enumerate(p.fold_arities[1:]):
            coset_index = index >> arity
            log_n_cosets -= arity
            vals = rd.take(1 << arity)
            verify_opening(oracle, coset_index, vals, depths[i + 1], log_n_cosets, layers[i + 1], digests(rd.take(2 * (log_n_cosets - depths[i + 1]))))
            values = ints(vals)
            if next_value != values[index % (1 << arity)]:
                raise FriVerifyError("IncorrectFold", "query_round %d index %d" % (i, index))
            next_value = fold_chunk(oracle, s_evals, log_domain, p.rs_log_len() - fold_round, coset_index, values, fold_challenges[fold_round : fold_round + arity])
            index = coset_index
            fold_round += arity
        if next_value != terminate[index]:
            raise FriVerifyError("IncorrectFold", "query_round %d index %d" % (p.n_oracles() - 1, index))
    assert rd.at == rd.u.shape[0], "the advice is longer than the proof"
    return final_value


# ---------------------------------------------------------------------------------------------- the Python prover
Proof = namedtuple("Proof", "commitments codewords trees advice")  # commitments[0]: the codeword's; trees: (2 n - 1, 32) uint8 node arrays


def commit_and_fold(oracle, p, message, challenges, tamper=None):
    """commit_interleaved + every FRIFolder::execute_fold_round (fri/prove.rs:88-432) from the oracle's NTT, folds and Merkle trees:
    (codewords, trees) of the 1 + n_oracles committed oracles (the last one is the terminate codeword when anything is folded).
    tamper = (k, position): one bit of oracle k is flipped in what is committed and opened, while the folding goes on from the honest
    word -- a prover that commits to a wrong fold (k = n_oracles: to a terminate codeword that is no codeword)."""
    log_domain = p.rs_log_len()
    s_evals = oracle.ntt_s_evals(TW_LEVEL, log_domain)
    code = np.concatenate([np.ascontiguousarray(message, dtype=np.uint64)] * (1 << p.log_inv_rate))
    assert oracle.ntt_forward(code, 5, 5, s_evals, log_domain, p.log_batch_size + 2, p.rs_log_len(), 0, 0, 0, p.log_inv_rate) == 0
    coset_log = [p.fold_arities[k] if k < len(p.fold_arities) else p.n_final_challenges() for k in range(len(p.fold_arities) + 1)]
    if not p.fold_arities:
        coset_log = [p.log_dim + p.log_batch_size]
    codewords, trees = [], []
    cur, cur_log_len, cur_log_batch, pos = code, p.rs_log_len(), p.log_batch_size, 0
    for k in range(len(coset_log)):
        if k:
            arity = p.fold_arities[k - 1]
            chs = list(challenges[pos : pos + arity])
            pos += arity
            new_log_len = cur_log_len - (arity - cur_log_batch)
            nxt = oracle.arr(1 << new_log_len)
            assert oracle.fri_fold(s_evals, 5, log_domain, cur_log_len, cur_log_batch, chs, cur, nxt) == 0
            cur, cur_log_len, cur_log_batch = nxt, new_log_len, 0
        sent = cur
        if tamper and tamper[0] == k:
            sent = cur.copy()
            sent[tamper[1], 0] ^= np.uint64(1)
        rc, nodes = oracle.merkle_build(sent, 1 << coset_log[k])
        assert rc == 0
        codewords.append(sent)
        trees.append(nodes)
    return codewords, trees


def tree_layer(nodes, depth):
    log_len = (nodes.shape[0] + 1).bit_length() - 2
    start = (2 << log_len) - (2 << depth)
    return nodes[start : start + (1 << depth)]


def tree_branch(nodes, index, depth):
    """BinaryMerkleTree::branch (binary_merkle_tree.rs:121-141): leaf sibling first"""
    log_len = (nodes.shape[0] + 1).bit_length() - 2
    return [nodes[(((1 << j) - 1) << (log_len + 1 - j)) | ((index >> j) ^ 1)] for j in range(log_len - depth)]


def advice_block(p, codewords, trees, indices):
    """What FRIFolder::finish_proof writes to the decommitment (fri/prove.rs:483-507): slices of the codewords and of the trees"""
    depths = p.optimal_layer_depths()
    parts = [codewords[-1]]
    parts += [units(tree_layer(trees[i], depths[i])) for i in range(p.n_oracles())]
    for index in indices:
        for i, arity in enumerate(p.fold_arities):
            if i:
                index >>= arity
            parts.append(codewords[i][index << arity : (index + 1) << arity])
            br = tree_branch(trees[i], index, depths[i])
            if br:
                parts.append(units(np.stack(br)))
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.uint64)


def prove(oracle, p, message, challenges, indices, tamper=None):
    codewords, trees = commit_and_fold(oracle, p, message, challenges, tamper)
    return Proof([bytes(t[-1]) for t in trees], codewords, trees, advice_block(p, codewords, trees, indices))


# ---- inputs and proofs: computed once per process, handed out read-only
_cache = {}


def case(oracle, p):
    """(message, challenges, indices, Proof) of a shape, seeded by the shape"""
    if p not in _cache:
        seed = 0xF21 + 97 * [q for q, _ in SHAPES].index(p)
        message = oracle.random_b128(seed, 1 << (p.log_dim + p.log_batch_size))
        challenges = oracle.random_scalars(seed + 1, p.n_fold_rounds())
        idx = query_indices(oracle, p)
        pr = prove(oracle, p, message, challenges, idx)
        for a in [message, pr.advice] + pr.codewords + pr.trees:
            a.setflags(write=False)
        _cache[p] = (message, challenges, idx, pr)
    return _cache[p]
