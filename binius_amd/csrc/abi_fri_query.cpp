// binius_amd/csrc/abi_fri_query.cpp -- bn_fri_query_openings: the decommitment FRIFolder::finish_proof writes (crates/core/src/
// protocols/fri/prove.rs:483-507: terminate codeword, vcs_optimal_layers, prove_query for every index) from codewords and Merkle trees
// resident on the device, and bn_fri_query_proof_elems, its layout.  Argument validation and the plan of the launch; the kernel is in
// kernels_fri_query.hip.
//
// The kernel reads at addresses it computes from the indices, so everything an address depends on is checked here, before anything is
// launched: every index against 2^index_bits, and for every oracle that the shifted index is a coset of it (index_bits - index_shift <=
// log_n_cosets) and that its layer exists (layer_depth <= log_n_cosets).  The offsets inside the output are computed here, never taken
// from the caller.  One launch writes the whole block into the context's pinned, device-mapped staging (the buffer bn_gather_d2h
// grows on demand; the indices travel in its first bytes), one synchronisation, one host copy.
#include "abi_common.hpp"

namespace {

struct fq_layout {
	uint64_t header = 0, record = 0, total = 0;
	uint64_t layer_off[bn::kFriQueryMaxOracles], record_off[bn::kFriQueryMaxOracles];
};

// The sizes alone: BN_OK, or the error of the first descriptor that is out of range.  One call holds at most 2^26 elements (1 GiB of
// pinned staging), as bn_gather_d2h.
int fq_plan(const bn_fri_oracle *o, uint32_t n_oracles, uint64_t terminate_elems, uint64_t n_queries, fq_layout &l)
{
	BN_REQUIRE(n_oracles == 0 || o, "fri query: null argument");
	BN_REQUIRE(n_oracles <= BN_FRI_QUERY_MAX_ORACLES, "fri query: more oracles than one call takes (BN_FRI_QUERY_MAX_ORACLES)");
	constexpr uint64_t kMax = (uint64_t)1 << 26;
	BN_REQUIRE(terminate_elems <= kMax && n_queries <= kMax, "fri query: too many elements for one call");
	l.header = terminate_elems;
	for (uint32_t i = 0; i < n_oracles; i++) {
		BN_REQUIRE(o[i].log_n_cosets < 48 && o[i].log_coset_size < 48 && o[i].log_n_cosets + o[i].log_coset_size < 48, "fri query: codeword size out of range (< 2^48)");
		BN_REQUIRE(o[i].layer_depth <= o[i].log_n_cosets, "IncorrectLayerDepth: layer_depth is larger than log_n_cosets");
		BN_REQUIRE(o[i].layer_depth <= 26 && o[i].log_coset_size <= 26, "fri query: too many elements for one call");
		l.layer_off[i] = l.header;
		l.header += (uint64_t)2 << o[i].layer_depth;
		l.record_off[i] = l.record;
		l.record += ((uint64_t)1 << o[i].log_coset_size) + 2 * (uint64_t)(o[i].log_n_cosets - o[i].layer_depth);
		BN_REQUIRE(l.header <= kMax && l.record <= kMax, "fri query: too many elements for one call");
	}
	l.total = l.header + n_queries * l.record; // (both factors <= 2^26)
	BN_REQUIRE(l.total <= kMax, "fri query: too many elements for one call");
	return BN_OK;
}

} // namespace

extern "C" {

int bn_fri_query_proof_elems(const void *oracles, uint32_t n_oracles, uint64_t terminate_elems, uint64_t n_queries, uint64_t *header_elems_out,
                             uint64_t *record_elems_out, uint64_t *total_elems_out)
{
	BN_REQUIRE(header_elems_out && record_elems_out && total_elems_out, "fri query: null argument");
	fq_layout l;
	if (const int rc = fq_plan((const bn_fri_oracle *)oracles, n_oracles, terminate_elems, n_queries, l)) return rc;
	*header_elems_out = l.header;
	*record_elems_out = l.record;
	*total_elems_out = l.total;
	return BN_OK;
}

int bn_fri_query_openings(bn_ctx *ctx, const void *oracles, uint32_t n_oracles, const void *d_terminate, uint64_t terminate_elems, const uint64_t *indices,
                          uint64_t n_queries, uint32_t index_bits, bn_f128 *h_out, uint64_t out_elems)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	const bn_fri_oracle *o = (const bn_fri_oracle *)oracles;
	fq_layout l;
	if (const int rc = fq_plan(o, n_oracles, terminate_elems, n_queries, l)) return rc;
	BN_REQUIRE(out_elems == l.total, "fri query: out_elems is not what bn_fri_query_proof_elems states for these arguments");
	BN_REQUIRE((terminate_elems == 0 || d_terminate) && (n_queries == 0 || indices) && (l.total == 0 || h_out), "fri query: null argument");
	BN_REQUIRE(aligned16(d_terminate), "fri query: pointers must be 16-byte aligned");
	BN_REQUIRE(index_bits < 48, "fri query: index_bits out of range (< 48)");
	for (uint32_t i = 0; i < n_oracles; i++) {
		BN_REQUIRE(o[i].d_codeword && o[i].d_nodes, "fri query: null codeword or node array");
		BN_REQUIRE(aligned16(o[i].d_codeword, o[i].d_nodes), "fri query: pointers must be 16-byte aligned");
		// indices[q] >> index_shift < 2^(index_bits - index_shift) must be a coset of the oracle
		BN_REQUIRE(o[i].index_shift <= index_bits && index_bits - o[i].index_shift <= o[i].log_n_cosets, "fri query: index_bits - index_shift exceeds the oracle's log_n_cosets");
	}
	for (uint64_t q = 0; q < n_queries; q++)
		BN_REQUIRE(indices[q] >> index_bits == 0, "IndexOutOfRange: a query index is not below 2^index_bits");

	// ---- everything the launch reads is brought up to date (a fold deferred on a codeword, a tree whose leaves are one)
	BN_FLUSH_FOR(ctx, bn_range{d_terminate, terminate_elems});
	for (uint32_t i = 0; i < n_oracles; i++)
		BN_FLUSH_FOR(ctx, bn_range{o[i].d_codeword, (uint64_t)1 << (o[i].log_n_cosets + o[i].log_coset_size)},
		             bn_range{o[i].d_nodes, 2 * (((uint64_t)2 << o[i].log_n_cosets) - 1)});
	if (l.total == 0) {
		ctx->fq_calls++;
		return BN_OK;
	}

	const size_t idx_bytes = ((size_t)n_queries * 8 + 15) & ~(size_t)15;
	const size_t need = idx_bytes + (size_t)l.total * sizeof(f128);
	if (need > ctx->gather_bytes) {
		BN_HIP(hipStreamSynchronize(ctx->stream));
		if (ctx->h_gather) hipHostFree(ctx->h_gather);
		ctx->h_gather = nullptr;
		ctx->gather_bytes = 0;
		size_t cap = 1 << 16;
		while (cap < need) cap <<= 1;
		if (hipHostMalloc(&ctx->h_gather, cap, hipHostMallocMapped) != hipSuccess)
			return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (pinned gather buffer)");
		BN_HIP(hipHostGetDevicePointer(&ctx->d_gather, ctx->h_gather, 0));
		ctx->gather_bytes = cap;
	}
	if (n_queries) std::memcpy(ctx->h_gather, indices, (size_t)n_queries * 8);

	bn::fri_query_args a{};
	for (uint32_t i = 0; i < n_oracles; i++)
		a.o[i] = bn::fri_query_oracle{o[i].d_codeword, o[i].d_nodes, o[i].log_n_cosets, o[i].log_coset_size, o[i].layer_depth, o[i].index_shift,
		                              l.layer_off[i], l.record_off[i]};
	a.terminate = d_terminate;
	a.terminate_elems = terminate_elems;
	a.header_elems = l.header;
	a.record_elems = l.record;
	a.n_oracles = n_oracles;
	a.n_queries = (uint32_t)n_queries;
	a.header_wgs = (uint32_t)((l.header + bn::kFriQueryHeaderChunk - 1) / bn::kFriQueryHeaderChunk);
	BN_HIP(bn::launch_fri_query(ctx->stream, a, (const uint64_t *)ctx->d_gather, (char *)ctx->d_gather + idx_bytes));
	BN_HIP(hipStreamSynchronize(ctx->stream));
	std::memcpy(h_out, (const char *)ctx->h_gather + idx_bytes, (size_t)l.total * sizeof(f128));
	ctx->fq_calls++;
	ctx->fq_launches++;
	ctx->fq_openings += n_queries * n_oracles;
	return BN_OK;
}

int bn_fri_query_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_FQ_CALLS] = ctx->fq_calls;
	counters[BN_FQ_LAUNCHES] = ctx->fq_launches;
	counters[BN_FQ_OPENINGS] = ctx->fq_openings;
	return BN_OK;
}

} // extern "C"
