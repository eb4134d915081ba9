// binius_amd/csrc/abi_prodtree.cpp -- bn_product_tree_layers: every layer of a batch of halves-product trees, the witness of the
// GKR grand-product argument (GrandProductWitness::new, core/src/protocols/gkr_gpa/gkr_gpa.rs:38-90), and bn_pad_with_ones, the
// full-length copies of truncated inputs its prover folds.  Argument validation and the plan of launches; the kernels are in
// kernels_prodtree.hip.
//
// The plan: a tree of n variables goes through stages, each a job of one launch -- while its current layer has more than 2^15
// elements, two layers per job of the bit-sliced form (one when only one is left above 2^15; two wave-batches per step when a launch
// has more batches than wave slots), then six per job of the workgroup form.  Stage i of every tree of the batch shares launch i
// (one launch per form), so a batch costs the launches of its largest tree: 2^24 takes 5 + 3, 2^16 takes 1 + 3, anything up to 2^6 takes one.  All job tables of a call are uploaded in one copy.
#include <algorithm>

#include "abi_common.hpp"

namespace {

struct stage_list {
	std::vector<bn::prodtree_job> big, small;
	uint32_t big_units = 0, small_units = 0;
	uint64_t big_products = 0; // of the jobs' first layers
	bool dual = false;
};

} // namespace

extern "C" {

int bn_product_tree_layers(bn_ctx *ctx, uint32_t n_trees, const uint32_t *n_vars, const void *const *d_inputs, const uint64_t *input_lens,
                           void *const *d_layers, bn_f128 *products_out)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n_trees == 0) return BN_OK;
	BN_REQUIRE(n_vars && d_inputs && input_lens && d_layers && products_out, "null argument");
	BN_REQUIRE(n_trees <= (1u << 20), "too many trees for one call");
	for (uint32_t t = 0; t < n_trees; t++) {
		BN_REQUIRE(n_vars[t] <= BN_PRODUCT_TREE_MAX_VARS, "product tree: n_vars out of range (0 .. 28)");
		const uint64_t full = (uint64_t)1 << n_vars[t];
		BN_REQUIRE(input_lens[t] <= full, "product tree: input_len exceeds 2^n_vars");
		BN_REQUIRE(input_lens[t] == 0 || d_inputs[t], "product tree: null input");
		BN_REQUIRE(aligned16(d_inputs[t], d_layers[t]), "product tree: pointers must be 16-byte aligned");
		if (n_vars[t] == 0) continue; // (an arena of one element, which is not touched)
		BN_REQUIRE(d_layers[t], "product tree: null layer arena");
		BN_REQUIRE(input_lens[t] == 0 || !ranges_overlap(d_inputs[t], input_lens[t], d_layers[t], full), "product tree: the layer arena overlaps its input");
	}

	// ---- the stages of every tree; stage i of all trees shares a launch per form
	std::vector<stage_list> stages;
	std::vector<const f128 *> roots(n_trees);
	for (uint32_t t = 0; t < n_trees; t++) {
		const f128 *in = (const f128 *)d_inputs[t];
		f128 *arena = (f128 *)d_layers[t];
		uint32_t m = n_vars[t];
		roots[t] = m ? arena + 1 : (input_lens[t] ? in : nullptr);
		for (uint32_t st = 0; m > 0; st++) {
			if (stages.size() <= st) stages.emplace_back();
			stage_list &sl = stages[st];
			bn::prodtree_job jb{};
			const bool first = m == n_vars[t];
			jb.src = first ? in : arena + ((uint64_t)1 << m);
			jb.src_len = first ? input_lens[t] : (uint64_t)1 << m;
			jb.arena = arena;
			jb.m = m;
			if (m > bn::kProdtreeSmallMaxLog2) {
				jb.n_levels = std::min(bn::kProdtreeBigLevels, m - bn::kProdtreeSmallMaxLog2);
				sl.big_products += (uint64_t)1 << (m - 1);
				sl.big.push_back(jb); // (its first run: below, once the stage's form is known)
			} else {
				jb.n_levels = std::min(bn::kProdtreeSmallLevels, m);
				const uint64_t wgs = (uint64_t)1 << (m - jb.n_levels);
				BN_REQUIRE((uint64_t)sl.small_units + wgs < (1ull << 31), "product tree: batch too large for one call");
				jb.start = sl.small_units;
				sl.small_units += (uint32_t)wgs;
				sl.small.push_back(jb);
			}
			m -= jb.n_levels;
		}
	}

	// the bit-sliced form of a stage: two wave-batches per step when the launch has more batches than wave slots (as launch_mul9
	// chooses k_mul9_dual), which makes its runs twice as long
	for (stage_list &sl : stages) {
		sl.dual = sl.big_products > (uint64_t)ctx->n_cu * 8 * bn::kProdtreeBatch;
		for (bn::prodtree_job &jb : sl.big) {
			const uint64_t per_run = (uint64_t)(4 * bn::kProdtreeBatch * (sl.dual ? 2 : 1)) >> (jb.n_levels - 1);
			const uint64_t runs = (((uint64_t)1 << (jb.m - jb.n_levels)) + per_run - 1) / per_run;
			BN_REQUIRE((uint64_t)sl.big_units + runs < (1ull << 31), "product tree: batch too large for one call");
			jb.start = sl.big_units;
			sl.big_units += (uint32_t)runs;
		}
	}

	// ---- one upload: [job tables, stage by stage][root pointers]; the roots are gathered behind them
	call_upload up(ctx);
	std::vector<upload_section<bn::prodtree_job>> s_big, s_small;
	for (const stage_list &sl : stages) {
		s_big.push_back(up.reserve<bn::prodtree_job>(sl.big.size()));
		s_small.push_back(up.reserve<bn::prodtree_job>(sl.small.size()));
	}
	const auto s_roots = up.reserve<const f128 *>(n_trees);
	up.device_only();
	const auto s_prod = up.reserve<f128>(n_trees);
	if (const int rc = up.alloc()) return rc;
	for (size_t i = 0; i < stages.size(); i++) {
		std::copy(stages[i].big.begin(), stages[i].big.end(), up.host(s_big[i]));
		std::copy(stages[i].small.begin(), stages[i].small.end(), up.host(s_small[i]));
	}
	std::copy(roots.begin(), roots.end(), up.host(s_roots));
	BN_HIP(up.send());
	for (size_t i = 0; i < stages.size(); i++) {
		const stage_list &sl = stages[i];
		BN_HIP(bn::launch_prodtree_big(ctx->stream, ctx->n_cu, up.dev(s_big[i]), (uint32_t)sl.big.size(), sl.big_units, sl.dual));
		BN_HIP(bn::launch_prodtree_small(ctx->stream, up.dev(s_small[i]), (uint32_t)sl.small.size(), sl.small_units));
	}
	f128 *d_prod = up.dev(s_prod);
	BN_HIP(bn::launch_prodtree_roots(ctx->stream, up.dev(s_roots), n_trees, d_prod));
	// the products through the zero-copy mailbox, 64 at a time (the spin also covers the upload above: its host mirror may go)
	for (uint32_t t0 = 0; t0 < n_trees; t0 += 64) {
		f128 vals[64];
		const uint32_t cnt = std::min<uint32_t>(64, n_trees - t0);
		const int rc = publish_vals(ctx, d_prod + t0, 1, cnt, 0, 1, vals);
		if (rc) return rc;
		for (uint32_t i = 0; i < cnt; i++) products_out[t0 + i] = bn_f128{vals[i].lo, vals[i].hi};
	}
	return BN_OK;
}

int bn_pad_with_ones(bn_ctx *ctx, uint32_t n, const uint32_t *log_lens, const void *const *d_srcs, const uint64_t *src_lens, void *const *d_dsts)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	if (n == 0) return BN_OK;
	BN_REQUIRE(log_lens && d_srcs && src_lens && d_dsts, "null argument");
	BN_REQUIRE(n <= (1u << 20), "too many arrays for one call");
	std::vector<bn::prodtree_job> jobs(n);
	uint64_t blocks = 0;
	for (uint32_t t = 0; t < n; t++) {
		BN_REQUIRE(log_lens[t] <= BN_PRODUCT_TREE_MAX_VARS, "pad: log_len out of range (0 .. 28)");
		const uint64_t full = (uint64_t)1 << log_lens[t];
		BN_REQUIRE(src_lens[t] <= full, "pad: src_len exceeds 2^log_len");
		BN_REQUIRE(d_dsts[t] && (src_lens[t] == 0 || d_srcs[t]), "pad: null pointer");
		BN_REQUIRE(aligned16(d_srcs[t], d_dsts[t]), "pad: pointers must be 16-byte aligned");
		BN_REQUIRE(src_lens[t] == 0 || !ranges_overlap(d_srcs[t], src_lens[t], d_dsts[t], full), "pad: destination overlaps its source");
		jobs[t] = bn::prodtree_job{(const f128 *)d_srcs[t], (f128 *)d_dsts[t], src_lens[t], log_lens[t], 0, (uint32_t)blocks, 0};
		blocks += (full + 255) / 256;
		BN_REQUIRE(blocks < (1ull << 31), "pad: batch too large for one call");
	}
	char *scr = (char *)bn::ctx_scratch(ctx, jobs.size() * sizeof(bn::prodtree_job));
	if (!scr) return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (scratch)");
	BN_HIP(hipMemcpyAsync(scr, jobs.data(), jobs.size() * sizeof(bn::prodtree_job), hipMemcpyHostToDevice, ctx->stream));
	BN_HIP(bn::launch_prodtree_pad(ctx->stream, (const bn::prodtree_job *)scr, n, (uint32_t)blocks));
	BN_HIP(hipStreamSynchronize(ctx->stream)); // (the table is pageable host memory that goes out of scope)
	return BN_OK;
}

} // extern "C"
