// binius_amd/csrc/abi_fold.cpp -- the single-claim deferred fold: the fold entry points (bn_extrapolate_line*), where every deferral
// of this backend begins, and the flush that undoes it (flush_pending / flush_legacy), with the range helpers, the host tail's fold
// and write-back and the predicates both sides share.  The claim groups' side of the same calls is abi_group.cpp.
//
// bn_extrapolate_line_batch_scaled is a validated request (fold_call) and then the route order, decided in ONE place (fold_entry):
// wide batch in pieces | second chained fold | copy absorption | claim groups | host tail | survivors, flush, park.
// flush_legacy is "what dies" (flush_drop_state) and "what runs" (flush_run_folds).
#include <atomic>

#include "abi_common.hpp"
#include "hostmul.hpp"

namespace bnabi {
bool ranges_overlap(const void *p, uint64_t n_p, const void *q, uint64_t n_q)
{
	const char *a = (const char *)p, *b = (const char *)q;
	return n_p && n_q && a < b + n_q * sizeof(f128) && b < a + n_p * sizeof(f128);
}

// [p, p + n) touches none of the arrays the deferred fold reads or writes, nor the weighted shadow
bool independent_of_pending(bn_ctx *ctx, const void *p, uint64_t n)
{
	const bn_ctx::pending_fold &pf = ctx->pend;
	for (uint32_t i = 0; i < pf.count; i++)
		if (ranges_overlap(p, n, pf.x0[i], pf.n) || ranges_overlap(p, n, pf.x1[i], pf.n) || ranges_overlap(p, n, pf.src0[i], pf.n)) return false;
	if (ctx->shadow.valid && ctx->shadow.S && ranges_overlap(p, n, ctx->shadow.S, ctx->shadow.S_cap)) return false;
	return true;
}

// [p, p + n) overlaps an array the MLE-check shadow describes: the halves of the caller's a and b the next evaluation will
// pass, the indicator table (and the noted copy of its lower half, which the caller's next add turns into the table), S
bool shadow_touched_by_write(bn_ctx *ctx, const void *p, uint64_t n)
{
	const bn_ctx::shadow_state &sh = ctx->shadow;
	if (!sh.valid) return false;
	for (const void *q : {sh.a_lo, sh.a_hi, sh.b_lo, sh.b_hi})
		if (q && ranges_overlap(p, n, q, sh.half)) return true;
	if (sh.eq && ranges_overlap(p, n, sh.eq, sh.eq_len)) return true;
	if (sh.eq_copy_dst && ranges_overlap(p, n, sh.eq_copy_dst, sh.eq_len / 2)) return true;
	if (sh.S && ranges_overlap(p, n, sh.S, sh.S_cap)) return true;
	return false;
}

bool pre_matches(const bn_ctx::precomp_state &pre, const bn_ctx::pending_fold &pf)
{
	if (!pre.valid || pre.consumed || pf.count != 2 || pf.scale_mask || 2 * pf.n != pre.m) return false;
	auto is = [&](uint32_t i, int j) { return pf.src0[i] == pre.lo[j] && pf.x1[i] == pre.hi[j]; };
	return (is(0, 0) && is(1, 1)) || (is(0, 1) && is(1, 0));
}

// The host mirror of tiny folded arrays (bn_copy_d2h answers from it): `count` arrays of n elements at ptr[].  host_vals == nullptr:
// a publishing launch puts the values into the mailbox behind sequence number seq; else one value per array, computed on the host.
static void mirror_fill(bn_ctx *ctx, uint32_t count, uint32_t n, const void *const *ptr, uint64_t seq, const f128 *host_vals)
{
	bn_ctx::mirror_state &mr = ctx->mirror;
	mr.valid = true;
	mr.host = host_vals != nullptr;
	mr.seq = seq;
	mr.count = count;
	mr.n = n;
	for (uint32_t i = 0; i < count; i++) {
		mr.ptr[i] = ptr[i];
		if (host_vals) mr.host_vals[i] = host_vals[i];
	}
}

// ---- host tail (abi_kernels.cpp): the device catches up with the folds the host performed on its own copy
// publish: the caller is a host read -- when the arrays are down to one element each, the answer is already here
int host_tail_flush(bn_ctx *ctx, bool publish)
{
	bn_ctx::host_tail_state &ht = ctx->ht;
	if (!ht.active) return BN_OK;
	// (ht.active is cleared only once the write-back is enqueued: if the launch fails the host's folded copy is still the only
	// up-to-date one, and every later call comes back here and reports the error again instead of reading stale arrays)
	if (ht.n_levels) {
		// the host copy's first n0 elements per array ARE the caller's buffers after the folds (the host folds in place exactly as
		// the device would): into the pinned staging, then one launch maps them back to the tower basis and stores them
		uint64_t *stg = (uint64_t *)ctx->h_tail + 2 * (2 * bn::kHtMaxM);
		const uint32_t n0 = ht.chain.n0;
		for (int j = 0; j < 2; j++) std::memcpy(stg + 2 * (size_t)n0 * j, ht.y[j].data(), (size_t)n0 * 16);
		std::atomic_thread_fence(std::memory_order_seq_cst);
		prof_scope ps(ctx, BN_PROF_FOLD);
		BN_HIP(bn::launch_tail_writeback(ctx->stream, ht.chain, (const char *)ctx->d_tail + 2 * bn::kHtMaxM * sizeof(f128), (const char *)ctx->d_phi + 512 * sizeof(f128)));
		ctx->ht_flushed++;
	}
	ht.active = false;
	if (publish && ht.cur_m == 1 && !ht.evaluated && ht.n_levels) {
		f128 vals[2];
		for (int j = 0; j < 2; j++) vals[j] = bn::hostpoly_to_tower(bn::hp128{ht.y[j][0], ht.y[j][1]});
		mirror_fill(ctx, 2, 1, ht.cur_lo, 0, vals);
	}
	ht.n_levels = 0;
	return BN_OK;
}

// The fold batch (src0 | x1 -> x0, n elements each) is the fold of the host tail's current arrays: performed on the host
// copy, recorded for the device (true), or not the expected call (false: the caller flushes).
bool host_tail_fold(bn_ctx *ctx, void *const *x0, const void *const *src0, const void *const *x1, uint32_t count, uint64_t n, uint32_t scale_mask, f128 z)
{
	bn_ctx::host_tail_state &ht = ctx->ht;
	if (!ht.active || !ht.evaluated || ctx->pend.active || count != 2 || scale_mask || 2 * n != ht.cur_m) return false;
	auto is = [&](uint32_t i, int j) { return src0[i] == ht.cur_lo[j] && x1[i] == ht.cur_hi[j]; };
	int perm = -1;
	if (is(0, 0) && is(1, 1)) perm = 0;
	else if (is(0, 1) && is(1, 0)) perm = 1;
	if (perm < 0 || x0[0] == x0[1]) return false;
	// later folds are in place on the first fold's output (what the write-back of the host copy assumes)
	if (ht.n_levels > 0)
		for (uint32_t i = 0; i < 2; i++)
			if (x0[i] != src0[i]) return false;
	for (uint32_t i = 0; i < 2; i++) { // the output must not overlap what the batch reads of the OTHER array, nor x1 of its own
		const uint32_t o = 1 - i;
		if (ranges_overlap(x0[i], n, src0[o], n) || ranges_overlap(x0[i], n, x1[o], n) || ranges_overlap(x0[i], n, x1[i], n)) return false;
		if (x0[i] != src0[i] && ranges_overlap(x0[i], n, src0[i], n)) return false;
	}
	if (ht.n_levels == 0) {
		if (n > bn::kHtMaxM / 2) return false;
		for (uint32_t i = 0; i < 2; i++) ht.chain.out[perm ? 1 - (int)i : (int)i] = x0[i];
		ht.chain.n0 = (uint32_t)n;
	}
	ht.n_levels++;
	const bn::hp128 pz = bn::hostpoly_from_tower(z);
	for (int j = 0; j < 2; j++) bn::hostpoly_fold(reinterpret_cast<bn::hp128 *>(ht.y[j].data()), n, pz);
	for (uint32_t i = 0; i < 2; i++) {
		const int j = perm ? 1 - (int)i : (int)i;
		ht.cur_lo[j] = x0[i];
		ht.cur_hi[j] = (const char *)x0[i] + (n / 2) * sizeof(f128);
	}
	ht.cur_m = n;
	ht.evaluated = false;
	return true;
}

// A deferred fold as the plain launch: evals_0 is read from src0 where a deferred copy fed it (absorbed copy: read there, write
// here), then one scale pass over the upper half of every array the scale mask marks.
static int run_plain_fold(bn_ctx *ctx, const bn_ctx::pending_fold &pf)
{
	bn::fold_batch fb{};
	for (uint32_t i = 0; i < pf.count; i++) {
		fb.x0[i] = pf.x0[i];
		fb.x1[i] = pf.x1[i];
		fb.src0[i] = pf.src0[i] != pf.x0[i] ? pf.src0[i] : nullptr;
	}
	prof_scope ps(ctx, BN_PROF_FOLD);
	BN_HIP(bn::launch_extrapolate_line_batch(ctx->stream, ctx->n_cu, fb, pf.count, pf.n, pf.z));
	for (uint32_t i = 0; i < pf.count; i++)
		if ((pf.scale_mask >> i) & 1) BN_HIP(bn::launch_scale(ctx->stream, ctx->n_cu, (char *)pf.x0[i] + (pf.n / 2) * sizeof(f128), pf.n / 2, pf.hi_scale));
	return BN_OK;
}

int flush_first_fold(bn_ctx *ctx)
{
	if (!ctx->pend.active || !ctx->pend2.active) return BN_OK;
	arm_cancel(ctx); // (a kernel armed for the pair of folds cannot run half of it)
	const int rc = run_plain_fold(ctx, ctx->pend);
	if (rc) return rc;
	ctx->pend = ctx->pend2; // (pend2 keeps its fields: callers may still hold a reference to them)
	ctx->pend2.active = false;
	ctx->pre.valid = false;
	return BN_OK;
}

int flush_copies(bn_ctx *ctx)
{
	for (const auto &c : ctx->pend_copies)
		BN_HIP(hipMemcpyAsync(c.dst, c.src, c.n * sizeof(f128), hipMemcpyDeviceToDevice, ctx->stream));
	ctx->pend_copies.clear();
	return BN_OK;
}

// Every entry point that can observe device memory or the stream calls this first, so the deferral is invisible.
// everything deferred runs: the claim groups' folds (abi_group.cpp), then the single-claim state.  (The two sets of arrays are
// disjoint -- a batch only joins either side while it is independent of everything waiting -- so the order is free.)
int flush_pending(bn_ctx *ctx, bool keep_tail, bool publish_tiny, bool keep_shadow)
{
	{
		// (also with nothing deferred: a hosted prover may be owed its write-back, sums computed ahead die)
		const int rc = group_flush(ctx);
		if (rc) return rc;
	}
	return flush_legacy(ctx, keep_tail, publish_tiny, keep_shadow);
}

// ---- flush_legacy, first half: what dies.  The host tail's write-back, the side stream's lead, the resident and the armed kernel
// (unless keep_tail), the deferred copies (they run), the precomputed sums, the shadow (unless keep_shadow and nothing is deferred).
static int flush_drop_state(bn_ctx *ctx, bool keep_tail, bool publish_tiny, bool keep_shadow)
{
	if (int rc = host_tail_flush(ctx, publish_tiny)) return rc;
	if (!(keep_shadow && !ctx->pend.active)) side_join(ctx); // whatever follows may read what the side stream writes
	if (!keep_tail) {
		if (int rc = tail_cancel(ctx)) return rc;
		arm_cancel(ctx);
	}
	if (int rc = flush_copies(ctx)) return rc;
	ctx->pre.valid = false; // the precomputed next-round sums die with any call that is not the one they were made for
	// (keep_shadow: the end of a round evaluation that the shadow itself answered -- nothing is deferred any more;
	// bn_extrapolate_line_batch restores the shadow when the batch is the fold it expects)
	if (ctx->shadow.valid && !(keep_shadow && !ctx->pend.active)) {
		BN_SHDBG("flush_pending: dropped (fold_pending=%d, pend.active=%d)", (int)ctx->shadow.fold_pending, (int)ctx->pend.active);
		ctx->shadow.valid = false;
		ctx->shadow.fold_pending = false;
		ctx->shadow_dropped++;
	}
	return BN_OK;
}

// The arrays of the two deferred folds are the four elements per array the last two-round launch published (fin_y): the same two
// folds on the host, six products -- the caller's read of the final evaluations does not wait for the kernel.
static bool final_folds_on_host(const bn_ctx::final_y_state &fy, const bn_ctx::pending_fold &p1, const bn_ctx::pending_fold &p2, f128 *vals)
{
	if (!(fy.valid && p1.count == 2 && p1.n == 2 && p2.n == 1)) return false;
	for (uint32_t i = 0; i < 2; i++)
		if (!(p1.x0[i] == fy.lo[i] && p1.src0[i] == fy.lo[i] && (const char *)p1.x1[i] == (const char *)fy.lo[i] + 2 * sizeof(f128) && p2.x0[i] == fy.lo[i] &&
		      (const char *)p2.x1[i] == (const char *)fy.lo[i] + sizeof(f128)))
			return false;
	for (uint32_t i = 0; i < 2; i++) {
		const f128 *y = fy.y[i];
		const f128 u = y[0] ^ bn::mul_host(p1.z, y[0] ^ y[2]), v = y[1] ^ bn::mul_host(p1.z, y[1] ^ y[3]);
		vals[i] = u ^ bn::mul_host(p2.z, u ^ v);
	}
	return true;
}

// ---- flush_legacy, second half: what runs.  The one or two deferred folds as plain launches -- or, when the caller is a host read
// of a handful of elements (publish_tiny), as ONE launch that also mirrors the results into the mailbox.
static int flush_run_folds(bn_ctx *ctx, bool publish_tiny)
{
	if (!ctx->pend.active) return BN_OK;
	ctx->pend.active = false;
	const bn_ctx::pending_fold &p1 = ctx->pend, &p2 = ctx->pend2;
	if (p2.active) {
		// two folds were deferred (a round in between was answered from precomputed sums): in place, one after the other
		ctx->pend2.active = false;
		if (publish_tiny && (uint64_t)p2.count * p2.n <= 64 && !p1.scale_mask && !p2.scale_mask) {
			const uint64_t seq = ++ctx->mail_seq;
			prof_scope ps(ctx, BN_PROF_FOLD);
			BN_HIP(bn::launch_fold2_publish(ctx->stream, p1.x0, p1.src0, p1.x1, p1.count, (uint32_t)p2.n, p1.z, p2.z, ctx->d_mail, seq));
			// (with the host's values the kernel above still runs -- the caller's memory ends up as always --, nobody waits for it)
			f128 vals[2];
			const bool on_host = final_folds_on_host(ctx->fin_y, p1, p2, vals);
			mirror_fill(ctx, p2.count, (uint32_t)p2.n, p2.x0, seq, on_host ? vals : nullptr);
			ctx->fin_y.valid = false;
			return BN_OK;
		}
		const int rc = run_plain_fold(ctx, p1);
		return rc ? rc : run_plain_fold(ctx, p2);
	}
	if (publish_tiny && (uint64_t)p1.count * p1.n <= 64) {
		// the caller is a host read: fold and mirror the (few) results into the mailbox in one launch
		const uint64_t seq = ++ctx->mail_seq;
		prof_scope ps(ctx, BN_PROF_FOLD);
		BN_HIP(bn::launch_fold_publish(ctx->stream, p1.x0, p1.src0, p1.x1, p1.count, (uint32_t)p1.n, p1.z, ctx->d_mail, seq, p1.scale_mask, p1.hi_scale));
		mirror_fill(ctx, p1.count, (uint32_t)p1.n, p1.x0, seq, nullptr);
		return BN_OK;
	}
	return run_plain_fold(ctx, p1);
}

int flush_legacy(bn_ctx *ctx, bool keep_tail, bool publish_tiny, bool keep_shadow)
{
	const int rc = flush_drop_state(ctx, keep_tail, publish_tiny, keep_shadow);
	return rc ? rc : flush_run_folds(ctx, publish_tiny);
}

// ---- the fold entry: a validated request ...
struct fold_call {
	void *const *x0; // evals_0: written ...
	const void *const *x1;
	uint32_t count;
	uint64_t n;
	f128 z;
	uint32_t scale_mask;
	f128 hi_scale;
	bool group_applies;                 // group_fold_applies(), asked ONCE: the wide split and the group route rest on the same answer
	const void *src0[bn::kFoldCallMax]; // ... and read from here: x0 unless absorb_copies() found the deferred copy that feeds it
	fold_call(const bn_ctx *ctx, void *const *x0_, const void *const *x1_, uint32_t count_, uint64_t n_, f128 z_, uint32_t mask, f128 hi_scale_)
	    : x0(x0_), x1(x1_), count(count_), n(n_), z(z_), scale_mask(mask), hi_scale(hi_scale_), group_applies(group_fold_applies(ctx, count_, mask))
	{
		for (uint32_t i = 0; i < count; i++) src0[i] = x0[i];
	}
};

// the request becomes the deferred fold in slot pf (ctx->pend, or ctx->pend2 for the second chained fold)
static void park(bn_ctx::pending_fold &pf, const fold_call &fc)
{
	pf.active = true;
	pf.count = fc.count;
	pf.n = fc.n;
	pf.z = fc.z;
	pf.scale_mask = fc.scale_mask;
	pf.hi_scale = fc.hi_scale;
	for (uint32_t i = 0; i < fc.count; i++) {
		pf.x0[i] = fc.x0[i];
		pf.x1[i] = fc.x1[i];
		pf.src0[i] = fc.src0[i];
	}
}

// ... and its routes, in the order fold_entry tries them
static int fold_entry(bn_ctx *ctx, fold_call &fc);

// A batch wider than one launch's (a prover with more than kFoldBatchMax multilinears, piop/prove.rs:262-287) is the claim
// groups' (abi_group.cpp: deferred whole, folded by the jobs of the next evaluation's launch); where they do not apply it is
// the same folds in pieces of kFoldBatchMax, each through the routes again.  (A wide batch is never scaled: the validation.)
static routed route_wide(bn_ctx *ctx, const fold_call &fc)
{
	if (fc.count <= (uint32_t)bn::kFoldBatchMax || fc.group_applies) return routed::decline();
	for (uint32_t at = 0; at < fc.count; at += (uint32_t)bn::kFoldBatchMax) {
		const uint32_t c = fc.count - at < (uint32_t)bn::kFoldBatchMax ? fc.count - at : (uint32_t)bn::kFoldBatchMax;
		fold_call piece(ctx, fc.x0 + at, fc.x1 + at, c, fc.n, fc.z, 0, f128{0, 0});
		const int rc_p = fold_entry(ctx, piece);
		if (rc_p) return rc_p;
	}
	return routed::answer(BN_OK);
}

// A fold is already deferred, the round evaluation of its output has just been answered from the precomputed sums of
// a two-round launch (abi_kernels.cpp), and this batch folds that output in place: keep BOTH -- the next round
// evaluation folds twice in one pass (kernels_foldeval8.hip).
static routed route_second_fold(bn_ctx *ctx, const fold_call &fc)
{
	const bn_ctx::pending_fold &p1 = ctx->pend;
	if (!(p1.active && !ctx->pend2.active && ctx->pre.valid && ctx->pre.consumed && ctx->lazy_fold && fc.count == 2 && p1.count == 2 && fc.scale_mask == 0 &&
	      p1.scale_mask == 0 && 2 * fc.n == p1.n && ctx->pend_copies.empty()))
		return routed::decline();
	for (uint32_t i = 0; i < 2; i++)
		if (!(fc.x0[i] == p1.x0[i] && (const char *)fc.x1[i] == (const char *)p1.x0[i] + fc.n * sizeof(f128))) return routed::decline();
	park(ctx->pend2, fc); // (unscaled, in place: nothing has been absorbed while a fold is deferred)
	return routed::answer(BN_OK); // (an armed two-round kernel keeps waiting: it is armed for exactly this pair of folds)
}

// Deferred copies whose destination is one of the evals_0 are absorbed: the batch reads there and writes here.  All or none -- if
// one of them is not the batch's, or an absorbed source overlaps an array the batch writes, they all run later, in issue order.
static void absorb_copies(bn_ctx *ctx, fold_call &fc)
{
	if (ctx->pend_copies.empty() || ctx->pend.active) return;
	size_t absorbed = 0;
	for (const auto &c : ctx->pend_copies)
		for (uint32_t i = 0; i < fc.count; i++)
			if (c.dst == fc.x0[i] && c.n == fc.n && fc.src0[i] == fc.x0[i]) {
				fc.src0[i] = c.src;
				absorbed++;
				break;
			}
	// an absorbed copy is read while the fold writes: its source must not overlap any array the
	// batch writes (e.g. a copy chain s -> d1 -> d2 followed by a fold of both)
	bool clash = false;
	for (uint32_t i = 0; i < fc.count && !clash; i++)
		if (fc.src0[i] != fc.x0[i])
			for (uint32_t j = 0; j < fc.count; j++)
				if (ranges_overlap(fc.src0[i], fc.n, fc.x0[j], fc.n)) clash = true;
	if (absorbed == ctx->pend_copies.size() && !clash) {
		ctx->pend_copies.clear();
	} else {
		for (uint32_t i = 0; i < fc.count; i++) fc.src0[i] = fc.x0[i];
	}
}

// Claim groups (abi_group.cpp): a batch that is not the lone two-array shape of the single-claim machinery -- more than
// two arrays, other batches already waiting, or a second prover's batch arriving while the first one's is deferred -- waits
// beside the others; the next evaluations pick their folds up in one launch.
static routed route_groups(bn_ctx *ctx, const fold_call &fc)
{
	bool to_group = fc.group_applies;
	if (!to_group && ctx->grp.enabled && ctx->lazy_fold && !ctx->peer.active && !fc.scale_mask && !ctx->tail_max_n_in && plain_fold_deferred(ctx) && !ctx->shadow.valid) {
		// an independent second prover: nothing of its batch touches what the deferred fold reads or writes
		to_group = true;
		for (uint32_t i = 0; i < fc.count && to_group; i++)
			to_group = independent_of_pending(ctx, fc.x0[i], fc.n) && independent_of_pending(ctx, fc.x1[i], fc.n) && independent_of_pending(ctx, fc.src0[i], fc.n);
	}
	if (!to_group) return routed::decline();
	if (int rc_c = flush_copies(ctx)) return rc_c; // (copies the batch did not absorb: issued before it, they run before it)
	return group_defer_fold(ctx, fc.x0, fc.src0, fc.x1, fc.count, fc.n, fc.z);
}

// The fold of the host tail's current arrays is performed on the host's copy; the device catches up in one launch (host_tail_flush).
static routed route_host_tail(bn_ctx *ctx, const fold_call &fc)
{
	if (!ctx->ht.active) return routed::decline();
	// (deferred copies the batch did not absorb -- possible only while the device is still in step with the host copy --
	// were issued BEFORE this fold and may read what its write-back will overwrite: they run now, in issue order)
	if (int rc_c = flush_copies(ctx)) return rc_c;
	if (host_tail_fold(ctx, fc.x0, fc.src0, fc.x1, fc.count, fc.n, fc.scale_mask, fc.z)) return routed::answer(BN_OK);
	return routed::decline();
}

// ---- what of the earlier state survives a batch that is going to park: one predicate each
// a resident tail kernel survives only if the batch is the fold it is parked for
static bool tail_continues(const bn_ctx *ctx, const fold_call &fc)
{
	if (!(ctx->tail.active && fc.count == 2 && 2 * fc.n == ctx->tail.n_in_next)) return false;
	auto continues = [&](uint32_t i, uint32_t j) {
		return fc.x0[i] == ctx->tail.out[j] && fc.src0[i] == fc.x0[i] && (const char *)fc.x1[i] == (const char *)fc.x0[i] + fc.n * sizeof(f128);
	};
	return (continues(0, 0) && continues(1, 1)) || (continues(0, 1) && continues(1, 0));
}

// ... and so does an armed round: same order of the two arrays, same scale mask; z and the scale are its input
// (a two-fold kernel is armed for the pair pend + pend2: this batch would be its FIRST fold)
static bool arm_continues(const bn_ctx *ctx, const fold_call &fc)
{
	const bn_ctx::arm_state &am = ctx->arm;
	if (!(fc.count == 2 && 2 * fc.n == am.n_in && fc.scale_mask == am.scale_mask && !ctx->pend.active)) return false;
	for (uint32_t j = 0; j < 2; j++)
		if (!(fc.x0[j] == am.out[j] && fc.src0[j] == am.x0[j] && fc.x1[j] == am.x1[j])) return false;
	return true;
}

// the next-round sums of a two-round launch survive exactly one call: the fold of the arrays they describe
// (deferred copies that were not absorbed run inside flush_pending and may write the very arrays the sums describe)
static bool pre_survives(const bn_ctx *ctx, const fold_call &fc)
{
	if (ctx->pend.active || !ctx->lazy_fold || !ctx->pend_copies.empty()) return false;
	bn_ctx::pending_fold probe;
	probe.count = fc.count;
	probe.n = fc.n;
	probe.scale_mask = fc.scale_mask;
	for (uint32_t i = 0; i < fc.count; i++) {
		probe.src0[i] = fc.src0[i];
		probe.x1[i] = fc.x1[i];
	}
	return pre_matches(ctx->pre, probe);
}

// The weighted shadow of an MLE-check (abi_kernels.cpp) survives the fold of exactly its two arrays: *ia = which array of the
// batch is a (-1: the shadow ends with the flush).  The first time, the table is checked for the tensor structure the later
// rounds rely on; a table without it blocks the shadow for the smaller rounds of the instance (blocked_below).
static int shadow_survives(bn_ctx *ctx, const fold_call &fc, int *ia)
{
	bn_ctx::shadow_state &sh = ctx->shadow;
	int sh_ia = -1;
	if (sh.valid && !sh.fold_pending && !ctx->pend.active && ctx->lazy_fold && fc.count == 2 && fc.scale_mask == 0 && fc.n == sh.half) {
		auto is = [&](uint32_t i, const void *lo, const void *hi) { return fc.src0[i] == lo && fc.x1[i] == hi; };
		if (is(0, sh.a_lo, sh.a_hi) && is(1, sh.b_lo, sh.b_hi)) sh_ia = 0;
		else if (is(1, sh.a_lo, sh.a_hi) && is(0, sh.b_lo, sh.b_hi)) sh_ia = 1;
	}
	// (deferred copies that the batch did not absorb run inside flush_pending, on the main stream and in issue order: they
	// may write what the shadow describes or race the side stream's fold of b -- the shadow does not survive them)
	if (sh_ia >= 0 && !ctx->pend_copies.empty()) sh_ia = -1;
	if (sh_ia >= 0 && !sh.checked && fc.n >= 2) {
		// the caller goes on with this instance: is its table a tensor expansion (what the later rounds rely on)?
		bool ok = false;
		int rc_c = shadow_check_table(ctx, &ok);
		if (rc_c) return rc_c;
		if (!ok) {
			sh_ia = -1; // (no: the shadow ends with the flush and the literal kernels answer from here on)
			sh.blocked_below = sh.half;
		}
	}
	if (sh.valid)
		BN_SHDBG("fold batch: count=%u n=%llu half=%llu pend=%d fp=%d match=%d (src0 %p %p x1 %p %p | a %p %p b %p %p)", fc.count, (unsigned long long)fc.n,
		         (unsigned long long)sh.half, (int)ctx->pend.active, (int)sh.fold_pending, sh_ia, fc.src0[0], fc.count > 1 ? fc.src0[1] : nullptr, fc.x1[0],
		         fc.count > 1 ? fc.x1[1] : nullptr, sh.a_lo, sh.a_hi, sh.b_lo, sh.b_hi);
	*ia = sh_ia;
	return BN_OK;
}

// the shadow moves on to the folded arrays (batch array ia is a): they split next round by the variable of bit log2(n) - 1 of the
// table's index.  The fold to one element: nothing is evaluated after it, the shadow has done its work.
static void shadow_advance(bn_ctx *ctx, const fold_call &fc, int ia)
{
	bn_ctx::shadow_state &sh = ctx->shadow;
	const uint64_t n = fc.n;
	if (n < 2) {
		sh.valid = false;
		side_join(ctx);
		return;
	}
	const uint32_t kvar = ilog2(n) - 1;
	sh.valid = true;
	sh.fold_pending = true;
	sh.z = fc.z;
	sh.ia = (uint32_t)ia;
	sh.ib = 1 - sh.ia;
	sh.hi_scale = sh.rho_inv[kvar];
	sh.lambda_next = bn::mul_host(sh.lambda, sh.one_minus_zeta[kvar]);
	sh.a_lo = fc.x0[sh.ia];
	sh.a_hi = (const char *)fc.x0[sh.ia] + (n / 2) * sizeof(f128);
	sh.b_lo = fc.x0[sh.ib];
	sh.b_hi = (const char *)fc.x0[sh.ib] + (n / 2) * sizeof(f128);
	sh.half = n / 2;
}

// The batch parks in ctx->pend: everything else that is deferred runs (flush_pending), except the survivors.  The next API call
// launches the fold -- or, if that call is the round evaluation of exactly these arrays, both run as one kernel
// (kernels_foldeval9.hip).  Eager mode (BN_NO_LAZY_FOLD) flushes at once.
static int park_fold(bn_ctx *ctx, const fold_call &fc)
{
	bool keep_tail = tail_continues(ctx, fc);
	if (ctx->arm.active) {
		if (arm_continues(ctx, fc))
			keep_tail = true;
		else
			arm_cancel(ctx);
	}
	const bool keep_pre = pre_survives(ctx, fc);
	if (!keep_pre) ctx->fin_y.valid = false; // (Y's four elements describe the arrays the sums describe)
	int sh_ia = -1;
	int rc_ = shadow_survives(ctx, fc, &sh_ia);
	if (rc_) return rc_;
	// (the shadow's own fold: nothing is deferred, the shadow stays and the side stream is not joined -- its work, the folds
	// of b and of the table, depends on nothing the main stream does in between)
	rc_ = flush_pending(ctx, keep_tail, false, /*keep_shadow=*/sh_ia >= 0);
	if (rc_) return rc_;
	ctx->pre.valid = keep_pre;
	if (sh_ia >= 0) shadow_advance(ctx, fc, sh_ia);
	park(ctx->pend, fc);
	if (!ctx->lazy_fold) BN_FLUSH(ctx);
	return BN_OK;
}

// the route order
static int fold_entry(bn_ctx *ctx, fold_call &fc)
{
	ctx->mirror.valid = false;
	routed r = route_wide(ctx, fc);
	if (r.kind == routed::declined) r = route_second_fold(ctx, fc);
	if (r.kind == routed::declined) {
		absorb_copies(ctx, fc);
		r = route_groups(ctx, fc);
	}
	if (r.kind == routed::declined) {
		// (what ctx->pend, the mirror and the probe of pre_survives() are sized for: a wider batch was split or is the groups')
		BN_REQUIRE(fc.count <= (uint32_t)bn::kFoldBatchMax, "extrapolate_line batch: more slices than one launch takes reached the single-claim slot");
		r = route_host_tail(ctx, fc);
	}
	return r.kind == routed::declined ? park_fold(ctx, fc) : r.rc;
}
} // namespace bnabi

extern "C" {

// ---------------------------------------------------------------------------------- executor ops
int bn_extrapolate_line(bn_ctx *ctx, void *d_evals_0, uint64_t n0, const void *d_evals_1, uint64_t n1, const bn_f128 *z)
{
	BN_REQUIRE(ctx && z, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(n0 == n1, "evals_0 and evals_1 must be the same length");
	prof_scope ps(ctx, BN_PROF_FOLD);
	BN_HIP(bn::launch_extrapolate_line(ctx->stream, ctx->n_cu, d_evals_0, d_evals_1, n0, to_f(z)));
	return BN_OK;
}

int bn_extrapolate_line_batch(bn_ctx *ctx, void *const *d_evals_0, const void *const *d_evals_1, uint32_t count, uint64_t n,
                              const bn_f128 *z)
{
	return bn_extrapolate_line_batch_scaled(ctx, d_evals_0, d_evals_1, count, n, z, 0, nullptr);
}

int bn_extrapolate_line_batch_scaled(bn_ctx *ctx, void *const *d_evals_0, const void *const *d_evals_1, uint32_t count, uint64_t n,
                                     const bn_f128 *z, uint32_t scale_mask, const bn_f128 *hi_scale)
{
	BN_REQUIRE(ctx && z && d_evals_0 && d_evals_1, "null argument");
	BN_ENTER(ctx);
	BN_REQUIRE(count <= (uint32_t)bn::kFoldCallMax, "too many slices in one extrapolate_line batch");
	BN_REQUIRE(scale_mask == 0 || (hi_scale && (n & 1) == 0 && count <= 32 && (count >= 32 || (scale_mask >> count) == 0)),
	           "scaled fold: needs a scale, an even length and a mask within the batch (at most 32 slices)");
	if (count == 0) return BN_OK;
	fold_call fc(ctx, d_evals_0, d_evals_1, count, n, to_f(z), scale_mask, scale_mask ? to_f(hi_scale) : f128{0, 0});
	return fold_entry(ctx, fc);
}

} // extern "C"
