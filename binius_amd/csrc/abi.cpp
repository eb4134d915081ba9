// binius_amd/csrc/abi.cpp -- the extern "C" boundary declared in include/binius_amd.h:
// argument validation with the reference's error behaviour, context / stream / scratch
// management, the recorded-kernel dispatcher behind accumulate_kernels / map_kernels, and the
// host-only helpers (log_chunks_range, twiddle basis generation).
//
// No arithmetic fallback lives here: every op is a HIP kernel launch.  Host-side field arithmetic
// is used only for O(log n) metadata (twiddle basis = OnTheFlyTwiddleAccess::generate).
#include <atomic>

#include "abi_common.hpp"
#include "hostmul.hpp"

// ---------------------------------------------------------------------------------- errors
namespace {
thread_local std::string g_last_error;
}

namespace bn {
void set_error(const std::string &msg) { g_last_error = msg; }
int fail(int code, const std::string &msg)
{
	g_last_error = msg;
	return code;
}
int hip_fail(hipError_t e, const char *what)
{
	std::ostringstream os;
	os << "device error: " << hipGetErrorString(e) << " (" << what << ")";
	g_last_error = os.str();
	return BN_ERR_DEVICE;
}
void *ctx_scratch(bn_ctx *ctx, size_t bytes)
{
	if (bytes <= ctx->scratch_bytes)
		return ctx->scratch;
	// the previous buffer may still be in use by enqueued work
	hipStreamSynchronize(ctx->stream);
	if (ctx->scratch)
		hipFree(ctx->scratch);
	ctx->scratch = nullptr;
	ctx->scratch_bytes = 0;
	size_t want = bytes + (bytes >> 2);
	if (hipMalloc(&ctx->scratch, want) != hipSuccess) {
		if (hipMalloc(&ctx->scratch, bytes) != hipSuccess)
			return nullptr;
		want = bytes;
	}
	ctx->scratch_bytes = want;
	return ctx->scratch;
}
} // namespace bn

namespace bnabi {
// ---- resident tail kernel: host side of the protocol (device side: kernels_foldeval9.hip)
// command block in the pinned mailbox page: h_mail[80].lo = command word, h_mail[81] = z,
// h_mail[82].lo = status (the id of the last tail kernel that exited)

// Stop the resident kernel (if any) and wait until it has left the device.
int tail_cancel(bn_ctx *ctx)
{
	if (!ctx->tail.active) return BN_OK;
	ctx->tail.active = false;
	__atomic_store_n(tail_cmd(ctx), (ctx->tail.id << 20) | 0xFFFFFull, __ATOMIC_RELEASE);
	BN_HIP(hipStreamSynchronize(ctx->stream));
	return BN_OK;
}

// An armed kernel that will not be used: tell it to leave.  Nothing to wait for -- it exits without having touched
// anything, and whatever the caller enqueues next is ordered behind it by the stream.
void arm_cancel(bn_ctx *ctx)
{
	if (!ctx->arm.active) return;
	ctx->arm.active = false;
	ctx->arm_cancels++;
	__atomic_store_n(arm_cmd(ctx), (ctx->arm.id << 2) | 2ull, __ATOMIC_RELEASE);
}

// Pinned staging of the shadow's table check (the context's gather buffer, 64 KiB): offsets of eq[0], eq[2^k] | the gathered
// entries | at +16384 the ratios and the workgroup layout of the check kernel.
static int shadow_staging(bn_ctx *ctx)
{
	if (ctx->gather_bytes >= (1 << 16)) return BN_OK;
	BN_HIP(hipStreamSynchronize(ctx->stream));
	if (ctx->h_gather) hipHostFree(ctx->h_gather);
	ctx->h_gather = nullptr;
	ctx->gather_bytes = 0;
	if (hipHostMalloc(&ctx->h_gather, 1 << 16, hipHostMallocMapped) != hipSuccess) {
		(void)hipGetLastError();
		return BN_ERR_ALLOC;
	}
	BN_HIP(hipHostGetDevicePointer(&ctx->d_gather, ctx->h_gather, 0));
	ctx->gather_bytes = 1 << 16;
	return BN_OK;
}

// The shadow's table, looked at when the caller's first fold arrives (a lone evaluation never pays for it): the entries
// eq[0], eq[2^k] come to the host (one gather, one synchronisation), the ratios rho_k = eq[2^k] / eq[0] = zeta_k / (1 - zeta_k)
// are formed, and ONE pass checks eq[i] == eq[i - 2^k] * rho_k for every entry.  On the main stream, in line.  Measured and not
// kept: the check started beside ROUND 0 on the side stream (hides the synchronisations, slows that round's VALU-bound kernels
// and every lone evaluation by what it costs: 0.55 -> 0.76 ms at 2^24); the check beside ROUND 1 with the verdict collected
// when that round's result is in and the round answered again on a "no" (-25 us of 1.85 ms at n = 24, and a mid-size armed
// kernel -- two full-register workgroups on every CU -- starves the check until its 6 ms timeout unless arming is held back).
int shadow_check_table(bn_ctx *ctx, bool *ok)
{
	bn_ctx::shadow_state &sh = ctx->shadow;
	*ok = false;
	const uint64_t half = sh.eq_len;
	const uint32_t K = ilog2(half);
	const uint64_t n_items = K + 1;
	const size_t off_bytes = ((size_t)n_items * 8 + 15) & ~(size_t)15;
	if (shadow_staging(ctx) != BN_OK) return BN_OK;
	uint64_t *offs = (uint64_t *)ctx->h_gather;
	offs[0] = 0;
	for (uint32_t k = 0; k < K; k++) offs[k + 1] = (uint64_t)1 << k;
	BN_HIP(bn::launch_gather(ctx->stream, sh.eq, (const uint64_t *)ctx->d_gather, n_items, 1, (char *)ctx->d_gather + off_bytes));
	BN_HIP(hipStreamSynchronize(ctx->stream));
	// ---- what the rounds need are 1 / rho_k = eq[0] / eq[2^k] and 1 - zeta_k = 1 / (1 + rho_k) = eq[0] / (eq[0] + eq[2^k]), what
	// the check needs is rho_k = eq[2^k] / eq[0]: 2 K + 1 inverses, taken with ONE inversion (Montgomery's trick)
	const f128 *got = (const f128 *)((const char *)ctx->h_gather + off_bytes);
	const f128 e0 = got[0];
	if (e0 == f128{0, 0}) return BN_OK;
	const uint32_t N = 2 * K + 1;
	std::vector<f128> v(N), pre(N + 1), vinv(N);
	pre[0] = f128{1, 0};
	for (uint32_t k = 0; k < K; k++) {
		v[2 * k] = got[k + 1];
		v[2 * k + 1] = got[k + 1] ^ e0;
		if (v[2 * k] == f128{0, 0} || v[2 * k + 1] == f128{0, 0}) return BN_OK; // a coordinate 0 or 1: no weighting possible
	}
	v[2 * K] = e0;
	for (uint32_t j = 0; j < N; j++) pre[j + 1] = bn::mul_host(pre[j], v[j]);
	f128 inv = bn::invert_tower(pre[N]);
	for (uint32_t j = N; j-- > 0;) {
		vinv[j] = bn::mul_host(inv, pre[j]);
		inv = bn::mul_host(inv, v[j]);
	}
	sh.rho_inv.assign(K, f128{0, 0});
	sh.one_minus_zeta.assign(K, f128{0, 0});
	f128 *h_rho = (f128 *)((char *)ctx->h_gather + 16384);
	for (uint32_t k = 0; k < K; k++) {
		sh.rho_inv[k] = bn::mul_host(e0, vinv[2 * k]);
		sh.one_minus_zeta[k] = bn::mul_host(e0, vinv[2 * k + 1]);
		h_rho[k] = bn::mul_host(got[k + 1], vinv[2 * K]);
	}
	// ---- the whole table has the structure the ratios describe (*d_flag is zero between checks: only a failing check writes
	// it, and is followed by the reset below; ratios and workgroup layout travel through the pinned staging)
	uint32_t *h_fw = (uint32_t *)((char *)ctx->h_gather + 16384 + 40 * sizeof(f128));
	const uint32_t n_wg = bn::check_tensor_layout(K, h_fw);
	BN_HIP(bn::launch_check_tensor(ctx->stream, sh.eq, half, (const f128 *)((char *)ctx->d_gather + 16384),
	                               (const uint32_t *)((char *)ctx->d_gather + 16384 + 40 * sizeof(f128)), n_wg, K, ctx->d_flag));
	unsigned flag = 1;
	BN_HIP(hipMemcpyAsync(&flag, ctx->d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
	BN_HIP(hipStreamSynchronize(ctx->stream));
	if (flag) BN_HIP(hipMemsetAsync(ctx->d_flag, 0, sizeof(unsigned), ctx->stream));
	*ok = flag == 0;
	sh.checked = *ok;
	return BN_OK;
}

hipStream_t side_stream(bn_ctx *ctx)
{
	if (!ctx->side) {
		hipStream_t st = nullptr;
		hipEvent_t e_side = nullptr, e_main = nullptr;
		if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e_side, hipEventDisableTiming) != hipSuccess ||
		    hipEventCreateWithFlags(&e_main, hipEventDisableTiming) != hipSuccess) {
			// all or nothing: a stream without its two events would run unordered against the main stream
			(void)hipGetLastError();
			if (e_main) (void)hipEventDestroy(e_main);
			if (e_side) (void)hipEventDestroy(e_side);
			if (st) (void)hipStreamDestroy(st);
			return ctx->stream; // (no side stream: the work simply stays in line)
		}
		ctx->side = st;
		ctx->side_ev = e_side;
		ctx->main_ev = e_main;
	}
	if (!ctx->side_busy) {
		(void)hipEventRecord(ctx->main_ev, ctx->stream);
		(void)hipStreamWaitEvent(ctx->side, ctx->main_ev, 0);
		ctx->side_busy = true;
	}
	return ctx->side;
}

int side_run_queue(bn_ctx *ctx)
{
	if (ctx->side_queue.empty()) return BN_OK;
	hipStream_t st = side_stream(ctx);
	std::vector<bn_ctx::side_op> q;
	q.swap(ctx->side_queue);
	for (const auto &op : q) {
		switch (op.kind) {
		case bn_ctx::side_op::COPY: BN_HIP(hipMemcpyAsync(op.dst, op.src, op.n * sizeof(f128), hipMemcpyDeviceToDevice, st)); break;
		case bn_ctx::side_op::ADD_ASSIGN: BN_HIP(bn::launch_add_assign(st, op.dst, op.src, op.n)); break;
		case bn_ctx::side_op::ADD: BN_HIP(bn::launch_add(st, op.dst, op.src, op.src2, op.n)); break;
		case bn_ctx::side_op::FOLD: {
			bn::fold_batch fb{};
			fb.x0[0] = op.dst;
			fb.x1[0] = op.src;
			fb.src0[0] = op.src2;
			BN_HIP(bn::launch_extrapolate_line_batch(st, ctx->n_cu, fb, 1, op.n, op.z));
			break;
		}
		}
	}
	return BN_OK;
}

void side_join(bn_ctx *ctx)
{
	(void)side_run_queue(ctx);
	if (!ctx->side_busy) return;
	(void)hipEventRecord(ctx->side_ev, ctx->side);
	(void)hipStreamWaitEvent(ctx->stream, ctx->side_ev, 0);
	ctx->side_busy = false;
}

std::vector<unsigned char> recipe_bytes(const bn::fin_args &a)
{
	bn::fin_args r;
	std::memset(&r, 0, sizeof(r));
	r.n_terms = a.n_terms;
	r.n_values = a.n_values;
	r.n_ret = a.n_ret;
	r.n_slots = a.n_slots;
	for (uint32_t t = 0; t < a.n_terms; t++) {
		r.terms[t].value = a.terms[t].value;
		r.terms[t].slot = a.terms[t].slot;
		r.terms[t].coeff = a.terms[t].coeff;
	}
	for (uint32_t v = 0; v < a.n_values; v++) r.init[v] = a.init[v];
	for (uint32_t i = 0; i < a.n_ret; i++) r.ret_ids[i] = a.ret_ids[i];
	const unsigned char *p = reinterpret_cast<const unsigned char *>(&r);
	return std::vector<unsigned char>(p, p + sizeof(r));
}

// Waits for the sequence word the publishing kernel writes after its values (fine-grained host memory): a bounded spin, then a
// stream synchronisation so that device errors surface instead of hanging.  cancel_armed: an armed kernel queued behind the
// launch would sit out its whole timeout inside that synchronisation -- it is told to leave first.
int mail_wait(bn_ctx *ctx, uint64_t seq, bool cancel_armed)
{
	volatile uint64_t *seqw = &ctx->h_mail[64].lo;
	uint64_t spins = 0;
	while (__atomic_load_n(seqw, __ATOMIC_ACQUIRE) != seq) {
		if (++spins > (1ull << 22)) {
			if (cancel_armed) arm_cancel(ctx);
			BN_HIP(hipStreamSynchronize(ctx->stream));
			if (__atomic_load_n(seqw, __ATOMIC_ACQUIRE) != seq) return bn::fail(BN_ERR_DEVICE, "device error: result mailbox was not published");
			break;
		}
	}
	return BN_OK;
}

// one call at a time per context (the trait allows the host to call from several threads: rayon join/map)
// XOR of n_groups partial results in d_result[0 .. n_groups) -> host, through the zero-copy mailbox
// (one tiny kernel instead of a device-to-host copy plus a stream synchronisation)
int publish_result(bn_ctx *ctx, uint32_t n_groups, bn_f128 *h_out)
{
	const uint64_t seq = ++ctx->mail_seq;
	BN_HIP(bn::launch_xor_publish(ctx->stream, ctx->d_result, n_groups, 1, ctx->d_result + 96, ctx->d_mail, seq));
	const int rc = mail_wait(ctx, seq);
	if (rc) return rc;
	mail_read(ctx, 0, 1, h_out);
	return BN_OK;
}

// h_out[i] = XOR_g d_vals[g * g_stride + i * i_stride], i < group_len <= 64, through the zero-copy mailbox: one tiny kernel and a
// spin on the sequence word instead of a device-to-host copy plus a stream synchronisation (~20 us less per call)
int publish_vals(bn_ctx *ctx, const f128 *d_vals, uint32_t n_groups, uint32_t group_len, uint32_t g_stride, uint32_t i_stride, f128 *h_out)
{
	const uint64_t seq = ++ctx->mail_seq;
	BN_HIP(bn::launch_xor_publish(ctx->stream, d_vals, n_groups, group_len, ctx->d_result + 64, ctx->d_mail, seq, g_stride, i_stride));
	const int rc = mail_wait(ctx, seq);
	if (rc) return rc;
	mail_read(ctx, 0, group_len, h_out);
	return BN_OK;
}

int upload_ptrs(bn_ctx *ctx, const void *const *ptrs, uint32_t n, const void ***d_ptrs)
{
	// use slots [128, 256) of the mailbox: 128 * 16 B = 2 KiB = 256 pointers
	BN_REQUIRE(n <= 256, "too many rows");
	void *dst = (void *)(ctx->d_result + 128);
	BN_HIP(hipMemcpyAsync(dst, ptrs, n * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
	BN_HIP(hipStreamSynchronize(ctx->stream));
	*d_ptrs = (const void **)dst;
	return BN_OK;
}

int ensure_d_steps(const bn_expr *e)
{
	if (e->d_steps || e->steps.empty()) return BN_OK;
	const size_t bytes = e->steps.size() * sizeof(bn_step);
	hipError_t err = hipMalloc((void **)&e->d_steps, bytes);
	if (err == hipSuccess) err = hipMemcpy(e->d_steps, e->steps.data(), bytes, hipMemcpyHostToDevice);
	if (err != hipSuccess) return bn::hip_fail(err, "bn_expr upload");
	return BN_OK;
}
} // namespace bnabi

// call_upload (abi_common.hpp): the scratch for every reserved section, the zeroed host mirror for the uploaded ones
int call_upload::alloc()
{
	scr = (char *)bn::ctx_scratch(ctx, bytes);
	if (!scr) return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (scratch)");
	mirror.assign(std::min(bytes, upload_bytes), 0);
	return BN_OK;
}

extern "C" {

const char *bn_last_error(void) { return g_last_error.c_str(); }
const char *bn_version(void) { return "binius_amd gfx950 abi-1"; }

// ---------------------------------------------------------------------------------- context
int bn_ctx_create(int device, uint64_t arena_elems, bn_ctx **out)
{
	if (!out)
		return bn::fail(BN_ERR_INPUT_VALIDATION, "input validation: out is null");
	int n_dev = 0;
	BN_HIP(hipGetDeviceCount(&n_dev));
	if (n_dev == 0)
		return bn::fail(BN_ERR_DEVICE, "device error: no HIP device visible (this backend has no CPU fallback)");
	BN_REQUIRE(device >= 0 && device < n_dev, "device ordinal out of range");
	BN_HIP(hipSetDevice(device));
	hipDeviceProp_t prop;
	BN_HIP(hipGetDeviceProperties(&prop, device));
	bn_ctx *ctx = new bn_ctx();
	ctx->device = device;
	ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	BN_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
	ctx->own_stream = true;
	BN_HIP(hipEventCreate(&ctx->ev0));
	BN_HIP(hipEventCreate(&ctx->ev1));
	BN_HIP(hipMalloc((void **)&ctx->d_result, sizeof(f128) * bn::kResultSlots));
	BN_HIP(hipHostMalloc((void **)&ctx->h_result, sizeof(f128) * bn::kResultSlots, hipHostMallocDefault));
	BN_HIP(hipHostMalloc((void **)&ctx->h_mail, sizeof(f128) * 128, hipHostMallocMapped | hipHostMallocCoherent));
	std::memset(ctx->h_mail, 0, sizeof(f128) * 128);
	BN_HIP(hipHostGetDevicePointer((void **)&ctx->d_mail, ctx->h_mail, 0));
	BN_HIP(hipMemset(ctx->d_result, 0, sizeof(f128) * bn::kResultSlots));
	ctx->s_clean = true;
	BN_HIP(hipMalloc((void **)&ctx->d_ticket, sizeof(unsigned)));
	BN_HIP(hipMemset(ctx->d_ticket, 0, sizeof(unsigned)));
	BN_HIP(hipMalloc((void **)&ctx->d_arm_relay, 8 * sizeof(uint64_t)));
	BN_HIP(hipMemset(ctx->d_arm_relay, 0, 8 * sizeof(uint64_t)));
	if (const char *a = getenv("BN_ARM")) ctx->arm_enabled = atoi(a) != 0;
	if (const char *a = getenv("BN_TWO_ROUND")) ctx->two_round = atoi(a) != 0;
	if (const char *a = getenv("BN_MLECHECK_SHADOW")) ctx->shadow_enabled = atoi(a) != 0;
	if (const char *a = getenv("BN_CIRCUIT_MULTIPASS")) ctx->circuit_multipass = atoi(a) != 0;
	if (const char *a = getenv("BN_GROUP")) ctx->grp.enabled = atoi(a) != 0;
	if (const char *a = getenv("BN_GROUP_SPEC")) ctx->grp.speculate = atoi(a) != 0;
	ctx->grp.prof = getenv("BN_GROUP_PROF") != nullptr;
	if (const char *a = getenv("BN_HAL_EQ_SET")) ctx->hal_eq_set = atoi(a) != 0;
	if (const char *a = getenv("BN_HAL_COEF")) ctx->hal_coef = atoi(a) != 0;
	if (const char *a = getenv("BN_GROUP_CHAIN_MIN_LOG2")) ctx->grp.chain_min_rows = atoi(a) >= 63 ? ~(uint64_t)0 : (uint64_t)1 << (atoi(a) < 0 ? 0 : atoi(a));
	BN_HIP(hipMalloc((void **)&ctx->d_flag, sizeof(unsigned)));
	BN_HIP(hipMemset(ctx->d_flag, 0, sizeof(unsigned)));
	BN_HIP(hipMalloc((void **)&ctx->d_s_evals, sizeof(uint64_t) * BN_NTT_MAX_DIM * BN_NTT_MAX_DIM));
	BN_HIP(hipMalloc((void **)&ctx->d_mul8, 65536));
	BN_HIP(bn::launch_build_mul8(ctx->stream, ctx->d_mul8));
	if (arena_elems) {
		hipError_t e = hipMalloc(&ctx->arena, arena_elems * sizeof(f128));
		if (e != hipSuccess) {
			bn_ctx_destroy(ctx);
			return bn::fail(BN_ERR_ALLOC, "allocation error: allocator is out of memory (device arena)");
		}
		ctx->arena_elems = arena_elems;
	}
	ctx->lazy_fold = getenv("BN_NO_LAZY_FOLD") == nullptr;
	{
		// host tail: pinned staging for Y (2 x 256 elements) and the nibble table of the host's basis change on the device
		const char *e = getenv("BN_HOST_TAIL");
		if (!(e && e[0] == '0') && bn::hostpoly_available()) {
			std::vector<uint64_t> phi(2048);
			bn::hostpoly_phi_nibble_table(phi.data());
			bn::hostpoly_phi_inv_nibble_table(phi.data() + 1024);
			BN_HIP(hipHostMalloc(&ctx->h_tail, 3 * bn::kHtMaxM * sizeof(f128), hipHostMallocMapped | hipHostMallocCoherent));
			BN_HIP(hipMalloc((void **)&ctx->d_ht_tag, sizeof(uint64_t)));
			BN_HIP(hipMemset(ctx->d_ht_tag, 0, sizeof(uint64_t)));
			BN_HIP(hipHostGetDevicePointer(&ctx->d_tail, ctx->h_tail, 0));
			BN_HIP(hipMalloc(&ctx->d_phi, 1024 * sizeof(f128)));
			BN_HIP(hipMemcpy(ctx->d_phi, phi.data(), 1024 * sizeof(f128), hipMemcpyHostToDevice));
			ctx->ht_enabled = true;
			// (with the host's folds on VPCLMULQDQ, four products per instruction, 2^12 elements are taken over -- measured
			// against 2^8 and 2^10: n = 20 0.239 / 0.235 / 0.229 ms, n = 24 0.772 / 0.759 / 0.748, n = 25 1.291 / 1.276 / 1.281;
			// with the scalar PCLMULQDQ loops 2^8)
			ctx->ht_max = bn::hostpoly_vectorized() ? 4096 : 256;
			if (const char *l = getenv("BN_HOST_TAIL_MAX_LOG2")) {
				const int v = atoi(l);
				ctx->ht_max = (uint64_t)1 << (v < 2 ? 2 : (v > 12 ? 12 : v));
			}
		}
	}
	// hosted sessions of the claim groups: same switch and same limit as the single-claim host tail (BN_GROUP_HT_MAX_LOG2 moves it; 0 = off)
	if (ctx->ht_enabled) {
		ctx->grp.ht_max = ctx->ht_max;
		if (const char *l = getenv("BN_GROUP_HT_MAX_LOG2")) {
			const int v = atoi(l);
			ctx->grp.ht_max = v <= 0 ? 0 : (uint64_t)1 << (v > 12 ? 12 : v);
		}
		if (const char *l = getenv("BN_GROUP_HT_WORK_LOG2")) {
			const int v = atoi(l);
			ctx->grp.ht_work = (uint64_t)1 << (v < 0 ? 0 : (v > 17 ? 17 : v));
		}
	}
	if (const char *t = getenv("BN_TAIL_MAX_LOG2")) {
		const int l = atoi(t);
		ctx->tail_max_cfg = (l >= 3 && l <= 12) ? (1ull << l) : 0; // one workgroup: at most 2^12 elements per array
	}
	ctx->tail_max_n_in = ctx->lazy_fold ? ctx->tail_max_cfg : 0;
	*out = ctx;
	return BN_OK;
}

// ---------------------------------------------------------------------------------- peer exchange (finalize.hpp)
static_assert(BN_PEER_MAX_WORLD == bn::kPeerMaxWorld && BN_PEER_MAILBOX_BYTES == bn::kPeerMailboxBytes, "header constants out of step");
static_assert(BN_PEER_HANDLE_BYTES >= sizeof(hipIpcMemHandle_t), "hipIpc handle does not fit");

static void peer_release(bn_ctx *ctx)
{
	bn_ctx::peer_state &ps = ctx->peer;
	for (uint32_t w = 0; w < ps.world; w++)
		if (ps.box[w] && w != ps.rank) (void)hipIpcCloseMemHandle(ps.box[w]);
	if (ps.own) (void)hipFree(ps.own);
	(void)hipGetLastError();
	ps = bn_ctx::peer_state{};
}

int bn_peer_create(bn_ctx *ctx, uint32_t world, uint32_t rank, uint8_t *handle_out)
{
	BN_REQUIRE(ctx && handle_out, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(world >= 1 && world <= (uint32_t)bn::kPeerMaxWorld && rank < world, "peer exchange: world must be 1..16 and rank < world");
	BN_REQUIRE(!ctx->peer.own, "peer exchange: already created on this context");
	// fine-grained (uncached at the device's L2) so that system-scope stores from the peers and system-scope loads of the
	// owner meet in memory; plain hipMalloc memory is cached non-coherently with respect to other agents
	void *p = nullptr;
	hipError_t e = hipExtMallocWithFlags(&p, bn::kPeerMailboxBytes, hipDeviceMallocUncached);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		e = hipExtMallocWithFlags(&p, bn::kPeerMailboxBytes, hipDeviceMallocFinegrained);
	}
	if (e != hipSuccess) return bn::hip_fail(e, "hipExtMallocWithFlags (peer mailbox)");
	e = hipMemset(p, 0, bn::kPeerMailboxBytes);
	hipIpcMemHandle_t h;
	if (e == hipSuccess) e = hipIpcGetMemHandle(&h, p);
	if (e != hipSuccess) {
		(void)hipFree(p);
		return bn::hip_fail(e, "hipIpcGetMemHandle (peer mailbox)");
	}
	std::memset(handle_out, 0, BN_PEER_HANDLE_BYTES);
	std::memcpy(handle_out, &h, sizeof(h));
	ctx->peer.world = world;
	ctx->peer.rank = rank;
	if (const char *st = getenv("BN_PEER_STRESS")) ctx->peer.stress = (uint32_t)atoi(st);
	ctx->peer.own = p;
	ctx->peer.box[rank] = p;
	return BN_OK;
}

int bn_peer_connect(bn_ctx *ctx, const uint8_t *handles)
{
	BN_REQUIRE(ctx && handles, "null argument");
	BN_ENTER(ctx);
	bn_ctx::peer_state &ps = ctx->peer;
	BN_REQUIRE(ps.own && !ps.connected, "peer exchange: bn_peer_create first (and connect once)");
	for (uint32_t w = 0; w < ps.world; w++) {
		if (w == ps.rank) continue;
		hipIpcMemHandle_t h;
		std::memcpy(&h, handles + (size_t)w * BN_PEER_HANDLE_BYTES, sizeof(h));
		void *p = nullptr;
		hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
		if (e != hipSuccess) {
			for (uint32_t v = 0; v < w; v++)
				if (v != ps.rank && ps.box[v]) {
					(void)hipIpcCloseMemHandle(ps.box[v]);
					ps.box[v] = nullptr;
				}
			return bn::hip_fail(e, "hipIpcOpenMemHandle (peer mailbox)");
		}
		ps.box[w] = p;
	}
	ps.connected = true;
	return BN_OK;
}

int bn_host_tail_allow_peer(bn_ctx *ctx, int on)
{
	BN_REQUIRE(ctx, "null argument");
	BN_ENTER(ctx);
	ctx->ht_peer_ok = on != 0;
	return BN_OK;
}

int bn_host_tail_active(bn_ctx *ctx, int *active)
{
	BN_REQUIRE(ctx && active, "null argument");
	BN_ENTER(ctx);
	*active = ctx->ht.active ? 1 : 0;
	return BN_OK;
}

int bn_peer_set_active(bn_ctx *ctx, int on)
{
	BN_REQUIRE(ctx, "null argument");
	BN_ENTER(ctx);
	if (ctx->ht.active && !on) {
		// a host tail is running: nothing is deferred on the device and nothing armed -- the caller takes over the exchange of
		// the host rounds' partial sums (bn_host_tail_allow_peer); no flush, the tail goes on
		ctx->peer.active = false;
		return BN_OK;
	}
	BN_FLUSH(ctx);
	BN_REQUIRE(!on || ctx->peer.connected, "peer exchange: not connected");
	if (ctx->peer.active != (on != 0)) arm_cancel(ctx); // (a kernel armed under the other setting would publish the wrong thing)
	ctx->peer.active = on != 0;
	return BN_OK;
}

int bn_peer_stats(bn_ctx *ctx, uint64_t *stats)
{
	BN_REQUIRE(ctx && stats, "null argument");
	BN_ENTER(ctx);
	stats[0] = ctx->peer.round;
	stats[1] = ctx->peer.connected ? ctx->peer.world : 0;
	return BN_OK;
}

int bn_peer_destroy(bn_ctx *ctx)
{
	BN_REQUIRE(ctx, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	arm_cancel(ctx);
	BN_HIP(hipStreamSynchronize(ctx->stream));
	peer_release(ctx);
	return BN_OK;
}

int bn_ctx_destroy(bn_ctx *ctx)
{
	if (!ctx)
		return BN_OK;
	hipSetDevice(ctx->device);
	if (ctx->grp.prof) {
		static const char *names[] = {"parse", "match", "plan", "launch", "wait", "answer", "hosted", "defer_fold", "hosted_start_wait", "hosted_start_copy", "hosted_fold"};
		fprintf(stderr, "[bn group prof] host us by phase:");
		for (int i = 0; i < bn_ctx::group_state::P_N; i++) fprintf(stderr, " %s %.1f (%llu)", names[i], ctx->grp.prof_ns[i] / 1e3, (unsigned long long)ctx->grp.prof_calls[i]);
		fprintf(stderr, "\n");
	}
	arm_cancel(ctx);
	if (ctx->stream)
		hipStreamSynchronize(ctx->stream);
	peer_release(ctx);
	if (ctx->d_arm_relay) hipFree(ctx->d_arm_relay);
	if (ctx->hal_const) hipFree(ctx->hal_const);
	if (ctx->h_mul_jobs) hipHostFree(ctx->h_mul_jobs);
	if (ctx->side) {
		hipStreamSynchronize(ctx->side);
		hipStreamDestroy(ctx->side);
		if (ctx->side_ev) hipEventDestroy(ctx->side_ev);
		if (ctx->main_ev) hipEventDestroy(ctx->main_ev);
	}
	if (ctx->d_flag) hipFree(ctx->d_flag);
	if (ctx->d_phi) hipFree(ctx->d_phi);
	if (ctx->d_ht_tag) hipFree(ctx->d_ht_tag);
	if (ctx->h_tail) hipHostFree(ctx->h_tail);
	if (ctx->grp.h_stage) hipHostFree(ctx->grp.h_stage);
	if (ctx->grp.h_tables) hipHostFree(ctx->grp.h_tables);
	if (ctx->grp.h_gmail) hipHostFree(ctx->grp.h_gmail);
	if (ctx->grp.d_S) hipFree(ctx->grp.d_S);
	if (ctx->shadow.S) hipFree(ctx->shadow.S);
	if (ctx->ntt_cache) {
		bn::ntt_bs_cache *nc = (bn::ntt_bs_cache *)ctx->ntt_cache;
		if (nc->d_tables) hipFree(nc->d_tables);
		delete nc;
	}
	if (ctx->arena) hipFree(ctx->arena);
	if (ctx->scratch) hipFree(ctx->scratch);
	if (ctx->d_result) hipFree(ctx->d_result);
	if (ctx->d_mul8) hipFree(ctx->d_mul8);
	if (ctx->d_s_evals) hipFree(ctx->d_s_evals);
	if (ctx->d_ticket) hipFree(ctx->d_ticket);
	if (ctx->h_result) hipHostFree(ctx->h_result);
	if (ctx->h_mail) hipHostFree(ctx->h_mail);
	if (ctx->h_me_rets) hipHostFree(ctx->h_me_rets);
	if (ctx->h_gather) hipHostFree(ctx->h_gather);
	if (ctx->ev0) hipEventDestroy(ctx->ev0);
	if (ctx->ev1) hipEventDestroy(ctx->ev1);
	for (auto &r : ctx->prof) {
		hipEventDestroy(r.a);
		hipEventDestroy(r.b);
	}
	for (auto e : ctx->ev_pool) hipEventDestroy(e);
	if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
	delete ctx;
	return BN_OK;
}

int bn_arena_base(bn_ctx *ctx, void **d_base, uint64_t *elems)
{
	BN_REQUIRE(ctx && d_base && elems, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	*d_base = ctx->arena;
	*elems = ctx->arena_elems;
	return BN_OK;
}

int bn_ctx_set_stream(bn_ctx *ctx, void *hip_stream)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_HIP(hipSetDevice(ctx->device));
	BN_HIP(hipStreamSynchronize(ctx->stream));
	if (hip_stream == nullptr) {
		if (!ctx->own_stream) {
			BN_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
			ctx->own_stream = true;
			ctx->lazy_fold = getenv("BN_NO_LAZY_FOLD") == nullptr;
			ctx->tail_max_n_in = ctx->lazy_fold ? ctx->tail_max_cfg : 0; // (the resident tail comes back with the deferral)
		}
		return BN_OK;
	}
	if (ctx->own_stream)
		hipStreamDestroy(ctx->stream);
	ctx->stream = (hipStream_t)hip_stream;
	ctx->own_stream = false;
	// On a stream the caller also enqueues on, deferred folds/copies would be visible: work the caller
	// puts on the stream right after bn_extrapolate_line would run BEFORE the fold.  Deferral is
	// therefore off on caller-supplied streams unless the caller opts in (BN_LAZY_ON_SHARED_STREAM=1)
	// and promises to call bn_ctx_get_stream / bn_sync (both flush) before touching the stream itself.
	ctx->lazy_fold = getenv("BN_NO_LAZY_FOLD") == nullptr && getenv("BN_LAZY_ON_SHARED_STREAM") != nullptr;
	ctx->tail_max_n_in = ctx->lazy_fold ? ctx->tail_max_cfg : 0;
	return BN_OK;
}

int bn_ctx_get_stream(bn_ctx *ctx, void **hip_stream)
{
	BN_REQUIRE(ctx && hip_stream, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	*hip_stream = (void *)ctx->stream;
	return BN_OK;
}

int bn_sync(bn_ctx *ctx)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_HIP(hipStreamSynchronize(ctx->stream));
	return BN_OK;
}

int bn_prof_begin(bn_ctx *ctx)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	for (auto &r : ctx->prof) {
		ctx->ev_pool.push_back(r.a);
		ctx->ev_pool.push_back(r.b);
	}
	ctx->prof.clear();
	ctx->prof_on = true;
	return BN_OK;
}

int bn_prof_end(bn_ctx *ctx, double *ms_by_class, uint64_t *launches_by_class)
{
	BN_REQUIRE(ctx && ms_by_class && launches_by_class, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	ctx->prof_on = false;
	BN_HIP(hipStreamSynchronize(ctx->stream));
	for (int i = 0; i < BN_PROF_N; i++) {
		ms_by_class[i] = 0;
		launches_by_class[i] = 0;
	}
	for (auto &r : ctx->prof) {
		float ms = 0;
		BN_HIP(hipEventElapsedTime(&ms, r.a, r.b));
		ms_by_class[r.cls] += ms;
		launches_by_class[r.cls] += 1;
		ctx->ev_pool.push_back(r.a);
		ctx->ev_pool.push_back(r.b);
	}
	ctx->prof.clear();
	return BN_OK;
}

int bn_timer_begin(bn_ctx *ctx)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_HIP(hipEventRecord(ctx->ev0, ctx->stream));
	return BN_OK;
}

int bn_timer_end_ms(bn_ctx *ctx, float *ms)
{
	BN_REQUIRE(ctx && ms, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_HIP(hipEventRecord(ctx->ev1, ctx->stream));
	BN_HIP(hipEventSynchronize(ctx->ev1));
	BN_HIP(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
	return BN_OK;
}

// ---------------------------------------------------------------------------------- ComputeLayer
int bn_copy_h2d(bn_ctx *ctx, const bn_f128 *h_src, uint64_t src_len, void *d_dst, uint64_t dst_len)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_REQUIRE(src_len == dst_len, "precondition: src and dst buffers must have the same length");
	if (src_len == 0) return BN_OK;
	BN_HIP(hipMemcpyAsync(d_dst, h_src, src_len * sizeof(f128), hipMemcpyHostToDevice, ctx->stream));
	// the host buffer is caller-owned pageable memory: make the copy complete before returning
	BN_HIP(hipStreamSynchronize(ctx->stream));
	return BN_OK;
}

int bn_copy_d2h(bn_ctx *ctx, const void *d_src, uint64_t src_len, bn_f128 *h_dst, uint64_t dst_len)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	{
		// a read does not invalidate the host mirror of a tiny fold -- and may create it.  Of the claim groups' deferred folds only
		// those that touch what is read run (the final evaluations of a prover that finishes while the others go on,
		// front_loaded.rs:100-112): the rest stays deferred for the next round's launch
		int rc_ = flush_legacy(ctx, false, /*publish_tiny=*/ctx->lazy_fold);
		if (rc_) return rc_;
		// (a hosted prover's current arrays -- finish()'s reads of the final evaluations -- come from the host's copies)
		if (src_len == dst_len && src_len && group_host_read(ctx, d_src, src_len, h_dst)) return BN_OK;
		rc_ = group_flush_touching(ctx, d_src, src_len, /*publish_tiny=*/ctx->lazy_fold, /*write=*/false);
		if (rc_) return rc_;
	}
	BN_REQUIRE(src_len == dst_len, "precondition: src and dst buffers must have the same length");
	if (src_len == 0) return BN_OK;
	if (ctx->mirror.valid) {
		for (uint32_t i = 0; i < ctx->mirror.count; i++) {
			const char *base = (const char *)ctx->mirror.ptr[i];
			const char *p = (const char *)d_src;
			if (p >= base && p + src_len * sizeof(f128) <= base + (size_t)ctx->mirror.n * sizeof(f128)) {
				if (ctx->mirror.host) { // (n = 1: one element per array, computed on the host in flush_pending)
					h_dst[0].lo = ctx->mirror.host_vals[i].lo;
					h_dst[0].hi = ctx->mirror.host_vals[i].hi;
					return BN_OK;
				}
				const int rc = mail_wait(ctx, ctx->mirror.seq);
				if (rc) return rc;
				const size_t off = (size_t)i * ctx->mirror.n + (size_t)(p - base) / sizeof(f128);
				mail_read(ctx, (uint32_t)off, (uint32_t)src_len, h_dst);
				return BN_OK;
			}
		}
	}
	BN_HIP(hipMemcpyAsync(h_dst, d_src, src_len * sizeof(f128), hipMemcpyDeviceToHost, ctx->stream));
	BN_HIP(hipStreamSynchronize(ctx->stream));
	return BN_OK;
}

int bn_copy_d2d(bn_ctx *ctx, const void *d_src, uint64_t src_len, void *d_dst, uint64_t dst_len)
{
	BN_REQUIRE(ctx, "null ctx");
	BN_ENTER(ctx);
	BN_REQUIRE(src_len == dst_len, "precondition: src and dst buffers must have the same length");
	if (src_len == 0) return BN_OK;
	ctx->mirror.valid = false;
	if (ctx->pre.valid) {
		// a copy INTO the arrays the precomputed next-round sums describe makes them stale (a copy out of them -- the first
		// fold's "copy evals_0 into a fresh buffer" -- does not)
		const char *d0 = (const char *)d_dst, *d1 = d0 + dst_len * sizeof(f128);
		const size_t half = (size_t)(ctx->pre.m / 2) * sizeof(f128);
		for (int j = 0; j < 2; j++)
			for (const void *b : {ctx->pre.lo[j], ctx->pre.hi[j]})
				if (d0 < (const char *)b + half && (const char *)b < d1) ctx->pre.valid = false;
	}
	if (ctx->ht.active) {
		// a host tail: with folds outstanding the device arrays are stale (the chain runs first); with none, the host only holds
		// a copy -- which a write into the arrays ends
		const bn_ctx::host_tail_state &ht = ctx->ht;
		bool hit = ht.n_levels > 0;
		for (int j = 0; j < 2 && !hit; j++)
			hit = ranges_overlap(d_dst, dst_len, ht.cur_lo[j], ht.cur_m / 2) || ranges_overlap(d_dst, dst_len, ht.cur_hi[j], ht.cur_m / 2);
		if (hit) BN_FLUSH(ctx);
	}
	if (shadow_touched_by_write(ctx, d_dst, dst_len)) {
		// a write into an array the MLE-check shadow describes (the caller's a / b, the table or the noted copy of its lower
		// half, S itself): everything deferred runs first, in issue order, the side stream is joined and the shadow ends --
		// the literal kernels answer from here on (a deferred or side-queued copy must not leave S stale)
		BN_FLUSH(ctx);
		BN_HIP(hipMemcpyAsync(d_dst, d_src, src_len * sizeof(f128), hipMemcpyDeviceToDevice, ctx->stream));
		return BN_OK;
	}
	if (!group_independent(ctx, d_src, src_len, false) || !group_independent(ctx, d_dst, dst_len, true)) BN_FLUSH(ctx); // (ordered behind the deferred folds / hosted provers it touches)
	group_note_write(ctx, d_dst, dst_len); // (sums computed ahead from what is overwritten are stale)
	if (ctx->lazy_fold && !ctx->pend.active && ctx->pend_copies.size() < (size_t)bn::kFoldCallMax) { // (one per multilinear of the widest prover's first fold)
		// deferred: a fold into d_dst may absorb it (see bn_ctx::pending_copy)
		ctx->pend_copies.push_back({d_src, d_dst, src_len});
		return BN_OK;
	}
	if (ctx->pend.active && !ctx->pend2.active && ctx->pend_copies.empty() && !ctx->tail.active &&
	    independent_of_pending(ctx, d_src, src_len) && independent_of_pending(ctx, d_dst, dst_len)) {
		// A copy that touches none of the arrays of the deferred fold commutes with it: it runs now and the fold stays
		// deferred (the MLE-check prover copies the lower half of its indicator table between a fold and the next round
		// evaluation, v3/bivariate_mlecheck.rs:195-254).
		bn_ctx::shadow_state &sh = ctx->shadow;
		if (sh.valid && d_src == sh.eq && 2 * src_len == sh.eq_len) {
			// (writes INTO the shadow's arrays never get here: shadow_touched_by_write above)
			BN_SHDBG("copy of the table's lower half noted");
			sh.eq_copy_src = d_src;
			sh.eq_copy_dst = d_dst;
		}
		if (sh.valid)
			ctx->side_queue.push_back({bn_ctx::side_op::COPY, d_dst, d_src, nullptr, src_len, f128{0, 0}}); // (launched behind the next round's kernel)
		else
			BN_HIP(hipMemcpyAsync(d_dst, d_src, src_len * sizeof(f128), hipMemcpyDeviceToDevice, ctx->stream));
		return BN_OK;
	}
	BN_FLUSH(ctx);
	BN_HIP(hipMemcpyAsync(d_dst, d_src, src_len * sizeof(f128), hipMemcpyDeviceToDevice, ctx->stream));
	return BN_OK;
}

int bn_fill(bn_ctx *ctx, void *d_dst, uint64_t n, const bn_f128 *value)
{
	BN_REQUIRE(ctx && value, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	BN_HIP(bn::launch_fill(ctx->stream, d_dst, n, to_f(value)));
	return BN_OK;
}

// ---------------------------------------------------------------------------------- expressions
int bn_expr_compile(bn_ctx *ctx, const bn_step *steps, uint64_t n_steps, bn_expr **out)
{
	BN_REQUIRE(ctx && out, "null argument");
	BN_ENTER(ctx);
	BN_REQUIRE(n_steps == 0 || steps, "null steps");
	bn_expr *e = new bn_expr();
	e->device = ctx->device;
	e->steps.assign(steps, steps + n_steps);
	uint32_t n_vars = 0;
	// symbolic pass: which steps are pure products of variables?
	std::vector<std::vector<uint32_t>> prod(n_steps);
	std::vector<bool> is_prod(n_steps, false);
	for (uint64_t s = 0; s < n_steps; s++) {
		const bn_step &st = steps[s];
		switch (st.kind) {
		case BN_STEP_VAR:
			if (st.a + 1 > n_vars) n_vars = st.a + 1;
			is_prod[s] = true;
			prod[s] = {st.a};
			break;
		case BN_STEP_ADD:
		case BN_STEP_MUL:
			if (st.a >= s || st.b >= s) {
				delete e;
				return bn::fail(BN_ERR_INPUT_VALIDATION, "input validation: circuit step refers to a later step");
			}
			if (st.kind == BN_STEP_MUL && is_prod[st.a] && is_prod[st.b]) {
				is_prod[s] = true;
				prod[s] = prod[st.a];
				prod[s].insert(prod[s].end(), prod[st.b].begin(), prod[st.b].end());
			}
			break;
		case BN_STEP_POW:
			if (st.a >= s) {
				delete e;
				return bn::fail(BN_ERR_INPUT_VALIDATION, "input validation: circuit step refers to a later step");
			}
			break;
		case BN_STEP_CONST:
			break;
		default:
			delete e;
			return bn::fail(BN_ERR_INPUT_VALIDATION, "input validation: unknown circuit step kind");
		}
	}
	e->n_vars = n_vars;
	if (n_steps && is_prod[n_steps - 1] && prod[n_steps - 1].size() <= 4) {
		e->shape = bn_expr::PRODUCT;
		e->product_vars = prod[n_steps - 1];
	}
	// the device copy of the steps is only needed by the generic interpreter kernels: uploaded on
	// first use (ensure_d_steps), so compiling a product composition touches no device memory
	*out = e;
	return BN_OK;
}

// (the compiler itself -- level inference, dead-step removal, slot assignment -- is compose_tower.hpp; the program goes to the
// device at the first bn_compute_composite, as d_steps does)
int bn_expr_compile_tower(bn_ctx *ctx, const bn_step *steps, uint64_t n_steps, const uint32_t *input_levels, uint32_t n_inputs, uint32_t out_level,
                          bn_expr **out)
{
	BN_REQUIRE(ctx && out && steps && input_levels, "null argument");
	BN_ENTER(ctx);
	std::unique_ptr<bn::ct_program> prog(new bn::ct_program());
	const char *why = bn::ct_compile(steps, n_steps, input_levels, n_inputs, out_level, *prog);
	if (why) return bn::fail(BN_ERR_INPUT_VALIDATION, std::string("input validation: tower expression: ") + why);
	bn_expr *e = new bn_expr();
	e->device = ctx->device;
	e->steps.assign(steps, steps + n_steps);
	e->n_vars = n_inputs;
	e->tower = std::move(prog);
	*out = e;
	return BN_OK;
}

// (the plan -- duplicate programs dropped, job table, classes, LDS, the sweep over the outputs, the upload layout -- is
// compose_batch.hpp; nothing goes to the device here: the tables travel with each bn_compute_composite)
int bn_expr_compile_tower_batch(bn_ctx *ctx, const bn_expr *const *exprs, uint32_t n_exprs, const uint32_t *job_desc, const uint64_t *out_offsets, uint32_t n_jobs,
                                bn_expr **out)
{
	BN_REQUIRE(ctx && out && exprs && job_desc && out_offsets, "null argument");
	BN_ENTER(ctx);
	BN_REQUIRE(n_jobs >= 1 && n_jobs <= BN_COMPOSE_BATCH_MAX_JOBS, "tower batch: the number of jobs is 0 or above BN_COMPOSE_BATCH_MAX_JOBS");
	std::vector<bn_compose_job> jobs(n_jobs);
	for (uint32_t j = 0; j < n_jobs; j++) {
		const uint32_t *d = job_desc + (size_t)BN_COMPOSE_JOB_DESC_WORDS * j;
		jobs[j] = bn_compose_job{d[0], d[1], d[2], d[3], out_offsets[j]};
	}
	std::vector<const bn::ct_program *> progs(n_exprs, nullptr);
	for (uint32_t i = 0; i < n_exprs; i++) {
		BN_REQUIRE(exprs[i], "null argument");
		BN_REQUIRE(exprs[i]->tower != nullptr, "tower batch: a member is not a tower expression");
		BN_REQUIRE(exprs[i]->device == ctx->device, "tower batch: a member was compiled for another device");
		progs[i] = exprs[i]->tower.get();
	}
	std::unique_ptr<bn::compose_batch_plan> plan(new bn::compose_batch_plan());
	const char *why = bn::cb_plan(progs.data(), n_exprs, jobs.data(), n_jobs, *plan);
	if (why) return bn::fail(BN_ERR_INPUT_VALIDATION, std::string("input validation: tower batch: ") + why);
	bn_expr *e = new bn_expr();
	e->device = ctx->device;
	e->n_vars = plan->n_rows;
	e->tower_batch = std::move(plan);
	*out = e;
	return BN_OK;
}

} // extern "C"
namespace bn {
static std::atomic<uint64_t> g_expr_epoch{1};
uint64_t expr_epoch() { return g_expr_epoch.load(std::memory_order_relaxed); }
void expr_epoch_bump() { g_expr_epoch.fetch_add(1, std::memory_order_relaxed); }
} // namespace bn
extern "C" {

int bn_expr_free(bn_expr *expr)
{
	if (!expr) return BN_OK;
	bn::expr_epoch_bump();
	if (expr->d_steps) hipFree(expr->d_steps);
	if (expr->d_tower) hipFree(expr->d_tower);
	delete expr;
	return BN_OK;
}

int bn_expr_n_vars(const bn_expr *expr, uint32_t *n_vars)
{
	BN_REQUIRE(expr && n_vars, "null argument");
	*n_vars = expr->n_vars;
	return BN_OK;
}

int bn_arm_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	counters[BN_ARM_HITS] = ctx->arm_hits;
	counters[BN_ARM_CANCELS] = ctx->arm_cancels;
	counters[BN_ARM_EXPIRED] = ctx->arm_expired;
	counters[BN_ARM_NS_WAIT] = ctx->arm_ns_wait;
	counters[BN_ARM_NS_LAUNCH] = ctx->arm_ns_launch;
	counters[BN_ARM_NS_PARSE] = ctx->arm_ns_parse;
	counters[BN_ARM_HOSTED] = ctx->two_round_hosted;
	counters[BN_ARM_TWO_ROUND] = ctx->two_round_launches;
	counters[BN_ARM_SHADOW_CREATED] = ctx->shadow_created;
	counters[BN_ARM_SHADOW_ROUNDS] = ctx->shadow_rounds;
	counters[BN_ARM_SHADOW_DROPPED] = ctx->shadow_dropped;
	counters[BN_ARM_HT_STARTED] = ctx->ht_started;
	counters[BN_ARM_HT_ROUNDS] = ctx->ht_rounds;
	counters[BN_ARM_HT_FLUSHED] = ctx->ht_flushed;
	counters[BN_ARM_HT_MAX] = ctx->ht_enabled ? ctx->ht_max : 0;
	return BN_OK;
}

int bn_group_counters(bn_ctx *ctx, uint64_t *counters)
{
	BN_REQUIRE(ctx && counters, "null argument");
	BN_ENTER(ctx);
	const auto &g = ctx->grp;
	counters[BN_GROUP_LAUNCHES] = g.launches;
	counters[BN_GROUP_JOBS_FUSED] = g.jobs_fused;
	counters[BN_GROUP_JOBS_EVAL] = g.jobs_eval;
	counters[BN_GROUP_PREFOLDS] = g.prefolds;
	counters[BN_GROUP_SPEC_JOBS] = g.spec_jobs;
	counters[BN_GROUP_SPEC_HITS] = g.spec_hits;
	counters[BN_GROUP_EVALS] = g.evals;
	counters[BN_GROUP_FLUSHED_FOLDS] = g.flushed_folds;
	counters[BN_GROUP_HOSTED_STARTED] = g.hosted_started;
	counters[BN_GROUP_HOSTED_EVALS] = g.hosted_evals;
	counters[BN_GROUP_HOSTED_FOLDS] = g.hosted_folds;
	counters[BN_GROUP_HOSTED_WRITEBACKS] = g.hosted_writebacks;
	counters[BN_GROUP_JOBS_FOLD] = g.jobs_fold;
	counters[BN_GROUP_CHAINS] = g.chain_count;
	return BN_OK;
}

int bn_fp4_last_grids(bn_ctx *ctx, uint64_t *grids)
{
	BN_REQUIRE(ctx && grids, "null argument");
	BN_ENTER(ctx);
	const bn::fp4_grid_record &g = bn::fp4_last_grids();
	grids[BN_FP4_RE_GRID] = g.re_grid.load(std::memory_order_relaxed);
	grids[BN_FP4_RE_TILES] = g.re_tiles.load(std::memory_order_relaxed);
	grids[BN_FP4_RE_WS] = g.re_ws.load(std::memory_order_relaxed);
	grids[BN_FP4_FE_GRID] = g.fe_grid.load(std::memory_order_relaxed);
	grids[BN_FP4_FE_TILES] = g.fe_tiles.load(std::memory_order_relaxed);
	grids[BN_FP4_RE_MAX_TILES] = g.re_max_tiles.load(std::memory_order_relaxed);
	grids[BN_FP4_FE_MAX_TILES] = g.fe_max_tiles.load(std::memory_order_relaxed);
	return BN_OK;
}

int bn_host_scratch(bn_ctx *ctx, void **h_ptr, void **d_ptr, uint64_t *elems)
{
	BN_REQUIRE(ctx && h_ptr && d_ptr && elems, "null argument");
	BN_ENTER(ctx);
	BN_FLUSH(ctx);
	*h_ptr = ctx->h_mail + 96;
	*d_ptr = ctx->d_mail + 96;
	*elems = 32;
	return BN_OK;
}

int bn_device_numa_node(int device, int *node)
{
	BN_REQUIRE(node, "null argument");
	*node = -1;
	char bdf[64] = {0};
	BN_HIP(hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf) - 1, device));
	for (char *c = bdf; *c; c++)
		if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a'); // sysfs spells the address in lower case
	const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/numa_node";
	if (FILE *f = fopen(path.c_str(), "r")) {
		int v = -1;
		if (fscanf(f, "%d", &v) == 1) *node = v;
		fclose(f);
	}
	return BN_OK;
}

// XOR of n_groups device vectors of group_len (<= 64) elements, returned to the host through the
// zero-copy mailbox.  Not part of the reference interface: it is the combine step behind the
// per-round all_gather of the sharded prover (binius_amd/host/host_capi.cpp).
// ---------------------------------------------------------------------------------- host scalars
int bn_scalar_mul(const bn_f128 *a, const bn_f128 *b, bn_f128 *out)
{
	BN_REQUIRE(a && b && out, "null argument");
	f128 r = bn::mul_host(to_f(a), to_f(b)); // hostmul.hpp: table-based tower Karatsuba
	out->lo = r.lo;
	out->hi = r.hi;
	return BN_OK;
}

int bn_scalar_invert(const bn_f128 *a, bn_f128 *out)
{
	BN_REQUIRE(a && out, "null argument");
	// invert_or_zero semantics (0 -> 0); tower descent, ~1 us on the host
	f128 r = bn::invert_tower(to_f(a));
	if (a->lo == 0 && a->hi == 0) r = bn::f128_zero();
	out->lo = r.lo;
	out->hi = r.hi;
	return BN_OK;
}

} // extern "C"
