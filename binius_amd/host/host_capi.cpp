// binius_amd/host/host_capi.cpp -> libbinius_amd_host.so
//
// The compiled form of the C++ host mirror: a complete prover run behind one C call, so a benchmark or a test times the prover
// loop the way a compiled (Rust) host would drive the HAL -- for the BivariateSumcheckProver per round one accumulate_kernels, two
// scalar multiplications, one extrapolate_line per multilinear -- without interpreter overhead between HAL calls.  One entry point
// per mirror (sumcheck.hpp, sharded_sumcheck.hpp, batch_prover.hpp, eq_ind.hpp, fri.hpp, piop.hpp, gkr_gpa.hpp, gkr_exp.hpp, flush.hpp, evalcheck.hpp,
// zerocheck.hpp, ring_switch.hpp): it converts the C arrays (from_raw / to_raw), runs inside guarded(), which turns what is thrown into the return
// code and bnh_last_error().  Links only against the C ABI of include/binius_amd.h.
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/binius_amd_host.h"
#include "batch_prover.hpp"
#include "eq_ind.hpp"
#include "evalcheck.hpp"
#include "flush.hpp"
#include "fri.hpp"
#include "gkr_exp.hpp"
#include "gkr_gpa.hpp"
#include "piop.hpp"
#include "ring_switch.hpp"
#include "sharded_sumcheck.hpp"
#include "sumcheck.hpp"
#include "transcript.hpp"
#include "witness.hpp"
#include "zerocheck.hpp"

using namespace binius_amd;

namespace {
thread_local std::string g_err;

// ---- RCCL, bound at run time from the librccl.so the process already uses (torch's) -----------
struct rccl_unique_id {
	char internal[128];
};
typedef int (*fn_get_unique_id)(rccl_unique_id *);
typedef int (*fn_comm_init_rank)(void **comm, int nranks, rccl_unique_id id, int rank);
typedef int (*fn_all_gather)(const void *send, void *recv, size_t count, int dtype, void *comm, void *stream);
typedef int (*fn_comm_destroy)(void *comm);
typedef const char *(*fn_get_error_string)(int);
struct rccl_api {
	void *lib = nullptr;
	fn_get_unique_id get_unique_id = nullptr;
	fn_comm_init_rank comm_init_rank = nullptr;
	fn_all_gather all_gather = nullptr;
	fn_comm_destroy comm_destroy = nullptr;
	fn_get_error_string err = nullptr;
} g_rccl;
constexpr int kNcclUint8 = 1; // ncclDataType_t

// n product claims over m multilinears, as the C callers pass them: two indices per claim
std::vector<IndexCompositionBivariate> index_compositions(uint32_t m, uint32_t n, const uint32_t *comp_indices)
{
	std::vector<IndexCompositionBivariate> comps;
	for (uint32_t c = 0; c < n; c++) comps.push_back(IndexCompositionBivariate{m, {comp_indices[2 * c], comp_indices[2 * c + 1]}});
	return comps;
}

// the truncated quadratic round proofs (two coefficients a round, missing ones zero) and the provers' final evaluations, concatenated
void put_batch_output(const BatchSumcheckOutput &out, bn_f128 *round_proofs_out, bn_f128 *final_evals_out)
{
	for (size_t r = 0; r < out.round_proofs.size(); r++)
		for (size_t i = 0; i < 2; i++) round_proofs_out[2 * r + i] = i < out.round_proofs[r].size() ? out.round_proofs[r][i].raw() : bn_f128{0, 0};
	for (const auto &evals : out.multilinear_evals) final_evals_out = to_raw(evals, final_evals_out);
}

// GkrGpaOutput but its timings: per claim the product, the final evaluation and the final point, per step the round proofs and the
// layer evaluations, each concatenated
void put_gkr_gpa_output(const GkrGpaOutput &out, bn_f128 *products_out, bn_f128 *round_proofs_out, bn_f128 *layer_evals_out, bn_f128 *final_points_out,
                        bn_f128 *final_evals_out)
{
	to_raw(out.products, products_out);
	to_raw(out.final_evals, final_evals_out);
	for (const auto &pt : out.final_points) final_points_out = to_raw(pt, final_points_out);
	for (const auto &rp : out.round_proofs) round_proofs_out = to_raw(rp, round_proofs_out);
	for (const auto &le : out.layer_evals) layer_evals_out = to_raw(le, layer_evals_out);
}

// The transcript of an entry point: the caller's table (the _live form: a null table or a null callback it needs is rejected at once,
// before anything is launched) or the sample arrays of the array form, as the streams the mirror numbers.
struct EntryTranscript {
	std::unique_ptr<LiveTranscript> live;
	std::vector<std::vector<B128>> arrays;
	std::unique_ptr<ArrayTranscript> array;
	EntryTranscript(bool is_live, const bnh_transcript *table, bool need_bits = false)
	{
		if (is_live) live = std::make_unique<LiveTranscript>(table, need_bits);
	}
	TranscriptSource &source(std::vector<std::vector<B128>> streams, const uint64_t *bits = nullptr, size_t n_bits = 0)
	{
		if (live) return *live;
		arrays = std::move(streams);
		std::vector<ArrayTranscript::Stream> views;
		for (const auto &v : arrays) views.push_back(ArrayTranscript::stream(v));
		array = std::make_unique<ArrayTranscript>(std::move(views), bits, n_bits);
		return *array;
	}
};
// a single sample of the array form as a stream of one (empty when the pointer is null: the _live form)
std::vector<B128> one_sample(const bn_f128 *p) { return from_raw(p, p ? 1 : 0); }

// the body of an entry point: what it throws becomes the return code, the message goes to bnh_last_error()
template <class F>
int guarded(F &&body)
{
	try {
		return body();
	} catch (const Error &e) {
		g_err = e.what();
		return (int)e.kind();
	} catch (const std::exception &e) {
		g_err = e.what();
		return BN_ERR_CORE_LIB;
	}
}

// rccl, the fourth transport of the sharded prover (sharded_sumcheck.hpp), for ranks that do not share a node: the partial stays on
// the device; ONE collective per round, ncclAllGather of the rank's 32 bytes on the context's stream (stream-ordered after the
// kernels), then the XOR of the partials on the device, its result through the zero-copy mailbox
class RcclExchange : public RoundExchange {
public:
	RcclExchange(bn_ctx *ctx, void *comm, void *d_partial, void *d_gathered, int world)
	    : ctx_(ctx), comm_(comm), d_partial_(d_partial), d_gathered_(d_gathered), world_(world)
	{
	}
	void *device_partial() const override { return d_partial_; }
	std::vector<B128> combine(const std::vector<B128> &) override
	{
		if (g_rccl.all_gather(d_partial_, d_gathered_, 32, kNcclUint8, comm_, stream()) != 0) throw Error(Error::DeviceError, "ncclAllGather failed");
		bn_f128 ev[2];
		check(bn_xor_reduce(ctx_, d_gathered_, (uint32_t)world_, 2, ev));
		return from_raw(ev, 2);
	}
	// one ncclAllGather per multilinear (16 bytes per rank) rebuilds the residual multilinears in device scratch
	std::vector<FSlice> gather_residual(ComputeLayer &, DeviceBumpAllocator &dev_alloc, const std::vector<FSlice> &finals) override
	{
		void *s = stream(); // flushes the deferred last fold
		std::vector<FSliceMut> res;
		for (size_t j = 0; j < finals.size(); j++) res.push_back(dev_alloc.alloc((size_t)world_));
		for (size_t j = 0; j < finals.size(); j++)
			if (g_rccl.all_gather(finals[j].ptr, res[j].ptr, 16, kNcclUint8, comm_, s) != 0)
				throw Error(Error::DeviceError, "ncclAllGather (residual multilinears) failed");
		std::vector<FSlice> out;
		for (const auto &r : res) out.push_back(ComputeMemory::as_const(r));
		return out;
	}

private:
	void *stream() const
	{
		void *s = nullptr;
		check(bn_ctx_get_stream(ctx_, &s));
		return s;
	}
	bn_ctx *ctx_;
	void *comm_, *d_partial_, *d_gathered_;
	int world_;
};

// the transport of one sharded prove, by what the caller passed: the peer mailboxes, else the shared-memory segment, else the RCCL
// communicator, else the reduce callback
std::unique_ptr<RoundExchange> choose_exchange(bn_ctx *ctx, bool peer, void *shm, void *rccl_comm, bnh_round_reduce_fn reduce, void *reduce_user,
                                               void *d_partial, void *d_gathered, int world)
{
	if (peer) return std::make_unique<PeerExchange>(ctx, shm, world);
	if (shm) return std::make_unique<ShmExchange>(ctx, shm, world);
	if (rccl_comm) return std::make_unique<RcclExchange>(ctx, rccl_comm, d_partial, d_gathered, world);
	return std::make_unique<CallbackExchange>(reduce, reduce_user, d_partial);
}
} // namespace

extern "C" {

const char *bnh_last_error(void) { return g_err.c_str(); }

// ---- the array-backed transcript: samples served from arrays, every write recorded; pure host code, no context ------------------
struct bnh_transcript_replay {
	bnh_transcript table{};
	std::vector<bn_f128> samples;
	std::vector<uint64_t> bit_samples;
	size_t next_sample = 0, next_bits = 0;
	std::vector<uint8_t> written[2]; // per channel
	std::vector<std::pair<uint32_t, uint64_t>> events; // (kind, bytes or samples); neighbours of one kind are one event
	void log(uint32_t kind, uint64_t count)
	{
		if (!events.empty() && events.back().first == kind)
			events.back().second += count;
		else
			events.emplace_back(kind, count);
	}
};
static int replay_write(void *user, uint32_t channel, const void *bytes, uint64_t len)
{
	bnh_transcript_replay *h = (bnh_transcript_replay *)user;
	if (!h || channel > BNH_TR_DECOMMITMENT || (len && !bytes)) return 1;
	if (!len) return 0;
	h->written[channel].insert(h->written[channel].end(), (const uint8_t *)bytes, (const uint8_t *)bytes + len);
	h->log(channel == BNH_TR_MESSAGE ? BNH_TR_EVENT_WRITE_MESSAGE : BNH_TR_EVENT_WRITE_DECOMMITMENT, len);
	return 0;
}
static int replay_sample(void *user, bn_f128 *out, uint32_t n)
{
	bnh_transcript_replay *h = (bnh_transcript_replay *)user;
	if (!h || (n && !out) || h->samples.size() - h->next_sample < n) return 1;
	for (uint32_t i = 0; i < n; i++) out[i] = h->samples[h->next_sample++];
	if (n) h->log(BNH_TR_EVENT_SAMPLE, n);
	return 0;
}
static int replay_sample_bits(void *user, uint32_t bits, uint32_t n, uint64_t *out)
{
	bnh_transcript_replay *h = (bnh_transcript_replay *)user;
	if (!h || (n && !out) || bits > 64 || h->bit_samples.size() - h->next_bits < n) return 1;
	for (uint32_t i = 0; i < n; i++) out[i] = h->bit_samples[h->next_bits++] & (bits == 64 ? ~(uint64_t)0 : (((uint64_t)1 << bits) - 1));
	if (n) h->log(BNH_TR_EVENT_SAMPLE_BITS, n);
	return 0;
}

int bnh_transcript_replay_new(const bn_f128 *samples, uint64_t n_samples, const uint64_t *bit_samples, uint64_t n_bit_samples, bnh_transcript_replay **out)
{
	return guarded([&]() -> int {
		if (!out || (n_samples && !samples) || (n_bit_samples && !bit_samples)) throw Error(Error::InputValidation, "null argument");
		std::unique_ptr<bnh_transcript_replay> h(new bnh_transcript_replay);
		h->samples.assign(samples, samples + n_samples);
		h->bit_samples.assign(bit_samples, bit_samples + n_bit_samples);
		h->table = bnh_transcript{h.get(), replay_write, replay_sample, replay_sample_bits};
		*out = h.release();
		return 0;
	});
}
const bnh_transcript *bnh_transcript_replay_table(bnh_transcript_replay *handle) { return handle ? &handle->table : nullptr; }
int bnh_transcript_replay_written(bnh_transcript_replay *handle, uint32_t channel, uint8_t *buf, uint64_t max, uint64_t *len_out)
{
	return guarded([&]() -> int {
		if (!handle || !len_out || channel > BNH_TR_DECOMMITMENT) throw Error(Error::InputValidation, "null argument, or an unknown channel");
		const std::vector<uint8_t> &w = handle->written[channel];
		*len_out = w.size();
		if (w.size() > max) throw Error(Error::InputValidation, "the channel holds more bytes than buf");
		if (!w.empty()) {
			if (!buf) throw Error(Error::InputValidation, "null argument");
			std::memcpy(buf, w.data(), w.size());
		}
		return 0;
	});
}
int bnh_transcript_replay_events(bnh_transcript_replay *handle, uint32_t *kinds_out, uint64_t *counts_out, uint64_t max_events, uint64_t *n_events_out)
{
	return guarded([&]() -> int {
		if (!handle || !n_events_out) throw Error(Error::InputValidation, "null argument");
		*n_events_out = handle->events.size();
		if (handle->events.size() > max_events) throw Error(Error::InputValidation, "the log holds more events than the arrays");
		if (!handle->events.empty() && (!kinds_out || !counts_out)) throw Error(Error::InputValidation, "null argument");
		for (size_t i = 0; i < handle->events.size(); i++) {
			kinds_out[i] = handle->events[i].first;
			counts_out[i] = handle->events[i].second;
		}
		return 0;
	});
}
void bnh_transcript_replay_free(bnh_transcript_replay *handle) { delete handle; }

// ---- RCCL communicator for the sharded prover (one process per GPU) ----------------------------
int bnh_rccl_open(const char *librccl_path)
{
	if (g_rccl.lib) return 0;
	void *h = dlopen(librccl_path, RTLD_NOW | RTLD_GLOBAL);
	if (!h) {
		g_err = std::string("dlopen librccl failed: ") + dlerror();
		return BN_ERR_CORE_LIB;
	}
	g_rccl.lib = h;
	g_rccl.get_unique_id = (fn_get_unique_id)dlsym(h, "ncclGetUniqueId");
	g_rccl.comm_init_rank = (fn_comm_init_rank)dlsym(h, "ncclCommInitRank");
	g_rccl.all_gather = (fn_all_gather)dlsym(h, "ncclAllGather");
	g_rccl.comm_destroy = (fn_comm_destroy)dlsym(h, "ncclCommDestroy");
	g_rccl.err = (fn_get_error_string)dlsym(h, "ncclGetErrorString");
	if (!g_rccl.get_unique_id || !g_rccl.comm_init_rank || !g_rccl.all_gather || !g_rccl.comm_destroy) {
		g_err = "librccl does not export the expected nccl* symbols";
		return BN_ERR_CORE_LIB;
	}
	return 0;
}
static int rccl_check(int rc, const char *what)
{
	if (rc == 0) return 0;
	g_err = std::string(what) + ": " + (g_rccl.err ? g_rccl.err(rc) : "rccl error");
	return BN_ERR_DEVICE;
}
int bnh_rccl_unique_id(void *out128)
{
	if (!g_rccl.lib) return (g_err = "bnh_rccl_open was not called", BN_ERR_CORE_LIB);
	return rccl_check(g_rccl.get_unique_id((rccl_unique_id *)out128), "ncclGetUniqueId");
}
int bnh_rccl_init(const void *id128, int world, int rank, void **comm_out)
{
	if (!g_rccl.lib) return (g_err = "bnh_rccl_open was not called", BN_ERR_CORE_LIB);
	rccl_unique_id id;
	std::memcpy(&id, id128, sizeof(id));
	return rccl_check(g_rccl.comm_init_rank(comm_out, world, id, rank), "ncclCommInitRank");
}
int bnh_rccl_destroy(void *comm) { return comm && g_rccl.lib ? rccl_check(g_rccl.comm_destroy(comm), "ncclCommDestroy") : 0; }

// Combine hook for the sharded prover: called once per round with the device pointer holding this
// rank's partial (y_1, y_inf) (2 field elements); must return the XOR over all ranks in `evals`.
// ---- intra-node exchange of a few scalars per round through POSIX shared memory ---------------
// The sharded prover needs, every round, the XOR of one 32-byte partial per rank.  All ranks of the
// measured configuration sit on one node, so the cheapest exchange is the host's cache-coherent
// memory: every rank publishes (payload, round) in its own cache line pair and spins on the others'
// (~1 us per round, no launch, no device round trip) -- the device side of a round is then exactly
// the single-GPU one (fused kernel + result mailbox).  The RCCL all_gather path above stays for
// ranks that do not share a node.  Two slots per rank suffice: a rank can only get one round ahead
// (it needs everybody's round r+1 value, published after they have read round r).
struct shm_slot {
	alignas(64) std::atomic<uint64_t> seq;
	uint64_t v[7];
};
struct bnh_shm {
	shm_slot *base = nullptr; // [world][2]
	int world = 0, rank = 0;
	uint64_t round = 0;
	size_t bytes = 0;
	std::string name;
	bool owner = false;
};

int bnh_shm_open(const char *name, int world, int rank, int create, void **out)
{
	if (!name || !out || world < 1 || rank < 0 || rank >= world) return (g_err = "bnh_shm_open: bad arguments", BN_ERR_INPUT_VALIDATION);
	const size_t bytes = sizeof(shm_slot) * 2 * (size_t)world;
	int fd = create ? shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600) : shm_open(name, O_RDWR, 0600);
	if (fd < 0) return (g_err = std::string("shm_open failed: ") + strerror(errno), BN_ERR_CORE_LIB);
	if (create && ftruncate(fd, (off_t)bytes) != 0) {
		close(fd);
		shm_unlink(name);
		return (g_err = std::string("ftruncate failed: ") + strerror(errno), BN_ERR_CORE_LIB);
	}
	void *p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
	close(fd);
	if (p == MAP_FAILED) return (g_err = std::string("mmap failed: ") + strerror(errno), BN_ERR_CORE_LIB);
	if (create) std::memset(p, 0, bytes); // seq = 0 everywhere; rounds start at 1
	bnh_shm *h = new bnh_shm;
	h->base = (shm_slot *)p;
	h->world = world;
	h->rank = rank;
	h->bytes = bytes;
	h->name = name;
	h->owner = create != 0;
	*out = h;
	return 0;
}

int bnh_shm_close(void *hv)
{
	bnh_shm *h = (bnh_shm *)hv;
	if (!h) return 0;
	munmap(h->base, h->bytes);
	if (h->owner) shm_unlink(h->name.c_str());
	delete h;
	return 0;
}

// every rank contributes n_words (<= 7) 64-bit words; out[world * n_words] = all of them, rank-major
int bnh_shm_allgather(void *hv, const uint64_t *in, uint32_t n_words, uint64_t *out)
{
	bnh_shm *h = (bnh_shm *)hv;
	if (!h || !in || !out || n_words > 7) return (g_err = "bnh_shm_allgather: bad arguments", BN_ERR_INPUT_VALIDATION);
	const uint64_t r = ++h->round;
	shm_slot &mine = h->base[2 * h->rank + (r & 1)];
	for (uint32_t i = 0; i < n_words; i++) mine.v[i] = in[i];
	mine.seq.store(r, std::memory_order_release);
	for (int w = 0; w < h->world; w++) {
		shm_slot &s = h->base[2 * w + (r & 1)];
		uint64_t spins = 0;
		while (s.seq.load(std::memory_order_acquire) != r) {
			++spins;
			// a rank that is late by more than ~0.1 ms is probably not running (more ranks than granted host
			// CPUs): give the core away between looks instead of burning the quota
			if (spins > (1ull << 14) && (spins & 1023) == 0) std::this_thread::yield();
			if (spins > (1ull << 22)) {
				// slow path: yield every time, and give up after ~20 s (a rank died)
				std::this_thread::yield();
				if (spins > (1ull << 22) + 20000000ull) return (g_err = "shm exchange timed out waiting for a rank", BN_ERR_DEVICE);
			}
		}
		for (uint32_t i = 0; i < n_words; i++) out[(size_t)w * n_words + i] = s.v[i];
	}
	return 0;
}


// One full prove: execute -> fold for n_vars rounds, then finish.
//   d_multilins[m]      device pointers, 2^n_vars elements each (never modified: PreFold)
//   d_scratch           device memory for the folded multilinears, >= m * 2^(n_vars-1) elements
//   comp_indices        2 per composition (IndexComposition<BivariateProduct, 2>)
//   challenges[n_vars]  stand-in for the Fiat-Shamir transcript
//   round_coeffs_out    3 per round ; final_evals_out m
//   reduce              NULL on a single GPU
// With a transport (reduce, rccl_comm, shm, or the peer bit of tail_rounds) this rank proves its shard of a world's instance
// (sharded_sumcheck.hpp): the round evaluations pass through the exchange, and the residual rounds run inside this call when asked.
int bnh_bivariate_sumcheck_prove(bn_ctx *ctx, uint32_t n_vars, uint32_t m, const void *const *d_multilins, void *d_scratch,
                                 uint64_t scratch_elems, uint32_t n_comps, const uint32_t *comp_indices, const bn_f128 *sums,
                                 const bn_f128 *batch_coeff, const bn_f128 *challenges, bn_f128 *round_coeffs_out,
                                 bn_f128 *final_evals_out, bnh_round_reduce_fn reduce, void *reduce_user, void *d_partial,
                                 void *rccl_comm, int world, void *d_gathered, void *shm, int tail_rounds)
{
	// tail_rounds: bit 0 = run the residual rounds inside this call; bit 1 = the "peer" exchange
	const bool residual_rounds = (tail_rounds & 1) != 0, peer = (tail_rounds & 2) != 0;
	const int rc = guarded([&]() -> int {
		ComputeLayer hal(ctx);
		DeviceBumpAllocator dev_alloc(FSliceMut{d_scratch, (size_t)scratch_elems});
		std::vector<B128> host_mem(m + 4);
		HostBumpAllocator host_alloc(HostSliceMut{host_mem.data(), host_mem.size()});
		std::vector<FSlice> mls;
		for (uint32_t j = 0; j < m; j++) mls.push_back(FSlice{d_multilins[j], (size_t)1 << n_vars});
		const std::vector<IndexCompositionBivariate> comps = index_compositions(m, n_comps, comp_indices);
		const std::vector<B128> sv = from_raw(sums, n_comps);
		const B128 bc = from_raw(*batch_coeff);
		if (!reduce && !rccl_comm && !shm && !peer) {
			const AbiProfSpan prof;
			BivariateSumcheckProver prover(hal, dev_alloc, host_alloc, n_vars, comps, sv, mls);
			for (uint32_t r = 0; r < n_vars; r++) {
				std::vector<B128> rc = prover.execute(bc);
				for (size_t i = 0; i < 3 && i < rc.size(); i++) round_coeffs_out[3 * r + i] = rc[i].raw();
				prover.fold(from_raw(challenges[r]));
			}
			to_raw(prover.finish(), final_evals_out);
			prof.report(n_vars);
			return 0;
		}
		ShardedBivariateSumcheckProver prover(hal, dev_alloc, host_alloc, n_vars, comps, sv, mls, [&] {
			return choose_exchange(ctx, peer, shm, rccl_comm, reduce, reduce_user, d_partial, d_gathered, world);
		});
		for (uint32_t r = 0; r < n_vars; r++) {
			to_raw(prover.execute(bc), round_coeffs_out + 3 * r);
			prover.fold(from_raw(challenges[r]));
		}
		uint32_t log_world = 0;
		while ((1 << (log_world + 1)) <= world) log_world++;
		if (residual_rounds && log_world > 0) {
			bn_f128 *out = round_coeffs_out + 3 * n_vars;
			for (const auto &rc : prover.run_residual(bc, from_raw(challenges + n_vars, log_world))) out = to_raw(rc, out);
		}
		to_raw(prover.finish(), final_evals_out);
		return 0;
	});
	// every route has always left the host-tail permission cleared on every exit; the peer exchange clears its own
	if (!peer) (void)bn_host_tail_allow_peer(ctx, 0);
	return rc;
}

static thread_local int g_mlecheck_mode = -1;
int bnh_mlecheck_last_mode(void) { return g_mlecheck_mode; }

// ---- MLE-check prover behind a handle: SumcheckProver::{execute, fold, finish} (prove/batch_sumcheck.rs:38-70) one
// call each, so that a host whose challenges come out of a transcript can drive it round by round.
//   d_eq_ind             2^(n_vars-1) elements: tensor expansion of eq_ind_challenges[0 .. n_vars-1)
struct bnh_mlecheck {
	ComputeLayer hal;
	DeviceBumpAllocator dev_alloc;
	std::vector<B128> host_mem;
	HostBumpAllocator host_alloc;
	std::unique_ptr<WeightedMLEcheckProver> weighted;
	std::unique_ptr<BivariateMLEcheckProver> literal;
	uint32_t m;
	bnh_mlecheck(bn_ctx *ctx, void *d_scratch, uint64_t scratch_elems, uint32_t m_)
	    : hal(ctx), dev_alloc(FSliceMut{d_scratch, (size_t)scratch_elems}), host_mem(m_ + 4),
	      host_alloc(HostSliceMut{host_mem.data(), host_mem.size()}), m(m_)
	{
	}
};

int bnh_mlecheck_new(bn_ctx *ctx, uint32_t n_vars, uint32_t m, const void *const *d_multilins, const void *d_eq_ind,
                     const bn_f128 *eq_ind_challenges, void *d_scratch, uint64_t scratch_elems, uint32_t n_comps,
                     const uint32_t *comp_indices, const bn_f128 *sums, bnh_mlecheck **out)
{
	return guarded([&]() -> int {
		if (!out) throw Error(Error::InputValidation, "null argument");
		std::unique_ptr<bnh_mlecheck> h(new bnh_mlecheck(ctx, d_scratch, scratch_elems, m));
		std::vector<FSlice> mls;
		for (uint32_t j = 0; j < m; j++) mls.push_back(FSlice{d_multilins[j], (size_t)1 << n_vars});
		const std::vector<IndexCompositionBivariate> comps = index_compositions(m, n_comps, comp_indices);
		const std::vector<B128> sv = from_raw(sums, n_comps), eqc = from_raw(eq_ind_challenges, n_vars);
		const FSlice eq_table{d_eq_ind, (size_t)1 << (n_vars ? n_vars - 1 : 0)};
		// The weighted prover (sumcheck.hpp) when it applies: a proper 2-colouring of the compositions, invertible
		// indicator coordinates, enough scratch, and a table that IS the tensor expansion of the coordinates (the
		// constructor's contract: "an existing tensor expansion for eq_ind_challenges", bivariate_mlecheck.rs:69-71 --
		// spot-checked here on n_vars + 17 entries because the weighted prover derives the later tables from the
		// coordinates instead of folding the given one).
		std::vector<bool> weighted;
		const char *mode = getenv("BN_MLECHECK");
		if (!(mode && std::string(mode) == "eager") && n_vars >= 2 && n_comps > 0) {
			weighted = WeightedMLEcheckProver::colouring(m, comps);
			bool any = false;
			for (bool w : weighted) any = any || w;
			if (!any || !WeightedMLEcheckProver::coordinates_invertible(eqc, n_vars) ||
			    WeightedMLEcheckProver::required_device_memory(weighted, n_vars) > scratch_elems)
				weighted.clear();
		}
		if (!weighted.empty()) {
			std::vector<uint64_t> offs{0, eq_table.len() - 1};
			for (uint32_t i = 0; i + 1 < n_vars; i++) offs.push_back((uint64_t)1 << i);
			uint64_t lcg = eqc[0].raw().lo ^ 0x9E3779B97F4A7C15ull; // a few more, spread over the table
			for (int k = 0; k < 16; k++) {
				lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
				offs.push_back((lcg >> 20) & (eq_table.len() - 1));
			}
			std::vector<B128> got(offs.size());
			check(bn_gather_d2h(ctx, d_eq_ind, offs.data(), offs.size(), 1, reinterpret_cast<bn_f128 *>(got.data())));
			for (size_t k = 0; k < offs.size() && !weighted.empty(); k++) {
				B128 want = B128::ONE();
				for (uint32_t i = 0; i + 1 < n_vars; i++) want = want * (((offs[k] >> i) & 1) ? eqc[i] : B128::ONE() - eqc[i]);
				if (!(got[k] == want)) weighted.clear();
			}
		}
		g_mlecheck_mode = weighted.empty() ? 0 : 1;
		if (!weighted.empty())
			h->weighted.reset(new WeightedMLEcheckProver(h->hal, h->dev_alloc, h->host_alloc, n_vars, comps, sv, mls, eq_table, eqc, weighted));
		else
			h->literal.reset(new BivariateMLEcheckProver(h->hal, h->dev_alloc, h->host_alloc, n_vars, comps, sv, mls, eq_table, eqc));
		*out = h.release();
		return 0;
	});
}

// coeffs_out[4]: the round polynomial (degree 3)
int bnh_mlecheck_execute(bnh_mlecheck *h, const bn_f128 *batch_coeff, bn_f128 *coeffs_out)
{
	return guarded([&]() -> int {
		if (!h || !batch_coeff || !coeffs_out) throw Error(Error::InputValidation, "null argument");
		const B128 bc = from_raw(*batch_coeff);
		const std::vector<B128> rc = h->weighted ? h->weighted->execute(bc) : h->literal->execute(bc);
		for (size_t i = 0; i < 4; i++) coeffs_out[i] = i < rc.size() ? rc[i].raw() : bn_f128{0, 0};
		return 0;
	});
}

int bnh_mlecheck_fold(bnh_mlecheck *h, const bn_f128 *challenge)
{
	return guarded([&]() -> int {
		if (!h || !challenge) throw Error(Error::InputValidation, "null argument");
		const B128 z = from_raw(*challenge);
		if (h->weighted)
			h->weighted->fold(z);
		else
			h->literal->fold(z);
		return 0;
	});
}

// final_evals_out[m + 1]: the multilinears' evaluations, then eq_ind_prefix_eval.  The handle stays valid (free it).
int bnh_mlecheck_finish(bnh_mlecheck *h, bn_f128 *final_evals_out)
{
	return guarded([&]() -> int {
		if (!h || !final_evals_out) throw Error(Error::InputValidation, "null argument");
		to_raw(h->weighted ? h->weighted->finish() : h->literal->finish(), final_evals_out);
		return 0;
	});
}

void bnh_mlecheck_free(bnh_mlecheck *h) { delete h; }

// One complete BivariateMLEcheckProver run (v3/bivariate_mlecheck.rs) behind a C call.
//   round_coeffs_out     [4 * n_vars] (degree-3 round polynomials)
//   final_evals_out      [m + 1]      (the last one is eq_ind_prefix_eval)
int bnh_bivariate_mlecheck_prove(bn_ctx *ctx, uint32_t n_vars, uint32_t m, const void *const *d_multilins, const void *d_eq_ind,
                                 const bn_f128 *eq_ind_challenges, void *d_scratch, uint64_t scratch_elems, uint32_t n_comps,
                                 const uint32_t *comp_indices, const bn_f128 *sums, const bn_f128 *batch_coeff,
                                 const bn_f128 *challenges, bn_f128 *round_coeffs_out, bn_f128 *final_evals_out)
{
	bnh_mlecheck *h = nullptr;
	int rc = bnh_mlecheck_new(ctx, n_vars, m, d_multilins, d_eq_ind, eq_ind_challenges, d_scratch, scratch_elems, n_comps, comp_indices, sums, &h);
	for (uint32_t r = 0; rc == 0 && r < n_vars; r++) {
		rc = bnh_mlecheck_execute(h, batch_coeff, round_coeffs_out + 4 * r);
		if (rc == 0) rc = bnh_mlecheck_fold(h, &challenges[r]);
	}
	if (rc == 0) rc = bnh_mlecheck_finish(h, final_evals_out);
	bnh_mlecheck_free(h);
	return rc;
}

// FRI commit phase + all fold rounds + finalize through the C++ mirror (fri.hpp), everything on the device.
//   d_message        2^(log_dim + log_batch_size) elements (the interleaved message)
//   d_scratch        device memory for the codeword, the folded codewords and the Merkle trees:
//                    2 * 2^(log_dim + log_batch_size + log_inv_rate) elements are always enough
//   challenges       [log_dim + log_batch_size]
//   roots_out        [(n_arities + 1) * 32 bytes]: the commitment, then one root per committed oracle
//   terminate_out    [2^(log_inv_rate + n_final_challenges)] elements or NULL
//   phase_ms_out     [2] wall-clock milliseconds of the commit phase and of the fold phase, or NULL
int bnh_fri_commit_fold(bn_ctx *ctx, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities,
                        uint32_t n_arities, uint32_t n_test_queries, const void *d_message, void *d_scratch, uint64_t scratch_elems,
                        const bn_f128 *challenges, uint8_t *roots_out, bn_f128 *terminate_out, double *phase_ms_out)
{
	return guarded([&]() -> int {
		ComputeLayer hal(ctx);
		DeviceBumpAllocator dev_alloc(FSliceMut{d_scratch, (size_t)scratch_elems});
		FRIParams p(log_dim, log_inv_rate, log_batch_size, std::vector<size_t>(fold_arities, fold_arities + n_arities), n_test_queries);
		AdditiveNTT ntt(hal, 5, p.rs_log_len());
		BinaryMerkleTreeProver merkle(hal);
		hal.sync();
		const auto t0 = std::chrono::steady_clock::now();
		CommitOutput out = commit_interleaved(hal, dev_alloc, p, ntt, merkle, FSlice{d_message, (size_t)1 << (log_dim + log_batch_size)});
		hal.sync();
		const auto t1 = std::chrono::steady_clock::now();
		std::memcpy(roots_out, out.commitment.data(), 32);
		FRIFolder folder(hal, p, ntt, merkle, ComputeMemory::as_const(out.codeword), out.committed);
		size_t n_roots = 1;
		for (size_t r = 0; r < folder.n_rounds(); r++) {
			auto [has_root, root] = folder.execute_fold_round(dev_alloc, from_raw(challenges[r]));
			if (has_root) std::memcpy(roots_out + 32 * n_roots++, root.data(), 32);
		}
		auto fin = folder.finalize();
		hal.sync();
		const auto t2 = std::chrono::steady_clock::now();
		if (terminate_out) to_raw(fin.first, terminate_out);
		if (phase_ms_out) {
			phase_ms_out[0] = elapsed_ms(t0, t1);
			phase_ms_out[1] = elapsed_ms(t1, t2);
		}
		return 0;
	});
}

// bnh_fri_commit_fold with FRIFolder::finish_proof in place of finalize: the whole decommitment (terminate codeword, layers, every
// query's openings) from one launch.
//   query_indices    [n_test_queries], each below 2^index_bits
//   advice_out       [max_advice_elems]; *n_advice_elems_out: the elements written
//   phase_ms_out     [3] commit, fold, query phase, or NULL
static int fri_prove_body(bn_ctx *ctx, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities,
                          uint32_t n_test_queries, const void *d_message, void *d_scratch, uint64_t scratch_elems, const bn_f128 *challenges, uint8_t *roots_out,
                          const uint64_t *query_indices, bn_f128 *advice_out, uint64_t max_advice_elems, uint64_t *n_advice_elems_out, double *phase_ms_out, bool is_live,
                          const bnh_transcript *transcript)
{
	return guarded([&]() -> int {
		EntryTranscript et(is_live, transcript, n_test_queries != 0);
		if (!ctx || !d_message || !d_scratch || (!is_live && !challenges) || !roots_out || !advice_out || !n_advice_elems_out || (n_arities && !fold_arities) ||
		    (n_test_queries && !is_live && !query_indices))
			throw Error(Error::InputValidation, "null argument");
		if ((uint64_t)log_dim + log_batch_size + log_inv_rate >= 48) throw Error(Error::InputValidation, "FRI parameters out of range");
		ComputeLayer hal(ctx);
		DeviceBumpAllocator dev_alloc(FSliceMut{d_scratch, (size_t)scratch_elems});
		FRIParams p(log_dim, log_inv_rate, log_batch_size, std::vector<size_t>(fold_arities, fold_arities + n_arities), n_test_queries);
		// (before anything is launched or written: a caller's transcript must not absorb a proof whose advice it cannot take)
		if (p.advice_elems() > max_advice_elems) throw Error(Error::InputValidation, "the advice has more elements than advice_out holds");
		AdditiveNTT ntt(hal, 5, p.rs_log_len());
		BinaryMerkleTreeProver merkle(hal);
		hal.sync();
		const auto t0 = std::chrono::steady_clock::now();
		CommitOutput out = commit_interleaved(hal, dev_alloc, p, ntt, merkle, FSlice{d_message, (size_t)1 << (log_dim + log_batch_size)});
		hal.sync();
		const auto t1 = std::chrono::steady_clock::now();
		std::memcpy(roots_out, out.commitment.data(), 32);
		FRIFolder folder(hal, p, ntt, merkle, ComputeMemory::as_const(out.codeword), out.committed);
		// schedule: the commitment; per fold round ONE sample, then the round's commitment when the folder commits in it
		// (fri/prove.rs:307-432 as piop/prove.rs:343-358 drives it); then FRIFolder::finish_proof (fri/prove.rs:483-507): the terminate
		// codeword on the decommitment channel, sample_bits(index_bits) n_test_queries times, the layers and the openings on the
		// decommitment channel
		TranscriptSource &tr = et.source({from_raw(challenges, folder.n_rounds())}, query_indices, n_test_queries);
		tr.write_digest(out.commitment);
		size_t n_roots = 1;
		for (size_t r = 0; r < folder.n_rounds(); r++) {
			auto [has_root, root] = folder.execute_fold_round(dev_alloc, tr.sample(0, r));
			if (has_root) {
				std::memcpy(roots_out + 32 * n_roots++, root.data(), 32);
				tr.write_digest(root);
			}
		}
		hal.sync();
		const auto t2 = std::chrono::steady_clock::now();
		if (tr.observes_writes()) tr.write_scalars(folder.finalize().first, BNH_TR_DECOMMITMENT);
		const std::vector<uint64_t> drawn = tr.sample_bits_vec((uint32_t)p.index_bits(), 0, n_test_queries);
		const FriAdvice advice = folder.finish_proof(std::vector<size_t>(drawn.begin(), drawn.end()));
		const auto t3 = std::chrono::steady_clock::now(); // (finish_proof returns after its synchronisation)
		tr.write_scalars(advice.block.data() + advice.terminate_elems, advice.block.size() - advice.terminate_elems, BNH_TR_DECOMMITMENT);
		if (advice.block.size() > max_advice_elems) throw Error(Error::InputValidation, "the advice has more elements than advice_out holds");
		to_raw(advice.block, advice_out);
		*n_advice_elems_out = advice.block.size();
		if (phase_ms_out) {
			phase_ms_out[0] = elapsed_ms(t0, t1);
			phase_ms_out[1] = elapsed_ms(t1, t2);
			phase_ms_out[2] = elapsed_ms(t2, t3);
		}
		return 0;
	});
}

int bnh_fri_prove(bn_ctx *ctx, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities,
                  uint32_t n_test_queries, const void *d_message, void *d_scratch, uint64_t scratch_elems, const bn_f128 *challenges, uint8_t *roots_out,
                  const uint64_t *query_indices, bn_f128 *advice_out, uint64_t max_advice_elems, uint64_t *n_advice_elems_out, double *phase_ms_out)
{
	return fri_prove_body(ctx, log_dim, log_inv_rate, log_batch_size, fold_arities, n_arities, n_test_queries, d_message, d_scratch, scratch_elems, challenges, roots_out,
	                      query_indices, advice_out, max_advice_elems, n_advice_elems_out, phase_ms_out, false, nullptr);
}

int bnh_fri_prove_live(bn_ctx *ctx, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities,
                       uint32_t n_test_queries, const void *d_message, void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript, uint8_t *roots_out,
                       bn_f128 *advice_out, uint64_t max_advice_elems, uint64_t *n_advice_elems_out, double *phase_ms_out)
{
	return fri_prove_body(ctx, log_dim, log_inv_rate, log_batch_size, fold_arities, n_arities, n_test_queries, d_message, d_scratch, scratch_elems, nullptr, roots_out, nullptr,
	                      advice_out, max_advice_elems, n_advice_elems_out, phase_ms_out, true, transcript);
}

// diagnostic: the query phase timed two ways on the same resident codewords and trees (tools/bench_fri_query.py).  One commit and
// fold, then warmup + runs times, alternating: FRIFolder::finish_proof (one launch), and the per-opening route -- finalize's copy of
// the terminate codeword and one FRIQueryProver::prove_query per index (a copy_d2h and a bn_gather_d2h per opening; the layers are not
// part of it).  Wall clock between two synchronisations each.  *equal_out: the per-opening route (with the layers, fetched outside the
// timed window) returned the bytes of the advice.
int bnh_fri_query_phase_bench(bn_ctx *ctx, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities,
                              uint32_t n_test_queries, const void *d_message, void *d_scratch, uint64_t scratch_elems, const bn_f128 *challenges,
                              const uint64_t *query_indices, uint32_t warmup, uint32_t runs, double *new_ms_out, double *old_ms_out, uint64_t *advice_elems_out,
                              uint32_t *equal_out)
{
	return guarded([&]() -> int {
		if (!ctx || !d_message || !d_scratch || !challenges || !new_ms_out || !old_ms_out || !advice_elems_out || !equal_out || (n_arities && !fold_arities) ||
		    (n_test_queries && !query_indices))
			throw Error(Error::InputValidation, "null argument");
		if ((uint64_t)log_dim + log_batch_size + log_inv_rate >= 48) throw Error(Error::InputValidation, "FRI parameters out of range");
		ComputeLayer hal(ctx);
		DeviceBumpAllocator dev_alloc(FSliceMut{d_scratch, (size_t)scratch_elems});
		FRIParams p(log_dim, log_inv_rate, log_batch_size, std::vector<size_t>(fold_arities, fold_arities + n_arities), n_test_queries);
		AdditiveNTT ntt(hal, 5, p.rs_log_len());
		BinaryMerkleTreeProver merkle(hal);
		CommitOutput out = commit_interleaved(hal, dev_alloc, p, ntt, merkle, FSlice{d_message, (size_t)1 << (log_dim + log_batch_size)});
		FRIFolder folder(hal, p, ntt, merkle, ComputeMemory::as_const(out.codeword), out.committed);
		for (size_t r = 0; r < folder.n_rounds(); r++) folder.execute_fold_round(dev_alloc, from_raw(challenges[r]));
		const std::vector<size_t> indices(query_indices, query_indices + n_test_queries);
		FriAdvice advice;
		std::vector<B128> terminate;
		std::vector<std::vector<CosetOpening>> openings;
		for (uint32_t it = 0; it < warmup + runs; it++) {
			hal.sync();
			const auto t0 = std::chrono::steady_clock::now();
			advice = folder.finish_proof(indices);
			hal.sync();
			const auto t1 = std::chrono::steady_clock::now();
			openings.clear();
			auto fin = folder.finalize();
			for (size_t index : indices) openings.push_back(fin.second.prove_query(index));
			hal.sync();
			const auto t2 = std::chrono::steady_clock::now();
			terminate = std::move(fin.first);
			if (it >= warmup) {
				new_ms_out[it - warmup] = elapsed_ms(t0, t1);
				old_ms_out[it - warmup] = elapsed_ms(t1, t2);
			}
		}
		// the same bytes?
		std::vector<B128> flat = terminate;
		auto fin = folder.finalize();
		for (const auto &layer : fin.second.vcs_optimal_layers())
			for (const Digest &d : layer) {
				B128 two[2];
				std::memcpy(two, d.data(), 32);
				flat.insert(flat.end(), two, two + 2);
			}
		for (const auto &query : openings)
			for (const CosetOpening &o : query) {
				flat.insert(flat.end(), o.values.begin(), o.values.end());
				for (const Digest &d : o.branch) {
					B128 two[2];
					std::memcpy(two, d.data(), 32);
					flat.insert(flat.end(), two, two + 2);
				}
			}
		*advice_elems_out = advice.block.size();
		*equal_out = runs + warmup > 0 && flat.size() == advice.block.size() && std::memcmp(flat.data(), advice.block.data(), flat.size() * sizeof(B128)) == 0;
		return 0;
	});
}

// piop::prove (crates/core/src/piop/prove.rs:148-395) through the C++ mirror piop.hpp: commit_interleaved of the merged message
// (bnh_piop_prove) or the codeword and tree of an earlier bnh_piop_commit (bnh_piop_prove_committed), then
// one BivariateSumcheckProver per number of variables, the front-loaded batch prover interleaved with the FRI folder.
// The transcript comes back as a list of items in writing order: items_out[2 i] = kind (0 round proof, 1 final evaluations of a
// finished prover, 2 FRI round commitment, 3 FRI terminate codeword), items_out[2 i + 1] = number of scalars (kinds 0, 1, 3:
// consumed from scalars_out in order) or 1 digest (kind 2: consumed from digests_out in order).
namespace {
// What the two entry points of piop::prove share: everything but where the codeword and its tree come from.  `commit` runs between the
// first two time stamps and returns them: bnh_piop_prove commits the message there, bnh_piop_prove_committed wraps the caller's buffers.
// phase_ms[2]: that step, the prove.
using PiopCommitStep = std::function<std::pair<FSlice, BinaryMerkleTree>(ComputeLayer &, DeviceBumpAllocator &, const FRIParams &, const AdditiveNTT &, BinaryMerkleTreeProver &)>;
// The FRI query phase of an entry point that has one (bnh_piop_prove_committed_open): the indices in, the advice out
struct PiopQueryPhase {
	const uint64_t *query_indices;
	bn_f128 *advice_out;
	uint64_t max_advice_elems;
	uint64_t *n_advice_elems_out;
	bool is_live = false; // the _live form: no sample array is read, everything is drawn from `transcript`
	const bnh_transcript *transcript = nullptr;
};
static int piop_prove_body(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                    const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims, const bn_f128 *claim_sums,
                    uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities, uint32_t n_test_queries,
                    const PiopCommitStep &commit, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, uint32_t n_batch_coeffs,
                    const bn_f128 *challenges, uint32_t n_challenges, uint32_t *items_out, uint32_t max_items, uint32_t *n_items_out, bn_f128 *scalars_out,
                    uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out, uint32_t max_digests, uint32_t *n_digests_out, double *phase_ms,
                    const PiopQueryPhase *query = nullptr)
{
	{
		const bool is_live = query && query->is_live;
		EntryTranscript et(is_live, query ? query->transcript : nullptr, n_test_queries != 0);
		if (!ctx || !items_out || !n_items_out || !scalars_out || !n_scalars_out || !digests_out || !n_digests_out)
			throw Error(Error::InputValidation, "null argument");
		if ((n_committed && (!committed_n_vars || !d_committed)) || (n_transparent && (!transparent_n_vars || !d_transparent)) || (n_claims && (!claims || !claim_sums)) ||
		    (n_arities && !fold_arities) || (n_batch_coeffs && !batch_coeffs) || (n_challenges && !challenges))
			throw Error(Error::InputValidation, "null argument");
		if (query && (!query->advice_out || !query->n_advice_elems_out || (n_test_queries && !is_live && !query->query_indices))) throw Error(Error::InputValidation, "null argument");
		for (uint32_t i = 0; i < n_committed; i++)
			if (committed_n_vars[i] >= 48 || !d_committed[i]) throw Error(Error::InputValidation, "committed multilinear: null, or its number of variables out of range (< 48)");
		for (uint32_t i = 0; i < n_transparent; i++)
			if (transparent_n_vars[i] >= 48 || !d_transparent[i]) throw Error(Error::InputValidation, "transparent multilinear: null, or its number of variables out of range (< 48)");
		if (log_dim + log_batch_size + log_inv_rate >= 48) throw Error(Error::InputValidation, "FRI parameters out of range");
		ComputeLayer hal(ctx);
		DeviceBumpAllocator dev_alloc(FSliceMut{d_scratch, (size_t)scratch_elems});
		std::vector<size_t> n_varss;
		std::vector<FSlice> committed, transparents;
		size_t host_elems = 8;
		for (uint32_t i = 0; i < n_committed; i++) {
			if (i && committed_n_vars[i] < committed_n_vars[i - 1]) throw PiopError("CommittedsNotSorted");
			n_varss.push_back(committed_n_vars[i]);
			committed.push_back(FSlice{d_committed[i], (size_t)1 << committed_n_vars[i]});
			host_elems++;
		}
		for (uint32_t i = 0; i < n_transparent; i++) {
			transparents.push_back(FSlice{d_transparent[i], (size_t)1 << transparent_n_vars[i]});
			host_elems++;
		}
		std::vector<B128> host_mem(host_elems);
		HostBumpAllocator host_alloc(HostSliceMut{host_mem.data(), host_mem.size()});
		const CommitMeta commit_meta = CommitMeta::with_vars(n_varss);
		if (commit_meta.total_vars() != (size_t)log_dim + log_batch_size) throw PiopError("FRI message length does not match the commit metadata's total_vars");
		std::vector<PIOPSumcheckClaim> cl;
		for (uint32_t i = 0; i < n_claims; i++)
			cl.push_back(PIOPSumcheckClaim{claims[3 * i], claims[3 * i + 1], claims[3 * i + 2], from_raw(claim_sums[i])});
		const std::vector<B128> bcs = from_raw(batch_coeffs, n_batch_coeffs), chs = from_raw(challenges, n_challenges);
		FRIParams p(log_dim, log_inv_rate, log_batch_size, std::vector<size_t>(fold_arities, fold_arities + n_arities), n_test_queries);
		// (before anything is launched or written: a caller's transcript must not absorb a proof whose advice it cannot take)
		if (query && p.advice_elems() > query->max_advice_elems) throw Error(Error::InputValidation, "the advice has more elements than advice_out holds");
		AdditiveNTT ntt(hal, 5, p.rs_log_len());
		BinaryMerkleTreeProver merkle(hal);
		hal.sync();
		const auto t0 = std::chrono::steady_clock::now();
		const std::pair<FSlice, BinaryMerkleTree> co = commit(hal, dev_alloc, p, ntt, merkle);
		hal.sync();
		const auto t1 = std::chrono::steady_clock::now();
		if (AbiProf::on()) AbiProf::get() = AbiProf{};
		std::vector<size_t> query_indices;
		if (query && !is_live) query_indices.assign(query->query_indices, query->query_indices + n_test_queries);
		PiopProveOutput out = is_live ? piop_prove_live(hal, dev_alloc, host_alloc, p, ntt, merkle, commit_meta, co.second, co.first, committed, transparents, cl,
		                                                et.source({}), true)
		                              : piop_prove_impl(hal, dev_alloc, host_alloc, p, ntt, merkle, commit_meta, co.second, co.first, committed, transparents, cl, bcs, chs,
		                                                query ? &query_indices : nullptr);
		hal.sync();
		const auto t2 = std::chrono::steady_clock::now();
		if (AbiProf::on()) {
			const AbiProf &pr = AbiProf::get();
			fprintf(stderr, "[bnh prof] piop prove %.1f us: send_round_proof %.1f, receive_challenge %.1f, fri round %.1f | inside the ABI: kernel_launch %.1f (%llu calls), extrapolate_line %.1f (%llu), copies %.1f (%llu)\n",
			        1e3 * elapsed_ms(t1, t2), out.phase_ns[0] / 1e3, out.phase_ns[1] / 1e3, out.phase_ns[2] / 1e3, pr.ns[0] / 1e3,
			        (unsigned long long)pr.calls[0], pr.ns[1] / 1e3, (unsigned long long)pr.calls[1], pr.ns[2] / 1e3, (unsigned long long)pr.calls[2]);
		}
		uint32_t ni = 0, nd = 0;
		uint64_t ns = 0;
		for (const auto &it : out.transcript.items) {
			if (ni >= max_items) throw Error(Error::InputValidation, "transcript has more items than items_out holds");
			items_out[2 * ni] = (uint32_t)it.kind;
			if (it.kind == PiopTranscript::Item::FriCommitment) {
				if (nd >= max_digests) throw Error(Error::InputValidation, "transcript has more digests than digests_out holds");
				std::memcpy(digests_out + 32 * (size_t)nd++, it.digest.data(), 32);
				items_out[2 * ni + 1] = 1;
			} else {
				if (ns + it.scalars.size() > max_scalars) throw Error(Error::InputValidation, "transcript has more scalars than scalars_out holds");
				ns = to_raw(it.scalars, scalars_out + ns) - scalars_out;
				items_out[2 * ni + 1] = (uint32_t)it.scalars.size();
			}
			ni++;
		}
		if (query) {
			if (out.advice.size() > query->max_advice_elems) throw Error(Error::InputValidation, "the advice has more elements than advice_out holds");
			to_raw(out.advice, query->advice_out);
			*query->n_advice_elems_out = out.advice.size();
		}
		*n_items_out = ni;
		*n_scalars_out = ns;
		*n_digests_out = nd;
		phase_ms[0] = elapsed_ms(t0, t1);
		phase_ms[1] = elapsed_ms(t1, t2);
		return 0;
	}
}

// leaves of the tree over a codeword of these parameters: cosets of 2^arity_0, or of the whole message when nothing is folded
static size_t piop_commit_log_leaves(uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities)
{
	const size_t log_elems = (size_t)log_dim + log_batch_size;
	return log_elems + log_inv_rate - (n_arities ? fold_arities[0] : log_elems);
}

// the checks of merge_multilins' callers on the sizes alone: ascending, each below 48
static void piop_check_committed_n_vars(uint32_t n, const uint32_t *n_vars)
{
	if (n && !n_vars) throw Error(Error::InputValidation, "null argument");
	for (uint32_t i = 0; i < n; i++) {
		if (n_vars[i] >= 48) throw Error(Error::InputValidation, "committed multilinear: its number of variables out of range (< 48)");
		if (i && n_vars[i] < n_vars[i - 1]) throw PiopError("CommittedsNotSorted");
	}
}
} // namespace

int bnh_piop_prove(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                   const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims, const bn_f128 *claim_sums,
                   uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities, uint32_t n_test_queries,
                   const void *d_message, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, uint32_t n_batch_coeffs,
                   const bn_f128 *challenges, uint32_t n_challenges, uint8_t *commitment_out, uint32_t *items_out, uint32_t max_items, uint32_t *n_items_out,
                   bn_f128 *scalars_out, uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out, uint32_t max_digests, uint32_t *n_digests_out,
                   double *phase_ms_out)
{
	return guarded([&]() -> int {
		if (!commitment_out || !d_message) throw Error(Error::InputValidation, "null argument");
		const PiopCommitStep commit = [&](ComputeLayer &hal, DeviceBumpAllocator &dev_alloc, const FRIParams &p, const AdditiveNTT &ntt, BinaryMerkleTreeProver &merkle) {
			CommitOutput co = commit_interleaved(hal, dev_alloc, p, ntt, merkle, FSlice{d_message, (size_t)1 << (log_dim + log_batch_size)});
			std::memcpy(commitment_out, co.commitment.data(), 32);
			return std::make_pair(ComputeMemory::as_const(co.codeword), co.committed);
		};
		double ms[2] = {0, 0};
		const int rc = piop_prove_body(ctx, n_committed, committed_n_vars, d_committed, n_transparent, transparent_n_vars, d_transparent, n_claims, claims, claim_sums,
		                               log_dim, log_inv_rate, log_batch_size, fold_arities, n_arities, n_test_queries, commit, d_scratch, scratch_elems, batch_coeffs,
		                               n_batch_coeffs, challenges, n_challenges, items_out, max_items, n_items_out, scalars_out, max_scalars, n_scalars_out, digests_out,
		                               max_digests, n_digests_out, ms);
		if (phase_ms_out) phase_ms_out[0] = ms[0], phase_ms_out[1] = ms[1];
		return rc;
	});
}

// piop::prove from a commitment made earlier (bnh_piop_commit): the arguments of bnh_piop_prove, with the codeword and the flattened
// tree that call left in the caller's buffers in place of the message.  Only reads them; never commits.  phase_ms_out[1]: the prove.
static int piop_prove_committed_body(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                             const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims,
                             const bn_f128 *claim_sums, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities,
                             uint32_t n_arities, uint32_t n_test_queries, const void *d_codeword, const void *d_tree, void *d_scratch, uint64_t scratch_elems,
                             const bn_f128 *batch_coeffs, uint32_t n_batch_coeffs, const bn_f128 *challenges, uint32_t n_challenges, uint32_t *items_out,
                             uint32_t max_items, uint32_t *n_items_out, bn_f128 *scalars_out, uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out,
                             uint32_t max_digests, uint32_t *n_digests_out, double *phase_ms_out, const PiopQueryPhase *query)
{
	return guarded([&]() -> int {
		if (query && query->is_live) LiveTranscript(query->transcript, n_test_queries != 0); // (a null table is rejected before anything else is read)
		if (!d_codeword || !d_tree || (n_arities && !fold_arities)) throw Error(Error::InputValidation, "null argument");
		const PiopCommitStep commit = [&](ComputeLayer &hal, DeviceBumpAllocator &, const FRIParams &p, const AdditiveNTT &, BinaryMerkleTreeProver &) {
			BinaryMerkleTree tree;
			tree.log_len = piop_commit_log_leaves(log_dim, log_inv_rate, log_batch_size, fold_arities, n_arities);
			tree.nodes = FSlice{d_tree, BinaryMerkleTreeProver::required_device_memory((size_t)1 << tree.log_len)};
			tree.hal = &hal;
			return std::make_pair(FSlice{d_codeword, (size_t)1 << p.log_len()}, tree);
		};
		double ms[2] = {0, 0};
		const int rc = piop_prove_body(ctx, n_committed, committed_n_vars, d_committed, n_transparent, transparent_n_vars, d_transparent, n_claims, claims, claim_sums,
		                               log_dim, log_inv_rate, log_batch_size, fold_arities, n_arities, n_test_queries, commit, d_scratch, scratch_elems, batch_coeffs,
		                               n_batch_coeffs, challenges, n_challenges, items_out, max_items, n_items_out, scalars_out, max_scalars, n_scalars_out, digests_out,
		                               max_digests, n_digests_out, ms, query);
		if (phase_ms_out) phase_ms_out[0] = ms[1];
		return rc;
	});
}

int bnh_piop_prove_committed(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                             const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims,
                             const bn_f128 *claim_sums, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities,
                             uint32_t n_arities, uint32_t n_test_queries, const void *d_codeword, const void *d_tree, void *d_scratch, uint64_t scratch_elems,
                             const bn_f128 *batch_coeffs, uint32_t n_batch_coeffs, const bn_f128 *challenges, uint32_t n_challenges, uint32_t *items_out,
                             uint32_t max_items, uint32_t *n_items_out, bn_f128 *scalars_out, uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out,
                             uint32_t max_digests, uint32_t *n_digests_out, double *phase_ms_out)
{
	return piop_prove_committed_body(ctx, n_committed, committed_n_vars, d_committed, n_transparent, transparent_n_vars, d_transparent, n_claims, claims, claim_sums, log_dim,
	                                 log_inv_rate, log_batch_size, fold_arities, n_arities, n_test_queries, d_codeword, d_tree, d_scratch, scratch_elems, batch_coeffs,
	                                 n_batch_coeffs, challenges, n_challenges, items_out, max_items, n_items_out, scalars_out, max_scalars, n_scalars_out, digests_out,
	                                 max_digests, n_digests_out, phase_ms_out, nullptr);
}

// bnh_piop_prove_committed with the FRI query phase: the same item list, the decommitment of finish_proof in advice_out
int bnh_piop_prove_committed_open(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                             const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims,
                             const bn_f128 *claim_sums, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities,
                             uint32_t n_arities, uint32_t n_test_queries, const void *d_codeword, const void *d_tree, void *d_scratch, uint64_t scratch_elems,
                             const bn_f128 *batch_coeffs, uint32_t n_batch_coeffs, const bn_f128 *challenges, uint32_t n_challenges, uint32_t *items_out,
                             uint32_t max_items, uint32_t *n_items_out, bn_f128 *scalars_out, uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out,
                             uint32_t max_digests, uint32_t *n_digests_out, double *phase_ms_out, const uint64_t *query_indices, bn_f128 *advice_out,
                             uint64_t max_advice_elems, uint64_t *n_advice_elems_out)
{
	const PiopQueryPhase query{query_indices, advice_out, max_advice_elems, n_advice_elems_out};
	return piop_prove_committed_body(ctx, n_committed, committed_n_vars, d_committed, n_transparent, transparent_n_vars, d_transparent, n_claims, claims, claim_sums, log_dim,
	                                 log_inv_rate, log_batch_size, fold_arities, n_arities, n_test_queries, d_codeword, d_tree, d_scratch, scratch_elems, batch_coeffs,
	                                 n_batch_coeffs, challenges, n_challenges, items_out, max_items, n_items_out, scalars_out, max_scalars, n_scalars_out, digests_out,
	                                 max_digests, n_digests_out, phase_ms_out, &query);
}

// bnh_piop_prove_committed_open against the caller's transcript
int bnh_piop_prove_committed_open_live(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t n_transparent,
                                       const uint32_t *transparent_n_vars, const void *const *d_transparent, uint32_t n_claims, const uint32_t *claims,
                                       const bn_f128 *claim_sums, uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities,
                                       uint32_t n_arities, uint32_t n_test_queries, const void *d_codeword, const void *d_tree, void *d_scratch, uint64_t scratch_elems,
                                       const bnh_transcript *transcript, uint32_t *items_out, uint32_t max_items, uint32_t *n_items_out, bn_f128 *scalars_out,
                                       uint64_t max_scalars, uint64_t *n_scalars_out, uint8_t *digests_out, uint32_t max_digests, uint32_t *n_digests_out,
                                       double *phase_ms_out, bn_f128 *advice_out, uint64_t max_advice_elems, uint64_t *n_advice_elems_out)
{
	const PiopQueryPhase query{nullptr, advice_out, max_advice_elems, n_advice_elems_out, true, transcript};
	return piop_prove_committed_body(ctx, n_committed, committed_n_vars, d_committed, n_transparent, transparent_n_vars, d_transparent, n_claims, claims, claim_sums, log_dim,
	                                 log_inv_rate, log_batch_size, fold_arities, n_arities, n_test_queries, d_codeword, d_tree, d_scratch, scratch_elems, nullptr, 0, nullptr, 0,
	                                 items_out, max_items, n_items_out, scalars_out, max_scalars, n_scalars_out, digests_out, max_digests, n_digests_out, phase_ms_out, &query);
}

static thread_local double g_piop_commit_ms = 0;

// CommitMeta::total_vars and each multilinear's offset in the message of merge_multilins: pure host arithmetic
int bnh_piop_message_layout(uint32_t n, const uint32_t *n_vars, uint64_t *offsets_out, uint32_t *total_vars_out)
{
	return guarded([&]() -> int {
		if ((n && !offsets_out) || !total_vars_out) throw Error(Error::InputValidation, "null argument");
		piop_check_committed_n_vars(n, n_vars);
		uint64_t off = 0;
		for (uint32_t i = n; i-- > 0;) {
			offsets_out[i] = off;
			off += (uint64_t)1 << n_vars[i];
		}
		*total_vars_out = (uint32_t)CommitMeta::with_vars(std::vector<size_t>(n_vars, n_vars + n)).total_vars();
		return 0;
	});
}

// what bnh_piop_commit's caller provides, in field elements
int bnh_piop_commit_elems(uint32_t log_dim, uint32_t log_inv_rate, uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities,
                          uint64_t *codeword_elems_out, uint64_t *tree_elems_out)
{
	return guarded([&]() -> int {
		if (!codeword_elems_out || !tree_elems_out || (n_arities && !fold_arities)) throw Error(Error::InputValidation, "null argument");
		if ((uint64_t)log_dim + log_batch_size + log_inv_rate >= 48) throw Error(Error::InputValidation, "FRI parameters out of range");
		FRIParams p(log_dim, log_inv_rate, log_batch_size, std::vector<size_t>(fold_arities, fold_arities + n_arities), 0);
		*codeword_elems_out = (uint64_t)1 << p.log_len();
		*tree_elems_out = BinaryMerkleTreeProver::required_device_memory((size_t)1 << piop_commit_log_leaves(log_dim, log_inv_rate, log_batch_size, fold_arities, n_arities));
		return 0;
	});
}

// piop::commit (crates/core/src/piop/prove.rs:120-165) from the committed multilinears on the device, through fri.hpp's
// commit_interleaved over device slices: the merge into the codeword with every repeat, the batched NTT, the tree.
int bnh_piop_commit(bn_ctx *ctx, uint32_t n_committed, const uint32_t *committed_n_vars, const void *const *d_committed, uint32_t log_dim, uint32_t log_inv_rate,
                    uint32_t log_batch_size, const uint32_t *fold_arities, uint32_t n_arities, uint32_t n_test_queries, void *d_codeword, uint64_t codeword_elems,
                    void *d_tree, uint64_t tree_elems, uint8_t *commitment_out, double *phase_ms_out)
{
	return guarded([&]() -> int {
		if (!ctx || !d_codeword || !d_tree || !commitment_out || (n_committed && !d_committed) || (n_arities && !fold_arities))
			throw Error(Error::InputValidation, "null argument");
		piop_check_committed_n_vars(n_committed, committed_n_vars);
		uint64_t want_code = 0, want_tree = 0;
		if (const int rc = bnh_piop_commit_elems(log_dim, log_inv_rate, log_batch_size, fold_arities, n_arities, &want_code, &want_tree)) return rc;
		if (codeword_elems != want_code || tree_elems != want_tree)
			throw Error(Error::InputValidation, "piop commit: codeword_elems / tree_elems are not what bnh_piop_commit_elems states for these parameters");
		std::vector<FSlice> committed;
		for (uint32_t i = 0; i < n_committed; i++) {
			if (!d_committed[i]) throw Error(Error::InputValidation, "null argument");
			committed.push_back(FSlice{d_committed[i], (size_t)1 << committed_n_vars[i]});
		}
		if (CommitMeta::with_vars(std::vector<size_t>(committed_n_vars, committed_n_vars + n_committed)).total_vars() != (size_t)log_dim + log_batch_size)
			throw PiopError("FRI message length does not match the commit metadata's total_vars");
		ComputeLayer hal(ctx);
		DeviceBumpAllocator code_alloc(FSliceMut{d_codeword, (size_t)codeword_elems}), tree_alloc(FSliceMut{d_tree, (size_t)tree_elems});
		FRIParams p(log_dim, log_inv_rate, log_batch_size, std::vector<size_t>(fold_arities, fold_arities + n_arities), n_test_queries);
		AdditiveNTT ntt(hal, 5, p.rs_log_len());
		BinaryMerkleTreeProver merkle(hal);
		hal.sync();
		const auto t0 = std::chrono::steady_clock::now();
		CommitOutput co = commit_interleaved(hal, code_alloc, tree_alloc, p, ntt, merkle, committed, phase_ms_out);
		hal.sync();
		g_piop_commit_ms = elapsed_ms(t0, std::chrono::steady_clock::now());
		std::memcpy(commitment_out, co.commitment.data(), 32);
		return 0;
	});
}

// wall-clock milliseconds of the last bnh_piop_commit of this thread between the synchronisations around its commit_interleaved --
// what bnh_fri_commit_fold and bnh_piop_prove report as their commit phase; with phase_ms_out NULL there is no synchronisation inside
double bnh_piop_commit_last_ms(void) { return g_piop_commit_ms; }

// The front-loaded batch prover alone (protocols/sumcheck/prove/front_loaded.rs:33-203: BatchProver::run with the transcript's
// samples handed in): p BivariateSumcheckProvers on ONE layer, ascending by number of variables.
//   prover_desc[3 * i] = (n_vars, m, n_comps) of prover i; d_multilins: the m pointers of prover 0, then of prover 1, ...;
//   comp_indices / sums: likewise concatenated; batch_coeffs[n_provers]; challenges[max n_vars]
//   round_proofs_out[2 * total_rounds]: the truncated round polynomial of every round (missing coefficients zero);
//   final_evals_out: the provers' final evaluations concatenated in finishing (= input) order
static int batch_sumcheck_prove_body(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const void *const *d_multilins, const uint32_t *comp_indices,
                                     const bn_f128 *sums, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *challenges,
                                     bn_f128 *round_proofs_out, bn_f128 *final_evals_out, bool is_live, const bnh_transcript *transcript)
{
	return guarded([&]() -> int {
		// (public entry point: every pointer it dereferences and every shift amount it derives is checked first -- ADVICE r5)
		EntryTranscript et(is_live, transcript);
		if (!ctx || (n_provers && !prover_desc) || (!is_live && ((n_provers && !batch_coeffs) || !challenges)) || !round_proofs_out || !final_evals_out ||
		    (!d_scratch && scratch_elems))
			throw Error(Error::InputValidation, "null argument");
		size_t total_m = 0, total_c = 0;
		for (uint32_t i = 0; i < n_provers; i++) {
			if (prover_desc[3 * i] >= 48) throw Error(Error::InputValidation, "a prover's number of variables is out of range (< 48)");
			if (i && prover_desc[3 * i] < prover_desc[3 * (i - 1)]) throw Error(Error::InputValidation, "ClaimsOutOfOrder: provers ascend by number of variables");
			total_m += prover_desc[3 * i + 1];
			total_c += prover_desc[3 * i + 2];
		}
		if ((total_m && !d_multilins) || (total_c && (!comp_indices || !sums))) throw Error(Error::InputValidation, "null argument");
		for (size_t j = 0; j < total_m; j++)
			if (!d_multilins[j]) throw Error(Error::InputValidation, "null multilinear");
		ComputeLayer hal(ctx);
		DeviceBumpAllocator dev_alloc(FSliceMut{d_scratch, (size_t)scratch_elems});
		std::vector<B128> host_mem(total_m + 8);
		HostBumpAllocator host_alloc(HostSliceMut{host_mem.data(), host_mem.size()});
		std::vector<std::unique_ptr<BivariateSumcheckProver>> provers;
		size_t at_ml = 0, at_c = 0;
		for (uint32_t i = 0; i < n_provers; i++) {
			const uint32_t n_vars = prover_desc[3 * i], m = prover_desc[3 * i + 1], nc = prover_desc[3 * i + 2];
			std::vector<FSlice> mls;
			for (uint32_t j = 0; j < m; j++) mls.push_back(FSlice{d_multilins[at_ml + j], (size_t)1 << n_vars});
			provers.push_back(std::make_unique<BivariateSumcheckProver>(hal, dev_alloc, host_alloc, n_vars, index_compositions(m, nc, comp_indices + 2 * at_c),
			                                                            from_raw(sums + at_c, nc), mls));
			at_ml += m;
			at_c += nc;
		}
		// front_loaded::BatchProver::new (the batch coefficients, front_loaded.rs:51-59), then run (:175-197)
		const size_t total_rounds = provers.empty() ? 0 : provers.back()->n_vars();
		enum { BatchCoeffs = 0, Challenges = 1 };
		TranscriptSource &tr = et.source({from_raw(batch_coeffs, n_provers), from_raw(challenges, total_rounds)});
		const std::vector<B128> bcs = tr.sample_vec(BatchCoeffs, 0, n_provers);
		SumcheckBatchProver<BivariateSumcheckProver> batch(std::move(provers), bcs);
		put_batch_output(batch.run(tr, Challenges), round_proofs_out, final_evals_out);
		return 0;
	});
}

int bnh_batch_sumcheck_prove(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const void *const *d_multilins, const uint32_t *comp_indices,
                             const bn_f128 *sums, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *challenges,
                             bn_f128 *round_proofs_out, bn_f128 *final_evals_out)
{
	return batch_sumcheck_prove_body(ctx, n_provers, prover_desc, d_multilins, comp_indices, sums, d_scratch, scratch_elems, batch_coeffs, challenges, round_proofs_out,
	                                 final_evals_out, false, nullptr);
}

int bnh_batch_sumcheck_prove_live(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const void *const *d_multilins, const uint32_t *comp_indices,
                                  const bn_f128 *sums, void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript, bn_f128 *round_proofs_out,
                                  bn_f128 *final_evals_out)
{
	return batch_sumcheck_prove_body(ctx, n_provers, prover_desc, d_multilins, comp_indices, sums, d_scratch, scratch_elems, nullptr, nullptr, round_proofs_out,
	                                 final_evals_out, true, transcript);
}

// EqIndSumcheckProver (crates/core/src/protocols/sumcheck/prove/eq_ind.rs:378-644; binius_amd/host/eq_ind.hpp) over the old HAL
// (binius_hal::ComputationBackend -> bn_hal_round_evals / the ComputeLayer's folds), High-to-Low, compositions of degree 2: the
// zerocheck of a constraint set -- one composition per constraint over ALL multilinears of the table
// (core/src/constraint_system/prove.rs:431-505).
//   d_multilins[n_mls]: 2^n_vars elements each, FOLDED IN PLACE;  steps / steps_inf: the n_comps compositions and their leading
//   forms, concatenated (n_steps[c] / n_steps_inf[c] steps each);  sums[n_comps];  eq_ind_challenges[n_vars];
//   d_eq_ind: 2^(n_vars - 1) elements of scratch for the indicator's partial evaluations (expanded here, eq_ind.rs:430-446)
//   round_coeffs_out[(D + 2) * n_vars], D = max(2, largest degree): the round polynomials have degree D + 1 (D = 2 for the tables'
//   constraints: four coefficients per round); final_evals_out[n_mls + 1] (the last one: the indicator's prefix evaluation)
static int eqind_sumcheck_prove_body(bn_ctx *ctx, uint32_t n_vars, uint32_t n_mls, void *const *d_multilins, uint32_t n_comps, const bn_step *steps,
                                     const uint32_t *n_steps, const bn_step *steps_inf, const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *sums,
                                     const bn_f128 *eq_ind_challenges, void *d_eq_ind, uint64_t eq_ind_elems, const bn_f128 *batch_coeff, const bn_f128 *challenges,
                                     bn_f128 *round_coeffs_out, bn_f128 *final_evals_out, bool is_live, const bnh_transcript *transcript)
{
	return guarded([&]() -> int {
		EntryTranscript et(is_live, transcript);
		if (!ctx || (!d_multilins && n_mls) || (n_comps && (!steps || !n_steps || !steps_inf || !n_steps_inf || !sums)) || !eq_ind_challenges || !d_eq_ind ||
		    (!is_live && (!batch_coeff || !challenges)) || !round_coeffs_out || !final_evals_out)
			throw Error(Error::InputValidation, "null argument");
		if (n_vars == 0 || n_vars >= 40) throw Error(Error::InputValidation, "n_vars out of range");
		if (eq_ind_elems < ((uint64_t)1 << (n_vars - 1))) throw Error(Error::InputValidation, "the indicator's scratch holds fewer than 2^(n_vars - 1) elements");
		const bool prof = AbiProf::on(); // BNH_PROF=1: wall time of the set-up, of execute / fold over all rounds, of finish (diagnostic)
		auto now = [] { return std::chrono::steady_clock::now(); };
		const auto t_begin = now();
		ComputeLayer hal(ctx);
		Mi355xBackend backend(hal);
		DeviceBumpAllocator dev_alloc(FSliceMut{d_eq_ind, (size_t)eq_ind_elems});
		std::vector<FSlice> mls;
		for (uint32_t j = 0; j < n_mls; j++) mls.push_back(FSlice{d_multilins[j], (size_t)1 << n_vars});
		std::vector<EqIndComposition> comps;
		size_t at = 0, at_inf = 0;
		for (uint32_t c = 0; c < n_comps; c++) {
			EqIndComposition ec;
			ec.composition = hal.compile_expr(ArithCircuit::from_steps(std::vector<bn_step>(steps + at, steps + at + n_steps[c])));
			ec.composition_at_infinity = hal.compile_expr(ArithCircuit::from_steps(std::vector<bn_step>(steps_inf + at_inf, steps_inf + at_inf + n_steps_inf[c])));
			at += n_steps[c];
			at_inf += n_steps_inf[c];
			ec.degree = degrees ? degrees[c] : 2;
			comps.push_back(ec);
		}
		EqIndPointProver prover(hal, backend, dev_alloc, n_vars, std::move(mls), std::move(comps), from_raw(sums, n_comps), from_raw(eq_ind_challenges, n_vars));
		// a front-loaded batch of one: its coefficient first; what a round writes is the prover's polynomial times the coefficient
		// without its last coefficient (front_loaded.rs:128-135), while round_coeffs_out keeps the prover's own coefficients, all of them
		enum { BatchCoeff = 0, Challenges = 1 };
		TranscriptSource &tr = et.source({one_sample(batch_coeff), from_raw(challenges, n_vars)});
		const B128 bc = tr.sample(BatchCoeff, 0);
		double us_exec = 0, us_fold = 0;
		const auto t_setup = now();
		for (uint32_t r = 0; r < n_vars; r++) {
			const auto t0 = prof ? now() : std::chrono::steady_clock::time_point{};
			const std::vector<B128> rc = prover.execute(bc);
			const auto t1 = prof ? now() : t0;
			to_raw(rc, round_coeffs_out + rc.size() * r);
			if (tr.observes_writes()) {
				std::vector<B128> written(rc.begin(), rc.end() - (rc.empty() ? 0 : 1));
				for (B128 &c : written) c = c * bc;
				tr.write_scalars(written);
			}
			prover.fold(tr.sample(Challenges, r));
			if (prof) {
				us_exec += 1e3 * elapsed_ms(t0, t1);
				us_fold += 1e3 * elapsed_ms(t1);
			}
		}
		const auto t_rounds = now();
		const std::vector<B128> final_evals = prover.finish();
		tr.write_scalars(final_evals);
		to_raw(final_evals, final_evals_out);
		if (prof)
			fprintf(stderr, "[bnh prof] eq-ind sumcheck, %u rounds, %u multilinears, %u compositions: set-up %.1f us, execute %.1f us, fold %.1f us, finish %.1f us\n", n_vars,
			        n_mls, n_comps, 1e3 * elapsed_ms(t_begin, t_setup), us_exec, us_fold,
			        1e3 * elapsed_ms(t_rounds));
		return 0;
	});
}

int bnh_eqind_sumcheck_prove(bn_ctx *ctx, uint32_t n_vars, uint32_t n_mls, void *const *d_multilins, uint32_t n_comps, const bn_step *steps,
                             const uint32_t *n_steps, const bn_step *steps_inf, const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *sums,
                             const bn_f128 *eq_ind_challenges, void *d_eq_ind, uint64_t eq_ind_elems, const bn_f128 *batch_coeff, const bn_f128 *challenges,
                             bn_f128 *round_coeffs_out, bn_f128 *final_evals_out)
{
	return eqind_sumcheck_prove_body(ctx, n_vars, n_mls, d_multilins, n_comps, steps, n_steps, steps_inf, n_steps_inf, degrees, sums, eq_ind_challenges, d_eq_ind, eq_ind_elems,
	                                 batch_coeff, challenges, round_coeffs_out, final_evals_out, false, nullptr);
}

int bnh_eqind_sumcheck_prove_live(bn_ctx *ctx, uint32_t n_vars, uint32_t n_mls, void *const *d_multilins, uint32_t n_comps, const bn_step *steps,
                                  const uint32_t *n_steps, const bn_step *steps_inf, const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *sums,
                                  const bn_f128 *eq_ind_challenges, void *d_eq_ind, uint64_t eq_ind_elems, const bnh_transcript *transcript,
                                  bn_f128 *round_coeffs_out, bn_f128 *final_evals_out)
{
	return eqind_sumcheck_prove_body(ctx, n_vars, n_mls, d_multilins, n_comps, steps, n_steps, steps_inf, n_steps_inf, degrees, sums, eq_ind_challenges, d_eq_ind, eq_ind_elems,
	                                 nullptr, nullptr, round_coeffs_out, final_evals_out, true, transcript);
}

// gkr_gpa::batch_prove (crates/core/src/protocols/gkr_gpa/prove.rs:33-296) through the C++ mirror binius_amd/host/gkr_gpa.hpp; the
// arguments are described in include/binius_amd_host.h.
static int gkr_gpa_prove_body(bn_ctx *ctx, uint32_t n_claims, const uint32_t *n_vars, const void *const *d_inputs, const uint64_t *input_lens, void *const *d_arenas,
                              void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *sumcheck_challenges, const bn_f128 *gpa_challenges,
                              bn_f128 *products_out, bn_f128 *round_proofs_out, bn_f128 *layer_evals_out, bn_f128 *final_points_out, bn_f128 *final_evals_out,
                              double *step_ms_out, bool is_live, const bnh_transcript *transcript)
{
	return guarded([&]() -> int {
		EntryTranscript et(is_live, transcript);
		if (!ctx) throw Error(Error::InputValidation, "null ctx");
		if (n_claims == 0) return 0;
		if (!n_vars || !d_inputs || !input_lens || !d_arenas || !products_out || !final_evals_out) throw Error(Error::InputValidation, "null argument");
		size_t max_n = 0;
		std::vector<size_t> nv(n_claims);
		std::vector<FSlice> ins(n_claims);
		std::vector<FSliceMut> ars(n_claims);
		for (uint32_t t = 0; t < n_claims; t++) {
			if (n_vars[t] > BN_PRODUCT_TREE_MAX_VARS) throw Error(Error::InputValidation, "n_vars out of range (0 .. 28)");
			nv[t] = n_vars[t];
			max_n = std::max(max_n, nv[t]);
			ins[t] = FSlice{d_inputs[t], (size_t)input_lens[t]};
			if (nv[t] >= 1 && !d_arenas[t]) throw Error(Error::InputValidation, "null layer arena");
			ars[t] = FSliceMut{d_arenas[t], (size_t)1 << nv[t]};
		}
		if (max_n >= 1 && (!d_scratch || (!is_live && (!batch_coeffs || !gpa_challenges)) || !layer_evals_out || !final_points_out)) throw Error(Error::InputValidation, "null argument");
		if (max_n >= 2 && ((!is_live && !sumcheck_challenges) || !round_proofs_out)) throw Error(Error::InputValidation, "null argument");
		ComputeLayer hal(ctx);
		Mi355xBackend backend(hal);
		TranscriptSource &tr = et.source({from_raw(batch_coeffs, max_n), from_raw(sumcheck_challenges, max_n * (max_n ? max_n - 1 : 0) / 2), from_raw(gpa_challenges, max_n)});
		const GkrGpaOutput out = gkr_gpa_batch_prove(hal, backend, nv, ins, ars, FSliceMut{d_scratch, (size_t)scratch_elems}, tr);
		put_gkr_gpa_output(out, products_out, round_proofs_out, layer_evals_out, final_points_out, final_evals_out);
		for (size_t j = 0; step_ms_out && j < out.step_ms.size(); j++) step_ms_out[j] = out.step_ms[j];
		return 0;
	});
}

int bnh_gkr_gpa_prove(bn_ctx *ctx, uint32_t n_claims, const uint32_t *n_vars, const void *const *d_inputs, const uint64_t *input_lens, void *const *d_arenas,
                      void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *sumcheck_challenges, const bn_f128 *gpa_challenges,
                      bn_f128 *products_out, bn_f128 *round_proofs_out, bn_f128 *layer_evals_out, bn_f128 *final_points_out, bn_f128 *final_evals_out,
                      double *step_ms_out)
{
	return gkr_gpa_prove_body(ctx, n_claims, n_vars, d_inputs, input_lens, d_arenas, d_scratch, scratch_elems, batch_coeffs, sumcheck_challenges, gpa_challenges, products_out,
	                          round_proofs_out, layer_evals_out, final_points_out, final_evals_out, step_ms_out, false, nullptr);
}

int bnh_gkr_gpa_prove_live(bn_ctx *ctx, uint32_t n_claims, const uint32_t *n_vars, const void *const *d_inputs, const uint64_t *input_lens, void *const *d_arenas,
                           void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript, bn_f128 *products_out, bn_f128 *round_proofs_out,
                           bn_f128 *layer_evals_out, bn_f128 *final_points_out, bn_f128 *final_evals_out, double *step_ms_out)
{
	return gkr_gpa_prove_body(ctx, n_claims, n_vars, d_inputs, input_lens, d_arenas, d_scratch, scratch_elems, nullptr, nullptr, nullptr, products_out, round_proofs_out,
	                          layer_evals_out, final_points_out, final_evals_out, step_ms_out, true, transcript);
}

// gkr_exp::batch_prove (crates/core/src/protocols/gkr_exp/batch_prove.rs:46-315) through the C++ mirror binius_amd/host/gkr_exp.hpp; the
// arguments and the layout of the outputs are described in include/binius_amd_host.h.
static int gkr_exp_prove_body(bn_ctx *ctx, uint32_t n_witnesses, const uint32_t *widths, const uint32_t *kinds, const void *const *d_exponent_bits,
                              const bn_f128 *static_bases, const void *const *d_bases, void *const *d_arenas, uint32_t n_claims, const uint32_t *n_vars,
                              const bn_f128 *eval_points, const bn_f128 *evals, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs,
                              const bn_f128 *challenges, uint32_t *n_layers_out, uint32_t *rounds_per_layer_out, uint32_t *coeffs_per_round_out,
                              bn_f128 *round_proofs_out, uint32_t *provers_per_layer_out, uint32_t *evals_per_prover_out, bn_f128 *multilinear_evals_out,
                              uint32_t *claims_per_layer_out, uint32_t *claim_n_vars_out, bn_f128 *claim_points_out, bn_f128 *claim_evals_out, double *layer_ms_out,
                              bool is_live, const bnh_transcript *transcript)
{
	return guarded([&]() -> int {
		EntryTranscript et(is_live, transcript);
		if (!ctx) throw Error(Error::InputValidation, "null ctx");
		if (n_witnesses != n_claims) throw Error(Error::InputValidation, "MismatchedWitnessClaimLength");
		if (n_layers_out) *n_layers_out = 0;
		if (n_claims == 0) return 0;
		if (!widths || !kinds || !d_exponent_bits || !static_bases || !d_bases || !d_arenas || !n_vars || !evals || (!is_live && !batch_coeffs) || !n_layers_out ||
		    !rounds_per_layer_out || !coeffs_per_round_out || !round_proofs_out || !provers_per_layer_out || !evals_per_prover_out || !multilinear_evals_out ||
		    !claims_per_layer_out || !claim_n_vars_out || !claim_points_out || !claim_evals_out)
			throw Error(Error::InputValidation, "null argument");
		const size_t k = n_claims;
		size_t max_w = 0, max_n = 0, at_bits = 0, at_pt = 0;
		std::vector<GkrExpClaim> claims(k);
		for (size_t t = 0; t < k; t++) {
			GkrExpClaim &c = claims[t];
			if (n_vars[t] > BN_EXP_MAX_VARS) throw Error(Error::InputValidation, "n_vars out of range (0 .. 28)");
			if (widths[t] < 1 || widths[t] > BN_EXP_MAX_WIDTH) throw Error(Error::InputValidation, "width out of range (1 .. 128)");
			if (kinds[t] != BN_EXP_STATIC && kinds[t] != BN_EXP_DYNAMIC) throw Error(Error::InputValidation, "unknown kind");
			c.n_vars = n_vars[t];
			c.width = widths[t];
			c.dynamic = kinds[t] == BN_EXP_DYNAMIC;
			c.static_base = from_raw(static_bases[t]);
			c.base = FSlice{d_bases[t], c.dynamic ? (size_t)1 << c.n_vars : 0};
			c.bits.assign(d_exponent_bits + at_bits, d_exponent_bits + at_bits + c.width);
			at_bits += c.width;
			c.arena = FSliceMut{d_arenas[t], c.width << c.n_vars};
			if (c.n_vars && !eval_points) throw Error(Error::InputValidation, "null argument");
			c.eval_point = from_raw(eval_points + at_pt, c.n_vars);
			at_pt += c.n_vars;
			c.eval = from_raw(evals[t]);
			max_w = std::max(max_w, c.width);
			max_n = std::max(max_n, c.n_vars);
		}
		if (max_n && !is_live && !challenges) throw Error(Error::InputValidation, "null argument");
		if (!d_scratch && scratch_elems) throw Error(Error::InputValidation, "null argument");
		ComputeLayer hal(ctx);
		Mi355xBackend backend(hal);
		TranscriptSource &tr = et.source({from_raw(batch_coeffs, max_w * k), from_raw(challenges, max_w * max_n)});
		const GkrExpOutput out = gkr_exp_batch_prove(hal, backend, n_witnesses, claims, FSliceMut{d_scratch, (size_t)scratch_elems}, tr);
		*n_layers_out = (uint32_t)out.round_proofs.size();
		for (size_t L = 0; L < out.round_proofs.size(); L++) {
			rounds_per_layer_out[L] = (uint32_t)out.round_proofs[L].size();
			for (size_t r = 0; r < out.round_proofs[L].size(); r++) {
				coeffs_per_round_out[L * std::max<size_t>(max_n, 1) + r] = (uint32_t)out.round_proofs[L][r].size();
				round_proofs_out = to_raw(out.round_proofs[L][r], round_proofs_out);
			}
			provers_per_layer_out[L] = (uint32_t)out.multilinear_evals[L].size();
			for (size_t g = 0; g < out.multilinear_evals[L].size(); g++) {
				evals_per_prover_out[L * k + g] = (uint32_t)out.multilinear_evals[L][g].size();
				multilinear_evals_out = to_raw(out.multilinear_evals[L][g], multilinear_evals_out);
			}
			claims_per_layer_out[L] = (uint32_t)out.layer_claims[L].size();
			for (size_t i = 0; i < out.layer_claims[L].size(); i++) {
				const GkrExpLayerClaim &lc = out.layer_claims[L][i];
				claim_n_vars_out[L * 2 * k + i] = (uint32_t)lc.eval_point.size();
				claim_points_out = to_raw(lc.eval_point, claim_points_out);
				*claim_evals_out++ = lc.eval.raw();
			}
			if (layer_ms_out) layer_ms_out[L] = out.layer_ms[L];
		}
		return 0;
	});
}

int bnh_gkr_exp_prove(bn_ctx *ctx, uint32_t n_witnesses, const uint32_t *widths, const uint32_t *kinds, const void *const *d_exponent_bits,
                      const bn_f128 *static_bases, const void *const *d_bases, void *const *d_arenas, uint32_t n_claims, const uint32_t *n_vars,
                      const bn_f128 *eval_points, const bn_f128 *evals, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs,
                      const bn_f128 *challenges, uint32_t *n_layers_out, uint32_t *rounds_per_layer_out, uint32_t *coeffs_per_round_out,
                      bn_f128 *round_proofs_out, uint32_t *provers_per_layer_out, uint32_t *evals_per_prover_out, bn_f128 *multilinear_evals_out,
                      uint32_t *claims_per_layer_out, uint32_t *claim_n_vars_out, bn_f128 *claim_points_out, bn_f128 *claim_evals_out, double *layer_ms_out)
{
	return gkr_exp_prove_body(ctx, n_witnesses, widths, kinds, d_exponent_bits, static_bases, d_bases, d_arenas, n_claims, n_vars, eval_points, evals, d_scratch, scratch_elems,
	                          batch_coeffs, challenges, n_layers_out, rounds_per_layer_out, coeffs_per_round_out, round_proofs_out, provers_per_layer_out,
	                          evals_per_prover_out, multilinear_evals_out, claims_per_layer_out, claim_n_vars_out, claim_points_out, claim_evals_out, layer_ms_out, false,
	                          nullptr);
}

int bnh_gkr_exp_prove_live(bn_ctx *ctx, uint32_t n_witnesses, const uint32_t *widths, const uint32_t *kinds, const void *const *d_exponent_bits,
                           const bn_f128 *static_bases, const void *const *d_bases, void *const *d_arenas, uint32_t n_claims, const uint32_t *n_vars,
                           const bn_f128 *eval_points, const bn_f128 *evals, void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript,
                           uint32_t *n_layers_out, uint32_t *rounds_per_layer_out, uint32_t *coeffs_per_round_out, bn_f128 *round_proofs_out,
                           uint32_t *provers_per_layer_out, uint32_t *evals_per_prover_out, bn_f128 *multilinear_evals_out, uint32_t *claims_per_layer_out,
                           uint32_t *claim_n_vars_out, bn_f128 *claim_points_out, bn_f128 *claim_evals_out, double *layer_ms_out)
{
	return gkr_exp_prove_body(ctx, n_witnesses, widths, kinds, d_exponent_bits, static_bases, d_bases, d_arenas, n_claims, n_vars, eval_points, evals, d_scratch, scratch_elems,
	                          nullptr, nullptr, n_layers_out, rounds_per_layer_out, coeffs_per_round_out, round_proofs_out, provers_per_layer_out, evals_per_prover_out,
	                          multilinear_evals_out, claims_per_layer_out, claim_n_vars_out, claim_points_out, claim_evals_out, layer_ms_out, true, transcript);
}

// The product-check phase of the constraint-system prover (core/src/constraint_system/prove.rs:276-428) through the C++ mirror
// binius_amd/host/flush.hpp; the arguments and the layout of the outputs are described in include/binius_amd_host.h.
static int flush_prodcheck_prove_body(bn_ctx *ctx, uint32_t n_flushes, const uint32_t *channel_ids, const uint32_t *flush_n_vars, const uint32_t *n_selectors,
                              const uint32_t *selector_ids, const void *const *d_selectors, const uint32_t *n_entries, const uint32_t *entry_kinds,
                              const uint32_t *entry_ids, const void *const *d_entry_columns, const uint32_t *entry_levels, const bn_f128 *entry_consts,
                              uint32_t n_nonzero, const uint32_t *nonzero_ids, const void *const *d_nonzero_columns, const uint32_t *nonzero_levels,
                              const uint32_t *nonzero_n_vars, const bn_f128 *mixing_challenge, const bn_f128 *permutation_challenges, uint32_t n_channels,
                              void *d_scratch, uint64_t scratch_elems, const bn_f128 *gpa_batch_coeffs, const bn_f128 *gpa_sumcheck_challenges,
                              const bn_f128 *gpa_challenges, const bn_f128 *red_batch_coeffs, const bn_f128 *red_challenges, uint64_t *prefix_lens_out,
                              bn_f128 *products_out, bn_f128 *gpa_round_proofs_out, bn_f128 *gpa_layer_evals_out, bn_f128 *gpa_final_points_out,
                              bn_f128 *gpa_final_evals_out, uint32_t *n_checks_out, uint32_t *check_desc_out, uint32_t *check_ids_out,
                              bn_f128 *check_round_proofs_out, bn_f128 *check_final_evals_out, uint32_t *n_linear_out, uint32_t *linear_flushes_out,
                              double *phase_ms_out, bool is_live, const bnh_transcript *transcript)
{
	return guarded([&]() -> int {
		EntryTranscript et(is_live, transcript);
		if (!ctx) throw Error(Error::InputValidation, "null ctx");
		if (n_checks_out) *n_checks_out = 0;
		if (n_linear_out) *n_linear_out = 0;
		if (n_flushes + n_nonzero == 0) {
			// (nothing to prove, but the reference still draws the mixing and the permutation challenges here, prove.rs:329-330)
			if (is_live) flush_prodcheck_empty(*et.live, n_channels);
			return 0;
		}
		if ((!is_live && !mixing_challenge) || !d_scratch || !products_out || !gpa_final_evals_out || !n_checks_out || !n_linear_out) throw Error(Error::InputValidation, "null argument");
		if (n_flushes && (!channel_ids || !flush_n_vars || !n_selectors || !n_entries || !entry_kinds || !entry_ids || !d_entry_columns || !entry_levels || !entry_consts ||
		                  (!is_live && !permutation_challenges) || !prefix_lens_out || !check_desc_out || !check_ids_out || !check_round_proofs_out || !check_final_evals_out ||
		                  !linear_flushes_out || (!is_live && !red_batch_coeffs)))
			throw Error(Error::InputValidation, "null argument");
		if (n_nonzero && (!nonzero_ids || !d_nonzero_columns || !nonzero_levels || !nonzero_n_vars)) throw Error(Error::InputValidation, "null argument");
		std::vector<FlushSpec> flushes(n_flushes);
		std::vector<NonZeroSpec> nonzero(n_nonzero);
		size_t at_s = 0, at_e = 0, max_n = 0;
		for (uint32_t f = 0; f < n_flushes; f++) {
			FlushSpec &fl = flushes[f];
			fl.channel = channel_ids[f];
			fl.n_vars = flush_n_vars[f];
			max_n = std::max(max_n, fl.n_vars);
			if (n_selectors[f] && (!selector_ids || !d_selectors)) throw Error(Error::InputValidation, "null argument");
			for (uint32_t i = 0; i < n_selectors[f]; i++, at_s++) fl.selectors.push_back(FlushSelector{selector_ids[at_s], d_selectors[at_s]});
			for (uint32_t i = 0; i < n_entries[f]; i++, at_e++) {
				FlushEntry e;
				if (entry_kinds[at_e] != BNH_FLUSH_ORACLE && entry_kinds[at_e] != BNH_FLUSH_CONST) throw Error(Error::InputValidation, "unknown flush entry kind");
				e.is_const = entry_kinds[at_e] == BNH_FLUSH_CONST;
				e.id = entry_ids[at_e];
				e.column = d_entry_columns[at_e];
				e.level = entry_levels[at_e];
				e.base = from_raw(entry_consts[at_e]);
				fl.entries.push_back(e);
			}
		}
		for (uint32_t i = 0; i < n_nonzero; i++) {
			nonzero[i] = NonZeroSpec{nonzero_ids[i], nonzero_n_vars[i], d_nonzero_columns[i], nonzero_levels[i]};
			max_n = std::max(max_n, nonzero[i].n_vars);
		}
		if (max_n > BN_PRODUCT_TREE_MAX_VARS) throw Error(Error::InputValidation, "n_vars out of range (0 .. 28)");
		if (max_n >= 1 && ((!is_live && (!gpa_batch_coeffs || !gpa_challenges)) || !gpa_layer_evals_out || !gpa_final_points_out)) throw Error(Error::InputValidation, "null argument");
		if (max_n >= 2 && ((!is_live && !gpa_sumcheck_challenges) || !gpa_round_proofs_out)) throw Error(Error::InputValidation, "null argument");
		size_t red_n = 0;
		const std::vector<FlushMleCheck> groups = flush_groups(flushes);
		for (const FlushMleCheck &g : groups) red_n += g.n_vars;
		if (red_n && !is_live && !red_challenges) throw Error(Error::InputValidation, "null argument");
		ComputeLayer hal(ctx);
		Mi355xBackend backend(hal);
		// (the streams as flush.hpp numbers them: the grand-product argument's three, the reductions' two, the mixing and the permutation challenges)
		TranscriptSource &tr = et.source({from_raw(gpa_batch_coeffs, max_n), from_raw(gpa_sumcheck_challenges, max_n * (max_n ? max_n - 1 : 0) / 2), from_raw(gpa_challenges, max_n),
		                                  from_raw(red_batch_coeffs, groups.size()), from_raw(red_challenges, red_n), one_sample(mixing_challenge),
		                                  from_raw(permutation_challenges, n_channels)});
		const FlushProdcheckOutput out = flush_prodcheck_prove(hal, backend, flushes, nonzero, n_channels, FSliceMut{d_scratch, (size_t)scratch_elems}, tr);
		for (uint32_t f = 0; f < n_flushes; f++) prefix_lens_out[f] = out.prefix_lens[f];
		put_gkr_gpa_output(out.gpa, products_out, gpa_round_proofs_out, gpa_layer_evals_out, gpa_final_points_out, gpa_final_evals_out);
		*n_checks_out = (uint32_t)out.checks.size();
		size_t at_i = 0;
		for (size_t g = 0; g < out.checks.size(); g++) {
			const FlushMleCheck &c = out.checks[g];
			check_desc_out[3 * g] = (uint32_t)c.n_vars;
			check_desc_out[3 * g + 1] = (uint32_t)c.ids.size();
			check_desc_out[3 * g + 2] = c.round_proofs.empty() ? 0 : (uint32_t)c.round_proofs[0].size();
			for (size_t id : c.ids) check_ids_out[at_i++] = (uint32_t)id;
			for (const auto &r : c.round_proofs) check_round_proofs_out = to_raw(r, check_round_proofs_out);
			check_final_evals_out = to_raw(c.final_evals, check_final_evals_out);
		}
		*n_linear_out = (uint32_t)out.linear_flushes.size();
		for (size_t i = 0; i < out.linear_flushes.size(); i++) linear_flushes_out[i] = (uint32_t)out.linear_flushes[i];
		if (phase_ms_out)
			for (int i = 0; i < 4; i++) phase_ms_out[i] = out.phase_ms[i];
		return 0;
	});
}

int bnh_flush_prodcheck_prove(bn_ctx *ctx, uint32_t n_flushes, const uint32_t *channel_ids, const uint32_t *flush_n_vars, const uint32_t *n_selectors,
                              const uint32_t *selector_ids, const void *const *d_selectors, const uint32_t *n_entries, const uint32_t *entry_kinds,
                              const uint32_t *entry_ids, const void *const *d_entry_columns, const uint32_t *entry_levels, const bn_f128 *entry_consts,
                              uint32_t n_nonzero, const uint32_t *nonzero_ids, const void *const *d_nonzero_columns, const uint32_t *nonzero_levels,
                              const uint32_t *nonzero_n_vars, const bn_f128 *mixing_challenge, const bn_f128 *permutation_challenges, uint32_t n_channels,
                              void *d_scratch, uint64_t scratch_elems, const bn_f128 *gpa_batch_coeffs, const bn_f128 *gpa_sumcheck_challenges,
                              const bn_f128 *gpa_challenges, const bn_f128 *red_batch_coeffs, const bn_f128 *red_challenges, uint64_t *prefix_lens_out,
                              bn_f128 *products_out, bn_f128 *gpa_round_proofs_out, bn_f128 *gpa_layer_evals_out, bn_f128 *gpa_final_points_out,
                              bn_f128 *gpa_final_evals_out, uint32_t *n_checks_out, uint32_t *check_desc_out, uint32_t *check_ids_out,
                              bn_f128 *check_round_proofs_out, bn_f128 *check_final_evals_out, uint32_t *n_linear_out, uint32_t *linear_flushes_out,
                              double *phase_ms_out)
{
	return flush_prodcheck_prove_body(ctx, n_flushes, channel_ids, flush_n_vars, n_selectors, selector_ids, d_selectors, n_entries, entry_kinds, entry_ids, d_entry_columns,
	                                  entry_levels, entry_consts, n_nonzero, nonzero_ids, d_nonzero_columns, nonzero_levels, nonzero_n_vars, mixing_challenge,
	                                  permutation_challenges, n_channels, d_scratch, scratch_elems, gpa_batch_coeffs, gpa_sumcheck_challenges, gpa_challenges, red_batch_coeffs,
	                                  red_challenges, prefix_lens_out, products_out, gpa_round_proofs_out, gpa_layer_evals_out, gpa_final_points_out, gpa_final_evals_out,
	                                  n_checks_out, check_desc_out, check_ids_out, check_round_proofs_out, check_final_evals_out, n_linear_out, linear_flushes_out, phase_ms_out,
	                                  false, nullptr);
}

int bnh_flush_prodcheck_prove_live(bn_ctx *ctx, uint32_t n_flushes, const uint32_t *channel_ids, const uint32_t *flush_n_vars, const uint32_t *n_selectors,
                                   const uint32_t *selector_ids, const void *const *d_selectors, const uint32_t *n_entries, const uint32_t *entry_kinds,
                                   const uint32_t *entry_ids, const void *const *d_entry_columns, const uint32_t *entry_levels, const bn_f128 *entry_consts,
                                   uint32_t n_nonzero, const uint32_t *nonzero_ids, const void *const *d_nonzero_columns, const uint32_t *nonzero_levels,
                                   const uint32_t *nonzero_n_vars, uint32_t n_channels, void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript,
                                   uint64_t *prefix_lens_out, bn_f128 *products_out, bn_f128 *gpa_round_proofs_out, bn_f128 *gpa_layer_evals_out,
                                   bn_f128 *gpa_final_points_out, bn_f128 *gpa_final_evals_out, uint32_t *n_checks_out, uint32_t *check_desc_out, uint32_t *check_ids_out,
                                   bn_f128 *check_round_proofs_out, bn_f128 *check_final_evals_out, uint32_t *n_linear_out, uint32_t *linear_flushes_out,
                                   double *phase_ms_out)
{
	return flush_prodcheck_prove_body(ctx, n_flushes, channel_ids, flush_n_vars, n_selectors, selector_ids, d_selectors, n_entries, entry_kinds, entry_ids, d_entry_columns,
	                                  entry_levels, entry_consts, n_nonzero, nonzero_ids, d_nonzero_columns, nonzero_levels, nonzero_n_vars, nullptr, nullptr, n_channels,
	                                  d_scratch, scratch_elems, nullptr, nullptr, nullptr, nullptr, nullptr, prefix_lens_out, products_out, gpa_round_proofs_out,
	                                  gpa_layer_evals_out, gpa_final_points_out, gpa_final_evals_out, n_checks_out, check_desc_out, check_ids_out, check_round_proofs_out,
	                                  check_final_evals_out, n_linear_out, linear_flushes_out, phase_ms_out, true, transcript);
}

// One round of evalcheck's bivariate sumchecks (evalcheck/subclaims.rs:549-586 with the witness construction in front of it) through
// the C++ mirror binius_amd/host/evalcheck.hpp; the arguments and the layout of the outputs are described in include/binius_amd_host.h.
// (with_lincomb: the _lc entry, which alone accepts BNH_EC_LINCOMB and reads the term arrays and the offsets)
static int evalcheck_bivariate_prove_capi(bool with_lincomb, bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const uint32_t *ml_desc,
                                          const void *const *d_columns, uint32_t n_terms, const uint32_t *term_levels, const void *const *d_term_columns,
                                          const bn_f128 *term_coeffs, const bn_f128 *ml_offsets, const bn_f128 *point_pool, uint32_t pool_len,
                                          const uint32_t *comp_indices, const bn_f128 *sums, void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs,
                                          const bn_f128 *challenges, bn_f128 *round_proofs_out, bn_f128 *final_evals_out, bool is_live = false,
                                          const bnh_transcript *transcript = nullptr)
{
	return guarded([&]() -> int {
		EntryTranscript et(is_live, transcript);
		if (!ctx || (n_provers && (!prover_desc || (!is_live && !batch_coeffs))) || !round_proofs_out || !final_evals_out || (!d_scratch && scratch_elems) || (pool_len && !point_pool))
			throw Error(Error::InputValidation, "null argument");
		size_t total_m = 0, total_c = 0, max_b = 0;
		for (uint32_t i = 0; i < n_provers; i++) {
			if (prover_desc[3 * i] > 12) throw Error(Error::InputValidation, "a prover of an evalcheck round has at most 12 variables");
			max_b = std::max<size_t>(max_b, prover_desc[3 * i]);
			total_m += prover_desc[3 * i + 1];
			total_c += prover_desc[3 * i + 2];
		}
		if ((total_m && (!ml_desc || !d_columns)) || (total_c && (!comp_indices || !sums)) || (max_b && !is_live && !challenges)) throw Error(Error::InputValidation, "null argument");
		if (n_terms && (!term_levels || !d_term_columns || !term_coeffs)) throw Error(Error::InputValidation, "null argument");
		const std::vector<B128> pool = from_raw(point_pool, pool_len);
		std::vector<EvalcheckTerm> terms(n_terms);
		for (uint32_t t = 0; t < n_terms; t++) terms[t] = EvalcheckTerm{d_term_columns[t], term_levels[t], B128(term_coeffs[t].lo, term_coeffs[t].hi)};
		std::vector<EvalcheckProver> provers(n_provers);
		size_t at_ml = 0, at_c = 0;
		for (uint32_t i = 0; i < n_provers; i++) {
			EvalcheckProver &p = provers[i];
			p.n_vars = prover_desc[3 * i];
			const uint32_t m = prover_desc[3 * i + 1], nc = prover_desc[3 * i + 2];
			for (uint32_t j = 0; j < m; j++, at_ml++) {
				const uint32_t *d = ml_desc + (size_t)BNH_EC_DESC_WORDS * at_ml;
				EvalcheckMultilinear ml;
				switch (d[0]) {
				case BNH_EC_PROJECTION:
					ml.kind = EvalcheckMultilinear::Projection;
					ml.d_column = d_columns[at_ml];
					ml.tower_level = d[1];
					ml.n_vars = d[2];
					ml.suffix_off = d[3];
					ml.suffix_len = d[4];
					if (ml.suffix_len > 48) throw Error(Error::InputValidation, "a suffix has at most 48 coordinates");
					break;
				case BNH_EC_SHIFT_IND:
					ml.kind = EvalcheckMultilinear::ShiftInd;
					ml.block_size = d[1];
					ml.shift_offset = d[2];
					if (d[3] > BNH_SHIFT_LOGICAL_RIGHT) throw Error(Error::InputValidation, "shift indicator: unknown variant");
					ml.variant = (ShiftVariant)d[3];
					ml.r_off = d[4];
					ml.r_len = d[5];
					break;
				case BNH_EC_TOWER_BASIS:
					ml.kind = EvalcheckMultilinear::TowerBasis;
					ml.k = d[1];
					ml.iota = d[2];
					break;
				case BNH_EC_LINCOMB:
					if (!with_lincomb) throw Error(Error::InputValidation, "unknown multilinear kind");
					if (!ml_offsets) throw Error(Error::InputValidation, "null argument");
					ml.kind = EvalcheckMultilinear::LinComb;
					ml.n_vars = d[1];
					ml.suffix_off = d[2];
					ml.suffix_len = d[3];
					ml.first_term = d[4];
					ml.n_terms = d[5];
					ml.offset = B128(ml_offsets[at_ml].lo, ml_offsets[at_ml].hi);
					if (ml.suffix_len > 48) throw Error(Error::InputValidation, "a suffix has at most 48 coordinates");
					break;
				default: throw Error(Error::InputValidation, "unknown multilinear kind");
				}
				p.multilins.push_back(ml);
			}
			p.compositions = index_compositions(m, nc, comp_indices + 2 * at_c);
			p.sums = from_raw(sums + at_c, nc);
			at_c += nc;
		}
		ComputeLayer hal(ctx);
		TranscriptSource &tr = et.source({from_raw(batch_coeffs, n_provers), from_raw(challenges, max_b)});
		const EvalcheckOutput out = evalcheck_bivariate_prove(hal, provers, pool, FSliceMut{d_scratch, (size_t)scratch_elems}, tr, terms);
		put_batch_output(out, round_proofs_out, final_evals_out);
		return 0;
	});
}

int bnh_evalcheck_bivariate_prove(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const uint32_t *ml_desc, const void *const *d_columns,
                                  const bn_f128 *point_pool, uint32_t pool_len, const uint32_t *comp_indices, const bn_f128 *sums, void *d_scratch,
                                  uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *challenges, bn_f128 *round_proofs_out,
                                  bn_f128 *final_evals_out)
{
	return evalcheck_bivariate_prove_capi(false, ctx, n_provers, prover_desc, ml_desc, d_columns, 0, nullptr, nullptr, nullptr, nullptr, point_pool, pool_len, comp_indices,
	                                      sums, d_scratch, scratch_elems, batch_coeffs, challenges, round_proofs_out, final_evals_out);
}

int bnh_evalcheck_bivariate_prove_lc(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const uint32_t *ml_desc, const void *const *d_columns,
                                     uint32_t n_terms, const uint32_t *term_levels, const void *const *d_term_columns, const bn_f128 *term_coeffs,
                                     const bn_f128 *ml_offsets, const bn_f128 *point_pool, uint32_t pool_len, const uint32_t *comp_indices, const bn_f128 *sums,
                                     void *d_scratch, uint64_t scratch_elems, const bn_f128 *batch_coeffs, const bn_f128 *challenges, bn_f128 *round_proofs_out,
                                     bn_f128 *final_evals_out)
{
	return evalcheck_bivariate_prove_capi(true, ctx, n_provers, prover_desc, ml_desc, d_columns, n_terms, term_levels, d_term_columns, term_coeffs, ml_offsets, point_pool,
	                                      pool_len, comp_indices, sums, d_scratch, scratch_elems, batch_coeffs, challenges, round_proofs_out, final_evals_out);
}

int bnh_evalcheck_bivariate_prove_lc_live(bn_ctx *ctx, uint32_t n_provers, const uint32_t *prover_desc, const uint32_t *ml_desc, const void *const *d_columns,
                                          uint32_t n_terms, const uint32_t *term_levels, const void *const *d_term_columns, const bn_f128 *term_coeffs,
                                          const bn_f128 *ml_offsets, const bn_f128 *point_pool, uint32_t pool_len, const uint32_t *comp_indices, const bn_f128 *sums,
                                          void *d_scratch, uint64_t scratch_elems, const bnh_transcript *transcript, bn_f128 *round_proofs_out, bn_f128 *final_evals_out)
{
	return evalcheck_bivariate_prove_capi(true, ctx, n_provers, prover_desc, ml_desc, d_columns, n_terms, term_levels, d_term_columns, term_coeffs, ml_offsets, point_pool,
	                                      pool_len, comp_indices, sums, d_scratch, scratch_elems, nullptr, nullptr, round_proofs_out, final_evals_out, true, transcript);
}

// The evaluations in front of an evalcheck round (evalcheck/prove.rs:191-275) through evalcheck_evaluate_claims of the same mirror; the
// arguments are described in include/binius_amd_host.h.
static_assert(BNH_EVALCHECK_LO_SPLIT == kEvalcheckLoSplit, "include/binius_amd_host.h states the split the mirror uses");
namespace {
std::vector<EvalcheckEvalClaim> evalcheck_eval_claims(uint32_t n_claims, const uint32_t *claim_desc, const void *const *d_columns)
{
	std::vector<EvalcheckEvalClaim> claims;
	for (uint32_t i = 0; i < n_claims; i++)
		claims.push_back(EvalcheckEvalClaim{d_columns ? d_columns[i] : nullptr, claim_desc[4 * i], claim_desc[4 * i + 1], claim_desc[4 * i + 2], claim_desc[4 * i + 3]});
	return claims;
}
} // namespace

uint64_t bnh_evalcheck_evaluate_scratch_elems(uint32_t n_claims, const uint32_t *claim_desc, uint32_t lo_split)
{
	if (n_claims && !claim_desc) return 0;
	try {
		return evalcheck_evaluate_scratch_elems(evalcheck_eval_claims(n_claims, claim_desc, nullptr), lo_split ? lo_split : kEvalcheckLoSplit);
	} catch (const Error &) {
		return 0;
	}
}

int bnh_evalcheck_evaluate(bn_ctx *ctx, uint32_t n_claims, const uint32_t *claim_desc, const void *const *d_columns, const bn_f128 *point_pool, uint32_t pool_len,
                           void *d_scratch, uint64_t scratch_elems, bn_f128 *evals_out, double *phase_ms_out)
{
	return guarded([&]() -> int {
		if (!ctx || (n_claims && (!claim_desc || !d_columns || !evals_out)) || (pool_len && !point_pool) || (!d_scratch && scratch_elems))
			throw Error(Error::InputValidation, "null argument");
		ComputeLayer hal(ctx);
		const EvalcheckEvaluateOutput out = evalcheck_evaluate_claims(hal, evalcheck_eval_claims(n_claims, claim_desc, d_columns), from_raw(point_pool, pool_len),
		                                                              FSliceMut{d_scratch, (size_t)scratch_elems});
		if (!out.evals.empty()) to_raw(out.evals, evals_out);
		if (phase_ms_out)
			for (int i = 0; i < EvalcheckEvaluateOutput::NPhases; i++) phase_ms_out[i] = out.phase_ms[i];
		return 0;
	});
}

// batch_zerocheck::batch_prove (crates/core/src/protocols/sumcheck/prove/batch_zerocheck.rs:166-293) through the C++ mirror
// binius_amd/host/zerocheck.hpp; the arguments are described in include/binius_amd_host.h.
uint64_t bnh_zerocheck_batch_scratch_elems(uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols)
{
	std::vector<size_t> nv, nc;
	for (uint32_t p = 0; p < n_tables; p++) {
		if (n_vars[p] > BN_PE_MAX_VARS + 8) return 0;
		nv.push_back(n_vars[p]);
		nc.push_back(n_cols[p]);
	}
	return zerocheck_batch_scratch_elems(nv, nc, skip_rounds);
}

static int zerocheck_batch_prove_c(bn_ctx *ctx, uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols, const void *const *d_cols,
                              const uint32_t *tower_levels, const uint32_t *n_comps, const bn_step *steps, const uint32_t *n_steps, const bn_step *steps_inf,
                              const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *zerocheck_challenges, const bn_f128 *batch_coeffs,
                              const bn_f128 *univariate_challenge, const bn_f128 *sumcheck_challenges, const bn_f128 *reduction_batch_coeff,
                              const bn_f128 *reduction_challenges, void *d_scratch, uint64_t scratch_elems, bn_f128 *message_out, bn_f128 *round_coeffs_out,
                              bn_f128 *final_evals_out, bn_f128 *reduction_round_coeffs_out, bn_f128 *reduction_final_evals_out, bn_f128 *skipped_challenges_out,
                              bn_f128 *unskipped_challenges_out, bn_f128 *concat_multilinear_evals_out, double *phase_ms_out, uint64_t *phase_calls_out, bool tower,
                              bool is_live = false, const bnh_transcript *transcript = nullptr)
{
	return guarded([&]() -> int {
		EntryTranscript et(is_live, transcript);
		if (!ctx || !n_tables || !n_vars || !n_cols || !n_comps || (!is_live && (!batch_coeffs || !univariate_challenge || !reduction_batch_coeff || !reduction_challenges)) || !final_evals_out ||
		    !reduction_round_coeffs_out || !reduction_final_evals_out || !skipped_challenges_out || !concat_multilinear_evals_out || (!d_scratch && scratch_elems))
			throw Error(Error::InputValidation, "null argument");
		if (skip_rounds < 1 || skip_rounds > 8) throw Error(Error::InputValidation, "zerocheck: skip_rounds out of range (1 .. 8)");
		// (what the conversion below relies on is checked here; the mirror checks the rest before its first launch)
		size_t max_n = 0, total_cols = 0, total_comps = 0;
		for (uint32_t p = 0; p < n_tables; p++) {
			if (n_vars[p] > BN_PE_MAX_VARS) throw Error(Error::InputValidation, "zerocheck: n_vars out of range");
			if (p && n_vars[p] < n_vars[p - 1]) throw Error(Error::InputValidation, "ClaimsOutOfOrder: tables ascend by number of variables");
			max_n = n_vars[p];
			total_cols += n_cols[p];
			total_comps += n_comps[p];
		}
		if (skip_rounds > max_n) throw Error(Error::InputValidation, "IncorrectSkippedRoundsCount: skip_rounds exceeds the largest n_vars");
		if ((total_cols && (!d_cols || !tower_levels)) || (total_comps && (!steps || !n_steps || !steps_inf || !n_steps_inf || !degrees)))
			throw Error(Error::InputValidation, "null argument");
		const size_t rounds = max_n - skip_rounds;
		if (rounds && ((!is_live && (!zerocheck_challenges || !sumcheck_challenges)) || !round_coeffs_out || !unskipped_challenges_out)) throw Error(Error::InputValidation, "null argument");
		ComputeLayer hal(ctx);
		std::vector<ZerocheckTable> tables(n_tables);
		size_t at_col = 0, at_comp = 0, at_step = 0, at_inf = 0;
		for (uint32_t p = 0; p < n_tables; p++) {
			ZerocheckTable &t = tables[p];
			t.n_vars = n_vars[p];
			for (uint32_t c = 0; c < n_cols[p]; c++, at_col++) t.columns.push_back(ZerocheckColumn{d_cols[at_col], tower_levels[at_col]});
			for (uint32_t c = 0; c < n_comps[p]; c++, at_comp++) {
				if (degrees[at_comp] < 1 || ((uint64_t)degrees[at_comp] << skip_rounds) > 256)
					throw Error(Error::InputValidation, "zerocheck: a composition's degree d needs 1 <= d and d 2^k <= 256");
				t.base_compositions.emplace_back(steps + at_step, steps + at_step + n_steps[at_comp]);
				EqIndComposition ec;
				ec.composition = hal.compile_expr(ArithCircuit::from_steps(t.base_compositions.back()));
				ec.composition_at_infinity = hal.compile_expr(ArithCircuit::from_steps(std::vector<bn_step>(steps_inf + at_inf, steps_inf + at_inf + n_steps_inf[at_comp])));
				ec.degree = degrees[at_comp];
				t.compositions.push_back(ec);
				at_step += n_steps[at_comp];
				at_inf += n_steps_inf[at_comp];
			}
		}
		TranscriptSource &tr = et.source({from_raw(zerocheck_challenges, rounds), from_raw(batch_coeffs, n_tables), one_sample(univariate_challenge),
		                                  from_raw(sumcheck_challenges, rounds), one_sample(reduction_batch_coeff), from_raw(reduction_challenges, skip_rounds)});
		const ZerocheckBatchOutput out = zerocheck_batch_prove(hal, tables, skip_rounds, tr, FSliceMut{d_scratch, (size_t)scratch_elems}, tower);
		auto put = [](bn_f128 *dst, const std::vector<B128> &v) { return to_raw(v, dst); };
		if (!out.message.empty()) {
			if (!message_out) throw Error(Error::InputValidation, "null argument");
			put(message_out, out.message);
		}
		bn_f128 *at = round_coeffs_out;
		for (const auto &rc : out.round_coeffs) at = put(at, rc);
		at = final_evals_out;
		for (const auto &fe : out.final_evals) at = put(at, fe);
		at = reduction_round_coeffs_out;
		for (const auto &rc : out.reduction_round_coeffs) at = put(at, rc);
		put(reduction_final_evals_out, out.reduction_final_evals);
		put(skipped_challenges_out, out.skipped_challenges);
		if (rounds) put(unskipped_challenges_out, out.unskipped_challenges);
		put(concat_multilinear_evals_out, out.concat_multilinear_evals);
		for (int i = 0; i < ZerocheckBatchOutput::NPhases; i++) {
			if (phase_ms_out) phase_ms_out[i] = out.phase_ms[i];
			if (phase_calls_out) phase_calls_out[i] = out.phase_calls[i];
		}
		return 0;
	});
}

int bnh_zerocheck_batch_prove(bn_ctx *ctx, uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols, const void *const *d_cols,
                              const uint32_t *tower_levels, const uint32_t *n_comps, const bn_step *steps, const uint32_t *n_steps, const bn_step *steps_inf,
                              const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *zerocheck_challenges, const bn_f128 *batch_coeffs,
                              const bn_f128 *univariate_challenge, const bn_f128 *sumcheck_challenges, const bn_f128 *reduction_batch_coeff,
                              const bn_f128 *reduction_challenges, void *d_scratch, uint64_t scratch_elems, bn_f128 *message_out, bn_f128 *round_coeffs_out,
                              bn_f128 *final_evals_out, bn_f128 *reduction_round_coeffs_out, bn_f128 *reduction_final_evals_out, bn_f128 *skipped_challenges_out,
                              bn_f128 *unskipped_challenges_out, bn_f128 *concat_multilinear_evals_out, double *phase_ms_out, uint64_t *phase_calls_out)
{
	return zerocheck_batch_prove_c(ctx, n_tables, skip_rounds, n_vars, n_cols, d_cols, tower_levels, n_comps, steps, n_steps, steps_inf, n_steps_inf, degrees, zerocheck_challenges,
	                              batch_coeffs, univariate_challenge, sumcheck_challenges, reduction_batch_coeff, reduction_challenges, d_scratch, scratch_elems, message_out,
	                              round_coeffs_out, final_evals_out, reduction_round_coeffs_out, reduction_final_evals_out, skipped_challenges_out,
	                              unskipped_challenges_out, concat_multilinear_evals_out, phase_ms_out, phase_calls_out, false);
}

// the same prover for every arm of constraint_system/prove.rs:483-490: columns at level 0 or 3 .. 7, constants anywhere in B128
uint64_t bnh_zerocheck_batch_scratch_elems_tower(uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols, const uint32_t *tower_levels)
{
	std::vector<size_t> nv;
	std::vector<std::vector<uint32_t>> levels;
	size_t at = 0;
	for (uint32_t p = 0; p < n_tables; p++) {
		if (n_vars[p] > BN_PE_MAX_VARS + 8) return 0;
		nv.push_back(n_vars[p]);
		levels.emplace_back();
		for (uint32_t c = 0; c < n_cols[p]; c++, at++) {
			if (tower_levels[at] > 7) return 0;
			levels.back().push_back(tower_levels[at]);
		}
	}
	return zerocheck_batch_scratch_elems_tower(nv, levels, skip_rounds);
}

int bnh_zerocheck_batch_prove_tower(bn_ctx *ctx, uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols, const void *const *d_cols,
                                    const uint32_t *tower_levels, const uint32_t *n_comps, const bn_step *steps, const uint32_t *n_steps, const bn_step *steps_inf,
                                    const uint32_t *n_steps_inf, const uint32_t *degrees, const bn_f128 *zerocheck_challenges, const bn_f128 *batch_coeffs,
                                    const bn_f128 *univariate_challenge, const bn_f128 *sumcheck_challenges, const bn_f128 *reduction_batch_coeff,
                                    const bn_f128 *reduction_challenges, void *d_scratch, uint64_t scratch_elems, bn_f128 *message_out, bn_f128 *round_coeffs_out,
                                    bn_f128 *final_evals_out, bn_f128 *reduction_round_coeffs_out, bn_f128 *reduction_final_evals_out, bn_f128 *skipped_challenges_out,
                                    bn_f128 *unskipped_challenges_out, bn_f128 *concat_multilinear_evals_out, double *phase_ms_out, uint64_t *phase_calls_out)
{
	return zerocheck_batch_prove_c(ctx, n_tables, skip_rounds, n_vars, n_cols, d_cols, tower_levels, n_comps, steps, n_steps, steps_inf, n_steps_inf, degrees, zerocheck_challenges,
	                              batch_coeffs, univariate_challenge, sumcheck_challenges, reduction_batch_coeff, reduction_challenges, d_scratch, scratch_elems, message_out,
	                              round_coeffs_out, final_evals_out, reduction_round_coeffs_out, reduction_final_evals_out, skipped_challenges_out,
	                              unskipped_challenges_out, concat_multilinear_evals_out, phase_ms_out, phase_calls_out, true);
}

int bnh_zerocheck_batch_prove_tower_live(bn_ctx *ctx, uint32_t n_tables, uint32_t skip_rounds, const uint32_t *n_vars, const uint32_t *n_cols, const void *const *d_cols,
                                         const uint32_t *tower_levels, const uint32_t *n_comps, const bn_step *steps, const uint32_t *n_steps, const bn_step *steps_inf,
                                         const uint32_t *n_steps_inf, const uint32_t *degrees, const bnh_transcript *transcript, void *d_scratch, uint64_t scratch_elems,
                                         bn_f128 *message_out, bn_f128 *round_coeffs_out, bn_f128 *final_evals_out, bn_f128 *reduction_round_coeffs_out,
                                         bn_f128 *reduction_final_evals_out, bn_f128 *skipped_challenges_out, bn_f128 *unskipped_challenges_out,
                                         bn_f128 *concat_multilinear_evals_out, double *phase_ms_out, uint64_t *phase_calls_out)
{
	return zerocheck_batch_prove_c(ctx, n_tables, skip_rounds, n_vars, n_cols, d_cols, tower_levels, n_comps, steps, n_steps, steps_inf, n_steps_inf, degrees, nullptr, nullptr,
	                              nullptr, nullptr, nullptr, nullptr, d_scratch, scratch_elems, message_out, round_coeffs_out, final_evals_out, reduction_round_coeffs_out,
	                              reduction_final_evals_out, skipped_challenges_out, unskipped_challenges_out, concat_multilinear_evals_out, phase_ms_out, phase_calls_out, true,
	                              true, transcript);
}

// ring_switch::prove (crates/core/src/ring_switch/prove.rs:42-144) through the C++ mirror binius_amd/host/ring_switch.hpp; the arguments
// are described in include/binius_amd_host.h.
namespace {
void ring_switch_descs(uint32_t n_suffixes, const uint32_t *suffix_desc, uint32_t n_claims, const uint32_t *claim_desc, std::vector<RingSwitchSuffix> &suffixes,
                       std::vector<RingSwitchClaim> &claims)
{
	for (uint32_t i = 0; i < n_suffixes; i++) suffixes.push_back(RingSwitchSuffix{suffix_desc[3 * i], suffix_desc[3 * i + 1], suffix_desc[3 * i + 2]});
	for (uint32_t i = 0; i < n_claims; i++) claims.push_back(RingSwitchClaim{claim_desc[3 * i], claim_desc[3 * i + 1], claim_desc[3 * i + 2]});
}
} // namespace

uint64_t bnh_ring_switch_scratch_elems(uint32_t n_suffixes, const uint32_t *suffix_desc, uint32_t n_claims, const uint32_t *claim_desc)
{
	if ((n_suffixes && !suffix_desc) || (n_claims && !claim_desc)) return 0;
	std::vector<RingSwitchSuffix> suffixes;
	std::vector<RingSwitchClaim> claims;
	ring_switch_descs(n_suffixes, suffix_desc, n_claims, claim_desc, suffixes, claims);
	try {
		return ring_switch_scratch_elems(suffixes, claims);
	} catch (const Error &) {
		return 0;
	}
}

static int ring_switch_prove_body(bn_ctx *ctx, uint32_t n_columns, const void *const *d_columns, const uint32_t *column_desc, const bn_f128 *point_pool, uint32_t pool_len,
                          uint32_t n_suffixes, const uint32_t *suffix_desc, uint32_t n_prefixes, const uint32_t *prefix_kappas, uint32_t n_claims,
                          const uint32_t *claim_desc, const bn_f128 *mixing_challenges, uint32_t n_mixing_challenges, const bn_f128 *row_batch_challenges,
                          uint32_t n_row_batch_challenges, void *d_scratch, uint64_t scratch_elems, bn_f128 *mixed_tensor_elems_out, bn_f128 *row_batched_evals_out,
                          void **d_transparents_out, double *phase_ms_out, bool is_live, const bnh_transcript *transcript)
{
	return guarded([&]() -> int {
		EntryTranscript et(is_live, transcript);
		if (!ctx || (n_columns && (!d_columns || !column_desc)) || (pool_len && !point_pool) || (n_suffixes && !suffix_desc) || (n_prefixes && (!prefix_kappas || !mixed_tensor_elems_out)) ||
		    (n_claims && (!claim_desc || !row_batched_evals_out || !d_transparents_out)) || (n_mixing_challenges && !mixing_challenges) ||
		    (n_row_batch_challenges && !row_batch_challenges) || (!d_scratch && scratch_elems))
			throw Error(Error::InputValidation, "null argument");
		std::vector<bn_pe_column> columns;
		for (uint32_t c = 0; c < n_columns; c++) columns.push_back(bn_pe_column{d_columns[c], column_desc[2 * c], column_desc[2 * c + 1]});
		std::vector<RingSwitchSuffix> suffixes;
		std::vector<RingSwitchClaim> claims;
		ring_switch_descs(n_suffixes, suffix_desc, n_claims, claim_desc, suffixes, claims);
		ComputeLayer hal(ctx);
		TranscriptSource &tr = et.source({from_raw(mixing_challenges, n_mixing_challenges), from_raw(row_batch_challenges, n_row_batch_challenges)});
		const RingSwitchOutput out = ring_switch_prove(hal, columns, from_raw(point_pool, pool_len), suffixes, std::vector<uint32_t>(prefix_kappas, prefix_kappas + n_prefixes), claims,
		                                               tr, FSliceMut{d_scratch, (size_t)scratch_elems}, is_live ? -1 : (long)n_mixing_challenges,
		                                               is_live ? -1 : (long)n_row_batch_challenges);
		if (!out.mixed_tensor_elems.empty()) to_raw(out.mixed_tensor_elems, mixed_tensor_elems_out);
		if (!out.row_batched_evals.empty()) to_raw(out.row_batched_evals, row_batched_evals_out);
		for (size_t i = 0; i < out.transparents.size(); i++) d_transparents_out[i] = const_cast<void *>(out.transparents[i].ptr);
		if (phase_ms_out)
			for (int i = 0; i < RingSwitchOutput::NPhases; i++) phase_ms_out[i] = out.phase_ms[i];
		return 0;
	});
}

int bnh_ring_switch_prove(bn_ctx *ctx, uint32_t n_columns, const void *const *d_columns, const uint32_t *column_desc, const bn_f128 *point_pool, uint32_t pool_len,
                          uint32_t n_suffixes, const uint32_t *suffix_desc, uint32_t n_prefixes, const uint32_t *prefix_kappas, uint32_t n_claims,
                          const uint32_t *claim_desc, const bn_f128 *mixing_challenges, uint32_t n_mixing_challenges, const bn_f128 *row_batch_challenges,
                          uint32_t n_row_batch_challenges, void *d_scratch, uint64_t scratch_elems, bn_f128 *mixed_tensor_elems_out, bn_f128 *row_batched_evals_out,
                          void **d_transparents_out, double *phase_ms_out)
{
	return ring_switch_prove_body(ctx, n_columns, d_columns, column_desc, point_pool, pool_len, n_suffixes, suffix_desc, n_prefixes, prefix_kappas, n_claims, claim_desc,
	                              mixing_challenges, n_mixing_challenges, row_batch_challenges, n_row_batch_challenges, d_scratch, scratch_elems, mixed_tensor_elems_out,
	                              row_batched_evals_out, d_transparents_out, phase_ms_out, false, nullptr);
}

int bnh_ring_switch_prove_live(bn_ctx *ctx, uint32_t n_columns, const void *const *d_columns, const uint32_t *column_desc, const bn_f128 *point_pool, uint32_t pool_len,
                               uint32_t n_suffixes, const uint32_t *suffix_desc, uint32_t n_prefixes, const uint32_t *prefix_kappas, uint32_t n_claims,
                               const uint32_t *claim_desc, const bnh_transcript *transcript, void *d_scratch, uint64_t scratch_elems, bn_f128 *mixed_tensor_elems_out,
                               bn_f128 *row_batched_evals_out, void **d_transparents_out, double *phase_ms_out)
{
	return ring_switch_prove_body(ctx, n_columns, d_columns, column_desc, point_pool, pool_len, n_suffixes, suffix_desc, n_prefixes, prefix_kappas, n_claims, claim_desc, nullptr,
	                              0, nullptr, 0, d_scratch, scratch_elems, mixed_tensor_elems_out, row_batched_evals_out, d_transparents_out, phase_ms_out, true, transcript);
}

// The virtual columns of a constraint system derived on the device through the C++ mirror binius_amd/host/witness.hpp; the arguments are
// described in include/binius_amd_host.h.
namespace {
// the expressions of bnh_witness_compute's BNH_WIT_COMPUTED columns: expression e is steps[step_off[e] .. step_off[e + 1]) over the
// columns expr_inputs[expr_input_off[e] .. expr_input_off[e + 1])
struct witness_exprs {
	const bn_step *steps = nullptr;
	const uint32_t *step_off = nullptr, *inputs = nullptr, *input_off = nullptr;
	uint32_t n_exprs = 0;
};
std::vector<WitnessColumn> witness_columns(uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                                           const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, const witness_exprs &ex = witness_exprs{})
{
	if (n_columns && (!col_desc || !col_args || !lc_offsets)) throw Error(Error::InputValidation, "null argument");
	if (n_lc_terms && (!lc_terms || !lc_coeffs)) throw Error(Error::InputValidation, "null argument");
	if (ex.n_exprs && (!ex.step_off || !ex.input_off)) throw Error(Error::InputValidation, "null argument");
	for (uint32_t e = 0; e < ex.n_exprs; e++) {
		if (ex.step_off[e + 1] < ex.step_off[e] || ex.input_off[e + 1] < ex.input_off[e]) throw Error(Error::InputValidation, "witness: expression offsets decrease");
		if ((ex.step_off[e + 1] > ex.step_off[e] && !ex.steps) || (ex.input_off[e + 1] > ex.input_off[e] && !ex.inputs)) throw Error(Error::InputValidation, "null argument");
	}
	std::vector<WitnessColumn> cols(n_columns);
	for (uint32_t i = 0; i < n_columns; i++) {
		const uint32_t *d = col_desc + 4 * i;
		WitnessColumn &c = cols[i];
		c.kind = d[0];
		switch (c.kind) {
		case WitnessColumn::Given:
			c.d_evals = d_given ? d_given[i] : reinterpret_cast<const void *>(16); // (the scratch formula reads no pointer)
			c.tower_level = d[1];
			c.n_vars = d[2];
			break;
		case WitnessColumn::Shifted:
			c.inner = d[1];
			c.block_size = d[2];
			c.shift_variant = d[3];
			c.shift_offset = col_args[i];
			break;
		case WitnessColumn::Repeating:
			c.inner = d[1];
			c.log_count = d[2];
			break;
		case WitnessColumn::ZeroPadded:
			c.inner = d[1];
			c.n_pad_vars = d[2];
			c.start_index = d[3];
			c.nonzero_index = col_args[i];
			break;
		case WitnessColumn::Packed:
			c.inner = d[1];
			c.log_degree = d[2];
			break;
		case WitnessColumn::LinearCombination:
			if (d[1] > n_lc_terms || d[2] > n_lc_terms - d[1]) throw Error(Error::InputValidation, "witness: a combination's terms leave the term list");
			c.terms.assign(lc_terms + d[1], lc_terms + d[1] + d[2]);
			c.coefficients = from_raw(lc_coeffs + d[1], d[2]);
			c.n_vars = d[3];
			c.offset = B128(lc_offsets[i].lo, lc_offsets[i].hi);
			break;
		case WitnessColumn::ProjectedBits:
			c.inner = d[1];
			c.start_index = d[2];
			c.query_size = d[3];
			c.query_bits = col_args[i];
			break;
		case WitnessColumn::Constant:
		case WitnessColumn::StepDown:
		case WitnessColumn::StepUp:
		case WitnessColumn::SelectRow:
		case WitnessColumn::Incrementing:
		case WitnessColumn::Powers:
			c.tower_level = d[1];
			c.n_vars = d[2];
			c.index = col_args[i];
			c.value = B128(lc_offsets[i].lo, lc_offsets[i].hi);
			break;
		case WitnessColumn::Computed:
			c.n_vars = d[2];
			c.tower_level = d[3];
			if (ex.step_off) { // (without expressions -- bnh_witness_derive / _build -- witness_shapes rejects the kind)
				if (d[1] >= ex.n_exprs) throw Error(Error::InputValidation, "witness: a computed column names an expression that is not there");
				c.steps.assign(ex.steps + ex.step_off[d[1]], ex.steps + ex.step_off[d[1] + 1]);
				c.inputs.assign(ex.inputs + ex.input_off[d[1]], ex.inputs + ex.input_off[d[1] + 1]);
			}
			break;
		default:
			break; // (witness_shapes rejects it)
		}
	}
	return cols;
}

int witness_run(bool generate, bn_ctx *ctx, uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, void *d_scratch, uint64_t scratch_elems, void **d_columns_out,
                uint32_t *tower_levels_out, uint32_t *n_vars_out, uint32_t *n_waves_out, uint32_t *n_launches_out, const witness_exprs *ex = nullptr, bool batched = false)
{
	return guarded([&]() -> int {
		if (!ctx || (n_columns && (!d_given || !d_columns_out || !tower_levels_out || !n_vars_out)) || (!d_scratch && scratch_elems))
			throw Error(Error::InputValidation, "null argument");
		const std::vector<WitnessColumn> cols = witness_columns(n_columns, col_desc, col_args, d_given, lc_terms, lc_coeffs, n_lc_terms, lc_offsets, ex ? *ex : witness_exprs{});
		ComputeLayer hal(ctx);
		const WitnessOutput out = witness_derive(hal, cols, FSliceMut{d_scratch, (size_t)scratch_elems}, generate, /*compute=*/ex != nullptr, batched);
		for (uint32_t i = 0; i < n_columns; i++) {
			d_columns_out[i] = const_cast<void *>(out.columns[i].ptr);
			tower_levels_out[i] = out.columns[i].tower_level;
			n_vars_out[i] = out.columns[i].n_vars;
		}
		if (n_waves_out) *n_waves_out = out.n_waves;
		if (n_launches_out) *n_launches_out = out.n_launches;
		return 0;
	});
}
} // namespace

uint64_t bnh_witness_derive_scratch_elems(uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const uint32_t *lc_terms, const bn_f128 *lc_coeffs,
                                          uint32_t n_lc_terms, const bn_f128 *lc_offsets)
{
	try {
		return witness_derive_scratch_elems(witness_columns(n_columns, col_desc, col_args, nullptr, lc_terms, lc_coeffs, n_lc_terms, lc_offsets));
	} catch (const Error &) {
		return 0;
	}
}

int bnh_witness_derive(bn_ctx *ctx, uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                       const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, void *d_scratch, uint64_t scratch_elems, void **d_columns_out,
                       uint32_t *tower_levels_out, uint32_t *n_vars_out, uint32_t *n_waves_out, uint32_t *n_launches_out)
{
	return witness_run(false, ctx, n_columns, col_desc, col_args, d_given, lc_terms, lc_coeffs, n_lc_terms, lc_offsets, d_scratch, scratch_elems, d_columns_out, tower_levels_out,
	                   n_vars_out, n_waves_out, n_launches_out);
}

uint64_t bnh_witness_build_scratch_elems(uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const uint32_t *lc_terms, const bn_f128 *lc_coeffs,
                                         uint32_t n_lc_terms, const bn_f128 *lc_offsets)
{
	try {
		return witness_build_scratch_elems(witness_columns(n_columns, col_desc, col_args, nullptr, lc_terms, lc_coeffs, n_lc_terms, lc_offsets));
	} catch (const Error &) {
		return 0;
	}
}

int bnh_witness_build(bn_ctx *ctx, uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                      const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, void *d_scratch, uint64_t scratch_elems, void **d_columns_out,
                      uint32_t *tower_levels_out, uint32_t *n_vars_out, uint32_t *n_waves_out, uint32_t *n_launches_out)
{
	return witness_run(true, ctx, n_columns, col_desc, col_args, d_given, lc_terms, lc_coeffs, n_lc_terms, lc_offsets, d_scratch, scratch_elems, d_columns_out, tower_levels_out,
	                   n_vars_out, n_waves_out, n_launches_out);
}

uint64_t bnh_witness_compute_scratch_elems(uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const uint32_t *lc_terms, const bn_f128 *lc_coeffs,
                                           uint32_t n_lc_terms, const bn_f128 *lc_offsets, const bn_step *steps, const uint32_t *step_off, const uint32_t *expr_inputs,
                                           const uint32_t *expr_input_off, uint32_t n_exprs)
{
	try {
		const uint32_t zero[2] = {0, 0}; // (no expressions: empty offset tables of our own, so that the kind is known and its index checked)
		const witness_exprs ex{steps, n_exprs ? step_off : zero, expr_inputs, n_exprs ? expr_input_off : zero, n_exprs};
		return witness_compute_scratch_elems(witness_columns(n_columns, col_desc, col_args, nullptr, lc_terms, lc_coeffs, n_lc_terms, lc_offsets, ex));
	} catch (const Error &) {
		return 0;
	}
}

int bnh_witness_compute(bn_ctx *ctx, uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                        const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, void *d_scratch, uint64_t scratch_elems, void **d_columns_out,
                        uint32_t *tower_levels_out, uint32_t *n_vars_out, uint32_t *n_waves_out, uint32_t *n_launches_out, const bn_step *steps, const uint32_t *step_off,
                        const uint32_t *expr_inputs, const uint32_t *expr_input_off, uint32_t n_exprs)
{
	const uint32_t zero[2] = {0, 0};
	const witness_exprs ex{steps, n_exprs ? step_off : zero, expr_inputs, n_exprs ? expr_input_off : zero, n_exprs};
	return witness_run(true, ctx, n_columns, col_desc, col_args, d_given, lc_terms, lc_coeffs, n_lc_terms, lc_offsets, d_scratch, scratch_elems, d_columns_out, tower_levels_out,
	                   n_vars_out, n_waves_out, n_launches_out, &ex);
}

int bnh_witness_compute_batched(bn_ctx *ctx, uint32_t n_columns, const uint32_t *col_desc, const uint64_t *col_args, const void *const *d_given, const uint32_t *lc_terms,
                                const bn_f128 *lc_coeffs, uint32_t n_lc_terms, const bn_f128 *lc_offsets, void *d_scratch, uint64_t scratch_elems, void **d_columns_out,
                                uint32_t *tower_levels_out, uint32_t *n_vars_out, uint32_t *n_waves_out, uint32_t *n_launches_out, const bn_step *steps, const uint32_t *step_off,
                                const uint32_t *expr_inputs, const uint32_t *expr_input_off, uint32_t n_exprs)
{
	const uint32_t zero[2] = {0, 0};
	const witness_exprs ex{steps, n_exprs ? step_off : zero, expr_inputs, n_exprs ? expr_input_off : zero, n_exprs};
	return witness_run(true, ctx, n_columns, col_desc, col_args, d_given, lc_terms, lc_coeffs, n_lc_terms, lc_offsets, d_scratch, scratch_elems, d_columns_out, tower_levels_out,
	                   n_vars_out, n_waves_out, n_launches_out, &ex, /*batched=*/true);
}

} // extern "C"
