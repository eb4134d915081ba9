// binius_amd/host/sharded_sumcheck.hpp -- the bivariate-product sumcheck of sumcheck.hpp with the hypercube sharded over the ranks
// of a world (one process per GPU; rank g owns the global indices = g mod world: High-to-Low binding, the shard id sits in the
// variables bound last).
//
//   RoundExchange                     what a transport decides, and nothing else: where a local round's {y_1, y_inf} lands,
//                                     how the world's partials are combined, how (and whether) the residual instance is rebuilt
//   CallbackExchange, ShmExchange,    three of the four transports (the RCCL one lives next to its run-time binding in
//   PeerExchange                      host_capi.cpp, as does the function that chooses among the four)
//   ShardedBivariateSumcheckProver    execute / fold / finish over BivariateRoundCore, and run_residual: once every rank is down
//                                     to one element per multilinear, the last log2(world) rounds on the gathered residual instance
//
// The local rounds of a rank are the single-GPU prover's, call for call; only the round evaluations pass through the exchange.
#pragma once

#include <atomic>

#include "../../include/binius_amd_host.h"
#include "sumcheck.hpp"

namespace binius_amd {

class RoundExchange {
public:
	virtual ~RoundExchange() = default;
	// where this rank's {y_1, y_inf} of a local round lands: at this device address, or (null) in the host's mailbox
	virtual void *device_partial() const { return nullptr; }
	// the world's {y_1, y_inf} of a local round; `local`: this rank's from the host's mailbox, empty with a device_partial()
	virtual std::vector<B128> combine(const std::vector<B128> &local) = 0;
	// the last local round is folded: called once, before the residual gather or the final copies (the peer exchange goes off
	// here, where bn_peer_set_active(0) has always stood in the call sequence)
	virtual void end_local_rounds() {}
	// the residual multilinears, `world` elements each (index = rank), read-only, from the element every multilinear of this rank
	// has come down to; none: this transport rebuilds no residual instance
	virtual std::vector<FSlice> gather_residual(ComputeLayer &, DeviceBumpAllocator &, const std::vector<FSlice> & /*finals*/) { return {}; }
};

// callback: the partial stays on the device, the caller's reduce combines; no residual instance
class CallbackExchange : public RoundExchange {
public:
	CallbackExchange(bnh_round_reduce_fn reduce, void *user, void *d_partial) : reduce_(reduce), user_(user), d_partial_(d_partial) {}
	void *device_partial() const override { return d_partial_; }
	std::vector<B128> combine(const std::vector<B128> &) override
	{
		bn_f128 ev[2];
		if (reduce_(user_, d_partial_, ev)) throw Error(Error::CoreLibError, "round reduce callback failed");
		return from_raw(ev, 2);
	}

private:
	bnh_round_reduce_fn reduce_;
	void *user_, *d_partial_;
};

// shm: the device side of a round is the single-GPU one (result through the mailbox); the ranks' partials meet in the host's
// shared-memory segment (bnh_shm_allgather)
class ShmExchange : public RoundExchange {
public:
	ShmExchange(bn_ctx *ctx, void *shm, int world) : ctx_(ctx), shm_(shm), world_(world) {}
	std::vector<B128> combine(const std::vector<B128> &local) override
	{
		const uint64_t mine[4] = {local[0].raw().lo, local[0].raw().hi, local[1].raw().lo, local[1].raw().hi};
		const std::vector<uint64_t> all = allgather(mine, 4);
		bn_f128 ev[2] = {{0, 0}, {0, 0}};
		for (int w = 0; w < world_; w++) {
			ev[0].lo ^= all[4 * w + 0];
			ev[0].hi ^= all[4 * w + 1];
			ev[1].lo ^= all[4 * w + 2];
			ev[1].hi ^= all[4 * w + 3];
		}
		return from_raw(ev, 2);
	}
	// One exchange per three multilinears (a slot holds seven words) rebuilds the residual multilinears in the context's pinned,
	// device-visible scratch: no upload, and the rounds on them fold into device scratch.
	std::vector<FSlice> gather_residual(ComputeLayer &hal, DeviceBumpAllocator &, const std::vector<FSlice> &finals) override
	{
		const uint32_t m = (uint32_t)finals.size();
		std::vector<B128> fin(m);
		for (uint32_t j = 0; j < m; j++) hal.copy_d2h(finals[j], &fin[j], 1);
		void *h_scr = nullptr, *d_scr = nullptr;
		uint64_t scr_elems = 0;
		check(bn_host_scratch(ctx_, &h_scr, &d_scr, &scr_elems));
		if ((uint64_t)m * world_ > scr_elems) throw Error(Error::InputValidation, "residual instance does not fit the pinned scratch");
		bn_f128 *res = (bn_f128 *)h_scr;
		for (uint32_t j0 = 0; j0 < m; j0 += 3) {
			const uint32_t nj = (m - j0) < 3 ? (m - j0) : 3;
			uint64_t mine[6];
			for (uint32_t j = 0; j < nj; j++) {
				mine[2 * j] = fin[j0 + j].raw().lo;
				mine[2 * j + 1] = fin[j0 + j].raw().hi;
			}
			const std::vector<uint64_t> all = allgather(mine, 2 * nj);
			for (int w = 0; w < world_; w++)
				for (uint32_t j = 0; j < nj; j++) res[(size_t)(j0 + j) * world_ + w] = bn_f128{all[(size_t)w * 2 * nj + 2 * j], all[(size_t)w * 2 * nj + 2 * j + 1]};
		}
		std::atomic_thread_fence(std::memory_order_seq_cst);
		std::vector<FSlice> out;
		for (uint32_t j = 0; j < m; j++) out.push_back(FSlice{(char *)d_scr + (size_t)j * world_ * sizeof(bn_f128), (size_t)world_});
		return out;
	}

protected:
	bn_ctx *ctx_;

private:
	std::vector<uint64_t> allgather(const uint64_t *mine, uint32_t n_words)
	{
		std::vector<uint64_t> all((size_t)n_words * world_);
		if (bnh_shm_allgather(shm_, mine, n_words, all.data())) throw Error(Error::DeviceError, bnh_last_error());
		return all;
	}
	void *shm_;
	int world_;
};

// peer: the ranks' partials are XORed on the devices, inside the kernels' finalize step (bn_peer_*; the context must be connected),
// and the host finds the world's {y_1, y_inf} in its own mailbox.  From the launch after which the library holds the arrays on the
// host (bn_host_tail_active; every rank sees it after the same launch: the shards have the same size) the rounds' LOCAL partials
// come back from host arithmetic and meet in the shared-memory segment, which also carries the residual instance.
class PeerExchange : public ShmExchange {
public:
	PeerExchange(bn_ctx *ctx, void *shm, int world) : ShmExchange(ctx, shm, world), scope_{ctx}
	{
		if (!shm) throw Error(Error::InputValidation, "the peer exchange needs the shared-memory segment for the residual instance");
		check(bn_host_tail_allow_peer(ctx, 1)); // (the host rounds' partials are exchanged here, through the segment)
		scope_.set(true);
	}
	std::vector<B128> combine(const std::vector<B128> &local) override
	{
		if (host_rounds_) return ShmExchange::combine(local);
		int active = 0;
		check(bn_host_tail_active(ctx_, &active));
		if (active) {
			host_rounds_ = true;
			scope_.set(false);
		}
		return local;
	}
	void end_local_rounds() override { scope_.set(false); }

private:
	struct Scope { // local rounds reduced on the devices, everything else local; restored on every exit
		bn_ctx *c;
		bool on = false;
		void set(bool v)
		{
			if (v != on) {
				if (bn_peer_set_active(c, v ? 1 : 0) != 0) throw Error(Error::DeviceError, bn_last_error());
				on = v;
			}
		}
		~Scope()
		{
			if (on) (void)bn_peer_set_active(c, 0);
			(void)bn_host_tail_allow_peer(c, 0);
		}
	} scope_;
	bool host_rounds_ = false;
};

class ShardedBivariateSumcheckProver : public BivariateRoundCore {
public:
	// open_exchange() -> std::unique_ptr<RoundExchange>: called once the compositions are compiled, so that a transport that
	// changes the context's settings (the peer exchange) does so after the last bn_expr_compile, as the C entry always has
	template <class OpenExchange>
	ShardedBivariateSumcheckProver(ComputeLayer &hal, DeviceBumpAllocator &dev_alloc, HostBumpAllocator &host_alloc, size_t n_vars,
	                               const std::vector<IndexCompositionBivariate> &compositions, const std::vector<B128> &sums,
	                               const std::vector<FSlice> &multilins, OpenExchange &&open_exchange)
	    : BivariateRoundCore(hal, dev_alloc, host_alloc, n_vars, sums, multilins)
	{
		for (const auto &c : compositions) evaluators_.push_back(hal.compile_expr(c.expression()));
		exchange_ = open_exchange();
	}

	// a local round's evaluations are the world's, through the exchange; a residual round's are the same on every rank
	std::vector<B128> execute(B128 batch_coeff)
	{
		const B128 sum = batched_sum(batch_coeff);
		std::vector<B128> evals;
		if (!local_) {
			evals = round_evals(batch_coeff);
		} else if (void *d_partial = exchange_->device_partial()) {
			calculate_round_evals_to_device(hal_, n_vars_remaining_, batch_coeff, current(), evaluators_, d_partial);
			evals = exchange_->combine({});
		} else {
			evals = exchange_->combine(round_evals(batch_coeff));
		}
		const std::vector<B128> round_coeffs = calculate_round_coeffs_from_evals(sum, evals);
		set_coeffs(round_coeffs);
		return round_coeffs;
	}
	void fold(B128 challenge) { fold_multilinears(challenge); }

	// After the local rounds: the world's last elements become the residual instance (one multilinear of `world` elements per
	// multilinear, the same on every rank), and the rounds over its challenges.size() = log2(world) variables run with no
	// exchange.  Returns their round polynomials; none when the transport rebuilds no residual instance.
	std::vector<std::vector<B128>> run_residual(B128 batch_coeff, const std::vector<B128> &challenges)
	{
		leave_local_rounds();
		const std::vector<FSlice> residual = exchange_->gather_residual(hal_, dev_alloc_, current());
		std::vector<std::vector<B128>> round_proofs;
		if (residual.empty()) return round_proofs;
		reseat(challenges.size(), residual);
		for (const B128 &z : challenges) {
			round_proofs.push_back(execute(batch_coeff));
			fold(z);
		}
		return round_proofs;
	}

	std::vector<B128> finish()
	{
		leave_local_rounds();
		return final_evals();
	}

private:
	std::vector<FSlice> current() const
	{
		std::vector<FSlice> mls;
		for (const auto &m : multilins()) mls.push_back(ComputeMemory::as_const(m.evals));
		return mls;
	}
	void leave_local_rounds()
	{
		if (local_) exchange_->end_local_rounds();
		local_ = false;
	}
	std::unique_ptr<RoundExchange> exchange_;
	bool local_ = true;
};

} // namespace binius_amd
