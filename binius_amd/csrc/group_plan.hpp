// binius_amd/csrc/group_plan.hpp -- what a launch of kernels_group.hip is made of, decided on the host: the job table's layout
// and the PLANNER that deals the workgroups of one launch out to the jobs.  Host-only (no HIP include): the launcher
// (kernels_group.hip launch_group) plans and then launches; tests/cpp/group_plan_dump.cpp plans and prints (tests/test_group_plan.py).
//
// The workgroups go to the UNITS of the job list -- a job with its chain (jobs[i].chain followers directly behind it), or a lone
// job -- in proportion to their traffic, eight at a time where a unit gets at least eight so that its tiles keep the XCD-aware
// order; the table is sorted by first workgroup.  jobs[i].slot is the caller's; wg_begin / wg_count are filled in here.  Every
// job: n >= 1; all jobs of a chain: the same n; kind 0 / 3 / 4 jobs write out[] (2 n elements each).
//
// PACKED launches.  With more units than a launch has workgroups to give each a sensible share (a prover of the keccak width: a
// hundred claims and more, piop/prove.rs:262-287), the units are packed into U super-units of n_cu / U workgroups each, U a power
// of two: every workgroup of a super-unit runs ALL its jobs one after the other, each job on the workgroup's share of that
// job's tiles -- the chain mechanism of the kernel, used for jobs that do not depend on each other (chains that do stay whole
// and in order inside one super-unit).  Against one unit per job this costs a parity reduction per job and workgroup (~2 us) and
// buys (1) any number of jobs per launch, (2) balance -- 100 equal jobs on 256 workgroups are 2.56 workgroups each, i.e. 78 % of the
// chip busy; as 4 super-units of 25 jobs on 64 workgroups they are 100 % --, (3) the XCD-aware tile order (ranges in multiples of
// eight), and (4) every workgroup of the chip walks the jobs in the same order, so that an array shared by many claims (a
// transparent against every committed column) is re-read while it is still in the Infinity Cache.  U is chosen by a cost
// model (time per pair of tiles by job kind at the measured per-CU rate, fixed cost per job) over the longest super-unit.
//
// The order of every floating-point operation below is part of the behaviour (tests/golden/group_plans.json): decisions hang on
// comparisons of sums of doubles.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "gf128.hpp"

namespace bn {
constexpr int kGroupMaxJobs = 1024;  // jobs of one launch of kernels_group.hip (the table lives in pinned memory, not in the kernel arguments)
constexpr int kGroupMaxSlots = 1024; // accumulator slots of one launch: two per claim, the calling prover's and the riders'
constexpr int kGroupMaxGrid = 512;   // workgroups of one launch (the head-of-workgroup table in the kernel arguments)

struct group_job {
	const void *x0[2], *x1[2]; // kind 0: lower / upper half of the two arrays BEFORE the fold (2 n elements each); kind 1: lower half (evaluations
	                           // at 0) / upper half (evaluations at 1) of the two arrays as they are (n elements each)
	void *out[2];              // kind 0: where the folded arrays (2 n elements each) are written (may be x0)
	f128 z;                    // kind 0: the fold's challenge
	uint64_t n;                // evaluation points of the job
	uint32_t kind;             // 0 = fold + evaluate, 1 = evaluate, 2 = two plain inner products: rows x0[0] . x0[1] -> S[slot], x1[0] . x1[1] -> S[slot + 1] (x1 null: one),
	                           // 3 = fold only: arrays x0[sd] / x1[sd] -> out[sd] as kind 0, no sums (x0[1] null: one array)
	uint32_t slot;             // the job's sums are XORed into S[slot] (at 1) and S[slot + 1] (at infinity)
	uint32_t wg_begin, wg_count; // (filled in by the planner; wg_count = 0: a follower of the chain in front of it)
	uint32_t chain;            // the `chain` jobs that follow this one in the table are run by THIS job's workgroups, one after the other, each on
	                           // the tiles the workgroup had in this job (all jobs of a chain: the same n)
	uint32_t acquire;          // 1: the job reads what earlier jobs of its chain wrote (a workgroup reads back only its own tiles: its stores are
	                           // awaited and its vector cache invalidated first)
};
// (the kernel reads the table with scalar loads at these offsets: the layout is an interface)
static_assert(sizeof(group_job) == 96 && sizeof(void *) == 8, "group_job: 96 bytes");
static_assert(offsetof(group_job, n) == 64 && offsetof(group_job, kind) == 72 && offsetof(group_job, wg_begin) == 80 && offsetof(group_job, chain) == 88, "group_job layout");

constexpr uint32_t kGroupTilePoints = 256;  // points of a tile (gram.hpp kTP)
constexpr uint32_t kGroupWgTilesLog2 = 14;  // tiles of one job on one workgroup, at most: 2^22 points, the f32 counts stay exact

// ---- what the planner knows about a job by its kind (row 5: kind 3 with one array)
struct group_kind_facts {
	double weight;      // traffic per tile, relative (192 / 64 / 64 / 192 or 96 / 128 B per point)
	uint32_t elems;     // elements touched per point
	double pair_us;     // one pair of tiles (512 points) on one workgroup at ~ 5 TB/s / 256 CUs: microseconds
	double fixed_us;    // what a further job costs a workgroup besides its tiles: the pipeline of loads, staging and Gram steps drains and refills, the parity
	                    // words are reduced (measured: 50 equal jobs as 2 x 25 at 0.45 of the HBM peak against 0.52 for 64 jobs of 4 workgroups each)
};
constexpr group_kind_facts kGroupKindFacts[6] = {
	{3.0, 8, 5.0, 10.0}, {1.0, 4, 1.7, 10.0}, {1.0, 4, 1.7, 10.0}, {3.0, 6, 5.0, 3.0}, {2.0, 6, 3.4, 10.0}, {1.5, 3, 2.5, 3.0},
};
inline const group_kind_facts &group_facts(const group_job &j) { return kGroupKindFacts[j.kind == 3 && !j.x0[1] ? 5 : j.kind]; }

struct group_plan {
	enum status_t { ok, invalid, not_supported }; // (the launcher: hipSuccess, hipErrorInvalidValue, hipErrorNotSupported)
	status_t status = ok;
	uint32_t grid = 0;         // workgroups of the launch
	bool full = true;          // every job a whole number of tiles
	uint64_t total_elems = 0;  // elements the launch touches
	const group_job *table = nullptr; // n_jobs rows, sorted by first workgroup (the planner's memory: valid until it plans again)
	uint32_t n_jobs = 0;
	uint32_t head_of_wg[kGroupMaxGrid / 2] = {}; // the head job of every workgroup, two 16-bit job numbers per word
};
// streaming accesses once the launch's arrays cannot stay in the caches anyway: from 4 << nt_log2 elements touched
inline bool group_plan_streams(const group_plan &p, int nt_log2) { return p.full && nt_log2 < 62 && p.total_elems >= (4ull << nt_log2); }

// the units of a job list
struct group_unit {
	uint32_t first, len; // its jobs: [first, first + len)
	uint32_t tiles, cap; // tiles of each of its jobs; the most workgroups it can use (a workgroup wants a pair of tiles)
	double w;            // weight
};
struct group_units {
	std::vector<group_unit> u;
	double W = 0; // sum of the weights, in list order
	uint32_t max_tiles = 0;
	uint32_t size() const { return (uint32_t)u.size(); }
	const group_unit &operator[](uint32_t i) const { return u[i]; }
};

namespace group_plan_steps {
typedef group_plan::status_t status_t;
inline uint32_t wg_needed(uint32_t tiles) { return (tiles + (1u << kGroupWgTilesLog2) - 1) >> kGroupWgTilesLog2; } // the exactness bound

// ---- step 1: the units of the list, validated
inline status_t collect_units(const group_job *jobs, uint32_t n_jobs, uint32_t n_slots, int n_cu, group_units &un, group_plan &p)
{
	un.u.clear(); // (the memory stays: a planner's next list is as long as its last)
	un.W = 0;
	un.max_tiles = 0;
	for (uint32_t i = 0; i < n_jobs;) {
		const uint32_t l = 1 + jobs[i].chain;
		if (i + l > n_jobs) return group_plan::invalid;
		double wu = 0;
		const uint64_t nt = (jobs[i].n + kGroupTilePoints - 1) / kGroupTilePoints;
		for (uint32_t q = i; q < i + l; q++) {
			const group_job &j = jobs[q];
			if (j.n == 0 || j.kind > 4 || (j.kind != 3 && j.slot + 2 > n_slots) || j.n != jobs[i].n || (q > i && j.chain)) return group_plan::invalid;
			if (q == i && j.acquire) return group_plan::invalid; // (nothing in front of it to read back)
			if (j.n % kGroupTilePoints) p.full = false;
			wu += (double)nt * group_facts(j).weight;
			p.total_elems += j.n * group_facts(j).elems;
		}
		if (nt > (1ull << kGroupWgTilesLog2) * (uint64_t)n_cu) return group_plan::not_supported;
		un.u.push_back(group_unit{i, l, (uint32_t)nt, (uint32_t)(nt >= 2 ? nt / 2 : 1), wu});
		if ((uint32_t)nt > un.max_tiles) un.max_tiles = (uint32_t)nt;
		un.W += wu;
		i += l;
	}
	return group_plan::ok;
}

// the model: acc += what unit i costs each of `wgs` workgroups that share its tiles (job by job: the order of the sum is kept)
inline void add_unit_cost(double &acc, const group_job *jobs, const group_units &un, uint32_t i, uint32_t wgs)
{
	const uint64_t steps = ((uint64_t)un[i].tiles + 2 * wgs - 1) / (2 * wgs);
	for (uint32_t q = un[i].first; q < un[i].first + un[i].len; q++) acc += (double)steps * group_facts(jobs[q]).pair_us + group_facts(jobs[q]).fixed_us;
}

// ---- step 2: one unit per job by the model: every unit its proportional share of the workgroups, the longest one counts
inline double unpacked_cost(const group_job *jobs, const group_units &un, int n_cu)
{
	double worst = 0;
	for (uint32_t i = 0; i < un.size(); i++) {
		uint32_t c = (uint32_t)((double)n_cu * un[i].w / un.W);
		if (c < 1) c = 1;
		if (c > un[i].cap) c = un[i].cap;
		double cu = 0;
		add_unit_cost(cu, jobs, un, i, c);
		if (cu > worst) worst = cu;
	}
	return worst;
}

// ---- step 3a: U super-units of g = n_cu / U workgroups, U = 1, 2, 4, ...; units dealt out heaviest first to the least loaded
// super-unit; the U whose longest super-unit is shortest.  0: no U within the exactness bound.
inline uint32_t pack_sweep(const group_job *jobs, const group_units &un, int n_cu, const std::vector<uint32_t> &by_weight, double &best_cost, std::vector<uint32_t> &best_assign)
{
	const uint32_t n_units = un.size(), g_min = wg_needed(un.max_tiles);
	uint32_t best_U = 0;
	std::vector<uint32_t> assign(n_units);
	for (uint32_t U = 1; U <= (uint32_t)n_cu && U <= n_units; U <<= 1) {
		const uint32_t g = (uint32_t)n_cu / U;
		if (g < g_min || g == 0) break;
		std::vector<double> cost(U, 0.0);
		// (least loaded super-unit first: a heap -- a constraint set's request is hundreds of units)
		typedef std::pair<double, uint32_t> lu;
		std::priority_queue<lu, std::vector<lu>, std::greater<lu>> heap;
		for (uint32_t q = 0; q < U; q++) heap.push(lu{0.0, q});
		for (uint32_t o = 0; o < n_units; o++) {
			const uint32_t it = by_weight[o];
			const lu top = heap.top();
			heap.pop();
			assign[it] = top.second;
			heap.push(lu{top.first + un[it].w, top.second});
			add_unit_cost(cost[top.second], jobs, un, it, g);
		}
		double c = 0;
		for (uint32_t u = 0; u < U; u++)
			if (cost[u] > c) c = cost[u];
		if (!best_U || c < best_cost) {
			best_U = U;
			best_cost = c;
			best_assign = assign;
		}
	}
	return best_U;
}

// ---- step 3b: a forced number of super-units (measurement builds): heaviest first to the least loaded, the lower index among equals
inline void deal_forced(const group_units &un, const std::vector<uint32_t> &by_weight, uint32_t U, std::vector<uint32_t> &assign)
{
	std::vector<double> load(U, 0.0);
	assign.assign(un.size(), 0);
	for (uint32_t o = 0; o < un.size(); o++) {
		const uint32_t it = by_weight[o];
		uint32_t u = 0;
		for (uint32_t q = 1; q < U; q++)
			if (load[q] < load[u]) u = q;
		assign[it] = u;
		load[u] += un[it].w;
	}
}

// ---- step 4: the units of every super-unit, in the caller's order (a chain's jobs stay in order): by_unit[u_begin[u] .. u_begin[u + 1])
// (one counting pass -- a scan of all units per super-unit was 20 us of host time per launch at three hundred jobs on 128 super-units)
inline void deal_packed(const std::vector<uint32_t> &assign, uint32_t U, std::vector<uint32_t> &u_begin, std::vector<uint32_t> &by_unit)
{
	const uint32_t n_units = (uint32_t)assign.size();
	u_begin.assign(U + 1, 0);
	by_unit.resize(n_units);
	for (uint32_t it = 0; it < n_units; it++) u_begin[assign[it] + 1]++;
	for (uint32_t u = 0; u < U; u++) u_begin[u + 1] += u_begin[u];
	std::vector<uint32_t> fill(u_begin.begin(), u_begin.end() - 1);
	for (uint32_t it = 0; it < n_units; it++) by_unit[fill[assign[it]]++] = it;
}

// ---- step 5: every unit its proportional share of the workgroups; round8: in multiples of eight from eight on.  false: the
// minimum shares do not fit.
inline bool deal_shares(const group_units &un, int n_cu, bool round8, std::vector<uint32_t> &c_out, double &max_load)
{
	const uint32_t n_units = un.size();
	c_out.assign(n_units, 0);
	// first pass: the proportional share, rounded down (round8: to a multiple of eight from eight on), at least the workgroups
	// the exactness bound asks for, at most one per pair of tiles
	uint32_t used = 0;
	for (uint32_t i = 0; i < n_units; i++) {
		uint32_t c = (uint32_t)((double)n_cu * un[i].w / un.W);
		if (round8 && c >= 8) c &= ~7u;
		if (c < wg_needed(un[i].tiles)) c = wg_needed(un[i].tiles);
		if (c > un[i].cap) c = un[i].cap;
		if (c < 1) c = 1;
		c_out[i] = c;
		used += c;
	}
	// (minimums can overshoot only with very many very uneven units: take from the largest)
	while (used > (uint32_t)n_cu) {
		uint32_t big = 0;
		for (uint32_t i = 1; i < n_units; i++)
			if (c_out[i] > c_out[big]) big = i;
		if (c_out[big] <= 1 || c_out[big] - 1 < wg_needed(un[big].tiles)) return false;
		c_out[big]--;
		used--;
	}
	// the rest goes to whoever has the most work per workgroup (round8: eight at a time for units in multiples of eight)
	// (a heap: the heaviest load first, the lower index among equals -- a unit that cannot grow any more never can again, counts
	// and `used` only rise; the scan of all units per workgroup handed out was 25 us of host time per launch at 175 units)
	typedef std::pair<double, uint32_t> lu; // (load, n_units - 1 - index)
	std::priority_queue<lu> heap;
	for (uint32_t i = 0; i < n_units; i++)
		if (un[i].w > 0) heap.push(lu{un[i].w / c_out[i], n_units - 1 - i});
	while (!heap.empty() && used < (uint32_t)n_cu) {
		const uint32_t i = n_units - 1 - heap.top().second;
		heap.pop();
		const uint32_t step = (round8 && c_out[i] >= 8 && (c_out[i] & 7) == 0) ? 8 : 1;
		if (c_out[i] + step > un[i].cap || used + step > (uint32_t)n_cu) continue;
		c_out[i] += step;
		used += step;
		heap.push(lu{un[i].w / c_out[i], n_units - 1 - i});
	}
	max_load = 0;
	for (uint32_t i = 0; i < n_units; i++)
		if (un[i].w / c_out[i] > max_load) max_load = un[i].w / c_out[i];
	return true;
}

// In multiples of eight where that costs nothing (the XCD-aware tile order wants ranges in multiples of eight), plainly where the
// rounding would leave the launch out of balance: twelve equal jobs on 256 workgroups are 21.3 each; as 8 x 24 + 4 x 16 the launch
// lasts as long as its 16-workgroup jobs (measured, k = 12 / n = 24: the fused launches at 0.47 - 0.50 of the HBM peak against 0.58
// for k = 3 and 0.55 for k = 50), as 4 x 22 + 8 x 21 it is balanced to 1.6 % (0.56)
inline bool choose_shares(const group_units &un, int n_cu, std::vector<uint32_t> &cnt)
{
	double load8 = 0, load1 = 0;
	std::vector<uint32_t> cnt1;
	const bool ok8 = deal_shares(un, n_cu, true, cnt, load8), ok1 = un.size() > 1 && deal_shares(un, n_cu, false, cnt1, load1);
	if (ok1 && (!ok8 || load1 < 0.97 * load8)) cnt.swap(cnt1); // (the XCD-aware order is worth a few per cent, measured on the single-claim kernels)
	return ok8 || ok1;
}

// ---- step 6: table order: the units whose count is a multiple of eight first (their ranges then start on multiples of eight)
inline std::vector<uint32_t> order_units(const std::vector<uint32_t> &cnt)
{
	std::vector<uint32_t> order;
	order.reserve(cnt.size());
	for (uint32_t i = 0; i < cnt.size(); i++)
		if ((cnt[i] & 7) == 0) order.push_back(i);
	for (uint32_t i = 0; i < cnt.size(); i++)
		if ((cnt[i] & 7) != 0) order.push_back(i);
	return order;
}

// ---- step 7: the jobs of `n_ids` units become the next rows of the table, ONE chain on workgroups [wg_begin, wg_begin + wg_count):
// the first row its head, the head of each of those workgroups
inline void write_range(const group_job *jobs, const group_units &un, const uint32_t *ids, uint32_t n_ids, uint32_t wg_begin, uint32_t wg_count, group_job *rows, uint32_t &k,
                        uint32_t *head_of_wg)
{
	const uint32_t head = k;
	for (uint32_t o = 0; o < n_ids; o++)
		for (uint32_t q = 0; q < un[ids[o]].len; q++, k++) {
			rows[k] = jobs[un[ids[o]].first + q];
			rows[k].wg_begin = wg_begin;
			rows[k].wg_count = 0;
			rows[k].chain = 0;
		}
	if (k == head) return; // (a super-unit without units cannot happen: U <= n_units and the heaviest-first deal fills every one)
	rows[head].wg_count = wg_count;
	rows[head].chain = k - head - 1;
	for (uint32_t x = wg_begin; x < wg_begin + wg_count; x++) head_of_wg[x >> 1] |= head << (16 * (x & 1));
}
} // namespace group_plan_steps

// Plans launches.  Owns what outlives a call: the remembered packing decisions and the table's memory (the launcher keeps one per
// thread; a test makes its own).
class group_planner {
public:
	// pack_forced / pack_u (BN_GROUP_PACK_U of measurement builds, tools/r06_pack_sweep.sh): forced: nothing is taken from the memo;
	// pack_u > 0: that many super-units where the bounds allow it; < 0: one unit per job where that is possible
	const group_plan &plan(const group_job *jobs, uint32_t n_jobs, uint32_t n_slots, int n_cu, bool pack_forced = false, int pack_u = 0)
	{
		if (decide(jobs, n_jobs, n_slots, n_cu, pack_forced, pack_u).status == group_plan::ok) deal();
		return out_;
	}
	// the two halves of plan(), for a caller that times them: the units and the packing decision; the dealing and the table
	const group_plan &decide(const group_job *jobs, uint32_t n_jobs, uint32_t n_slots, int n_cu, bool pack_forced, int pack_u)
	{
		out_ = group_plan{};
		jobs_ = jobs;
		n_cu_ = n_cu > kGroupMaxGrid ? kGroupMaxGrid : n_cu;
		packing_ = nullptr;
		if (n_jobs == 0 || n_jobs > (uint32_t)kGroupMaxJobs || n_slots > (uint32_t)kGroupMaxSlots) return fail(group_plan::not_supported);
		out_.n_jobs = n_jobs;
		const group_plan::status_t st = group_plan_steps::collect_units(jobs, n_jobs, n_slots, n_cu_, units_, out_);
		if (st != group_plan::ok) return fail(st);
		if (!choose_packing(pack_forced, pack_u)) return fail(group_plan::not_supported);
		return out_;
	}
	const group_plan &deal()
	{
		using namespace group_plan_steps;
		if (staged_.size() < out_.n_jobs) staged_.resize(out_.n_jobs);
		uint32_t k = 0;
		if (packing_ && packing_->packed) {
			const uint32_t U = packing_->U, g = (uint32_t)n_cu_ / U;
			std::vector<uint32_t> u_begin, by_unit;
			deal_packed(packing_->assign, U, u_begin, by_unit);
			for (uint32_t u = 0; u < U; u++) write_range(jobs_, units_, by_unit.data() + u_begin[u], u_begin[u + 1] - u_begin[u], u * g, g, staged_.data(), k, out_.head_of_wg);
			out_.grid = U * g;
		} else {
			std::vector<uint32_t> cnt;
			if (n_cu_ < (int)units_.size() || !choose_shares(units_, n_cu_, cnt)) return fail(group_plan::not_supported);
			for (const uint32_t u : order_units(cnt)) {
				write_range(jobs_, units_, &u, 1, out_.grid, cnt[u], staged_.data(), k, out_.head_of_wg);
				out_.grid += cnt[u];
			}
		}
		out_.table = staged_.data();
		return out_;
	}

private:
	// (a prover's rounds repeat one shape with halving sizes: the decision for "these many units of this much weight on this many
	// tiles" is remembered -- the model costs ~10 us of host time per launch at a hundred units)
	struct decision {
		uint32_t n_units = 0, max_tiles = 0, U = 0;
		int n_cu = 0;
		double W = 0;
		bool packed = false;
		std::vector<uint32_t> assign;
	};
	const group_plan &fail(group_plan::status_t st)
	{
		out_.status = st;
		return out_;
	}
	// ---- step 3: packed or one unit per job (packing_ == null: never in question); false: neither is possible
	bool choose_packing(bool pack_forced, int pack_u)
	{
		using namespace group_plan_steps;
		const uint32_t n_units = units_.size();
		if (!(n_units > 32 || (int)n_units > n_cu_)) return true;
		// (one entry per round size: a prove walks max_tiles down by halves, the next prove of the shape finds every one of them)
		decision &d = memo_[(n_units * 31u + units_.max_tiles * 7u + (uint32_t)n_cu_) & 63u];
		packing_ = &d;
		if (d.n_units == n_units && d.max_tiles == units_.max_tiles && d.W == units_.W && d.n_cu == n_cu_ && !pack_forced) return true;
		const double unpacked = (int)n_units <= n_cu_ ? unpacked_cost(jobs_, units_, n_cu_) : -1; // (cheap: one pass over the jobs)
		std::vector<uint32_t> by_weight(n_units);
		for (uint32_t i = 0; i < n_units; i++) by_weight[i] = i;
		std::stable_sort(by_weight.begin(), by_weight.end(), [&](uint32_t a, uint32_t b) { return units_[a].w > units_[b].w; });
		double best_cost = 0;
		std::vector<uint32_t> assign;
		uint32_t U = pack_sweep(jobs_, units_, n_cu_, by_weight, best_cost, assign);
		if (!U && unpacked < 0) {
			packing_ = nullptr; // (the slot keeps what it held)
			return false;
		}
		// (one unit per job where that is no worse by the same model)
		bool packed = !(unpacked >= 0 && (!U || unpacked <= best_cost));
		if (pack_u < 0 && unpacked >= 0) packed = false;
		const uint32_t g_min = wg_needed(units_.max_tiles);
		if (pack_u > 0 && (uint32_t)pack_u <= n_units && (uint32_t)n_cu_ / (uint32_t)pack_u >= (g_min ? g_min : 1)) {
			packed = true;
			U = (uint32_t)pack_u;
			deal_forced(units_, by_weight, U, assign);
		}
		d.n_units = n_units;
		d.n_cu = n_cu_;
		d.max_tiles = units_.max_tiles;
		d.W = units_.W;
		d.packed = packed;
		d.U = U;
		d.assign.swap(assign);
		return true;
	}

	std::vector<decision> memo_ = std::vector<decision>(64);
	std::vector<group_job> staged_;
	group_units units_;
	const decision *packing_ = nullptr;
	const group_job *jobs_ = nullptr;
	int n_cu_ = 0;
	group_plan out_;
};
} // namespace bn
