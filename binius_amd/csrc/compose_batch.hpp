// binius_amd/csrc/compose_batch.hpp -- a batch of tower-typed expressions (bn_expr_compile_tower_batch): the plan of the ONE launch that
// bn_compute_composite makes for it.  Host-only C++ beside compose_tower.hpp, nothing of HIP: the library plans with it, and a
// stand-alone program on the CPU (tests/cpp/compose_batch_check.cpp, also the target of a host sanitizer build) walks the grid the
// plan describes.
//
// The plan: the programs of the jobs with duplicates dropped, laid out one after the other in three sections (ops, constants, input
// levels); one device-visible row per job, in the caller's order, which is also the order of the first unit (`start`) a job owns -- a
// unit is kComposeUnitElems output elements, a workgroup of the kernel --; the elements-per-thread class of each job and the launch's
// dynamic LDS, the maximum over the jobs.  cb_plan checks what the jobs alone decide (bn_expr_compile_tower_batch), cb_check_call what
// the pointers of a call decide (bn_compute_composite); both answer nullptr or the reason of the rejection.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "compose_tower.hpp"

namespace bn {

// One job as the kernel reads it.  Offsets count entries of the call's sections (ct_op, f128, uint32_t); the kernel adds the bases.
struct compose_batch_job {
	uint32_t start;      // the first unit of the job; ascending through the table, jobs[0].start == 0
	uint32_t q;          // output elements a thread holds at a time: 4, 2 or 1 (compose_tower_per_thread of the program's slots)
	uint32_t ops_off;    // the program's ops: ops[ops_off .. ops_off + n_ops)
	uint32_t n_ops;
	uint32_t consts_off; // the program's constant table starts at consts[consts_off]
	uint32_t levels_off; // the program's input levels start at in_levels[levels_off]
	uint32_t first_row;  // input v is rows[first_row + v]
	uint32_t result;     // operand that holds the value of the expression
	uint32_t out_level;
	uint32_t n_slots;
	uint64_t out_elems;  // 2^(n_vars + out_level - 7)
	uint64_t out_offset; // in 16-byte elements from the call's output arena
	uint64_t reserved;
};
static_assert(sizeof(compose_batch_job) == 64, "compose_batch_job is read by the device in this layout");
static_assert(offsetof(compose_batch_job, start) == 0 && offsetof(compose_batch_job, q) == 4 && offsetof(compose_batch_job, ops_off) == 8 &&
                  offsetof(compose_batch_job, first_row) == 24 && offsetof(compose_batch_job, out_level) == 32 && offsetof(compose_batch_job, out_elems) == 40 &&
                  offsetof(compose_batch_job, out_offset) == 48,
              "compose_batch_job is read by the device in this layout");

struct compose_batch_plan {
	std::vector<ct_program> programs;      // distinct, in the order of their first job
	std::vector<compose_batch_job> jobs;   // the caller's order
	std::vector<uint32_t> job_program;     // jobs[j] runs programs[job_program[j]]
	std::vector<uint32_t> job_n_vars;
	uint32_t n_rows = 0;                   // rows a call must pass: max over jobs of first_row + the job's inputs
	uint32_t total_units = 0;              // the grid
	uint32_t lds_bytes = 0;                // dynamic LDS of the launch: the maximum over jobs, <= 64 KiB
	uint32_t n_ops = 0, n_consts = 0, n_levels = 0; // entries of the three program sections
};

inline bool cb_same_program(const ct_program &x, const ct_program &y)
{
	if (x.out_level != y.out_level || x.n_slots != y.n_slots || x.result != y.result) return false;
	if (x.ops.size() != y.ops.size() || x.consts.size() != y.consts.size() || x.input_levels != y.input_levels) return false;
	for (size_t i = 0; i < x.ops.size(); i++) {
		const ct_op &a = x.ops[i], &b = y.ops[i];
		if (a.kind != b.kind || a.dst != b.dst || a.a != b.a || a.b != b.b || a.exp != b.exp || a.level != b.level) return false;
	}
	for (size_t i = 0; i < x.consts.size(); i++)
		if (x.consts[i].lo != y.consts[i].lo || x.consts[i].hi != y.consts[i].hi) return false;
	return true;
}

struct cb_range {
	uint64_t begin, end;
	bool output;
};

// Plans `jobs` over the compiled programs `progs` (a null entry: a member that is no tower expression).  Nothing is kept of a rejected
// batch.
inline const char *cb_plan(const ct_program *const *progs, uint32_t n_progs, const bn_compose_job *jobs, uint32_t n_jobs, compose_batch_plan &out)
{
	if (!progs || !jobs) return "null argument";
	if (n_jobs == 0 || n_jobs > BN_COMPOSE_BATCH_MAX_JOBS) return "the number of jobs is 0 or above BN_COMPOSE_BATCH_MAX_JOBS";
	compose_batch_plan p;
	std::vector<uint32_t> program_of(n_progs, ~0u); // member -> distinct program
	std::vector<cb_range> outs;
	uint64_t units = 0;
	for (uint32_t j = 0; j < n_jobs; j++) {
		const bn_compose_job &jb = jobs[j];
		if (jb.expr >= n_progs) return "a job's expr is not below n_exprs";
		if (!progs[jb.expr]) return "a member is not a tower expression";
		if (jb.reserved != 0) return "reserved must be 0";
		const ct_program &prog = *progs[jb.expr];
		if (jb.n_vars > BN_PE_MAX_VARS) return "a column has at most 2^BN_PE_MAX_VARS values";
		if (jb.n_vars + prog.out_level < 7) return "an output is at least one 128-bit element";
		if (program_of[jb.expr] == ~0u) {
			uint32_t k = 0;
			while (k < p.programs.size() && !cb_same_program(p.programs[k], prog)) k++;
			if (k == p.programs.size()) p.programs.push_back(prog);
			program_of[jb.expr] = k;
		}
		const uint32_t n_inputs = (uint32_t)prog.input_levels.size();
		if (jb.first_row > 0xffffffffu - n_inputs) return "a job's rows leave 32 bits";
		compose_batch_job d{};
		d.q = compose_tower_per_thread(prog.n_slots);
		d.n_ops = (uint32_t)prog.ops.size();
		d.first_row = jb.first_row;
		d.result = prog.result;
		d.out_level = prog.out_level;
		d.n_slots = prog.n_slots;
		d.out_elems = (uint64_t)1 << (jb.n_vars + prog.out_level - 7);
		d.out_offset = jb.out_offset;
		if (d.out_offset > ~(uint64_t)0 - d.out_elems) return "an output range leaves 64 bits";
		const uint64_t n_units = (d.out_elems + kComposeUnitElems - 1) / kComposeUnitElems;
		if (units + n_units >= ((uint64_t)1 << 31)) return "the batch's units leave 31 bits";
		d.start = (uint32_t)units;
		units += n_units;
		p.jobs.push_back(d);
		p.job_program.push_back(program_of[jb.expr]);
		p.job_n_vars.push_back(jb.n_vars);
		p.n_rows = std::max(p.n_rows, jb.first_row + n_inputs);
		p.lds_bytes = std::max(p.lds_bytes, compose_tower_lds_bytes(prog.n_slots));
		outs.push_back(cb_range{d.out_offset, d.out_offset + d.out_elems, true});
	}
	// no two outputs overlap: one sweep over the sorted ranges
	std::sort(outs.begin(), outs.end(), [](const cb_range &x, const cb_range &y) { return x.begin < y.begin; });
	for (size_t i = 1; i < outs.size(); i++)
		if (outs[i].begin < outs[i - 1].end) return "two jobs' outputs overlap";
	// the upload layout: every distinct program once
	std::vector<uint32_t> ops_off, consts_off, levels_off;
	for (const ct_program &prog : p.programs) {
		ops_off.push_back(p.n_ops);
		consts_off.push_back(p.n_consts);
		levels_off.push_back(p.n_levels);
		p.n_ops += (uint32_t)prog.ops.size();
		p.n_consts += (uint32_t)prog.consts.size();
		p.n_levels += (uint32_t)prog.input_levels.size();
	}
	for (uint32_t j = 0; j < n_jobs; j++) {
		p.jobs[j].ops_off = ops_off[p.job_program[j]];
		p.jobs[j].consts_off = consts_off[p.job_program[j]];
		p.jobs[j].levels_off = levels_off[p.job_program[j]];
	}
	p.total_units = (uint32_t)units;
	out = std::move(p);
	return nullptr;
}

// the three program sections of the upload, each of the plan's size
inline void cb_fill(const compose_batch_plan &p, ct_op *ops, f128 *consts, uint32_t *levels)
{
	for (const ct_program &prog : p.programs) {
		ops = std::copy(prog.ops.begin(), prog.ops.end(), ops);
		consts = std::copy(prog.consts.begin(), prog.consts.end(), consts);
		levels = std::copy(prog.input_levels.begin(), prog.input_levels.end(), levels);
	}
}

inline uint64_t cb_column_elems(uint32_t n_vars, uint32_t level) { return n_vars + level <= 7 ? 1 : (uint64_t)1 << (n_vars + level - 7); }

// What a call's pointers decide: rows[0 .. n_rows) the input columns (addresses), `out` the arena of out_len elements.
inline const char *cb_check_call(const compose_batch_plan &p, const uint64_t *rows, uint32_t n_rows, uint64_t row_len, uint64_t out, uint64_t out_len)
{
	if (!rows || !out) return "null argument";
	if (row_len != out_len) return "row_len must equal out_len, the elements of the output arena";
	if (p.n_rows > n_rows) return "the batch reads more rows than the call passes";
	if (out & 15) return "misaligned pointer";
	if (out_len > (~(uint64_t)0 - out) / 16) return "the arena leaves the address space";
	std::vector<cb_range> ranges;
	for (size_t j = 0; j < p.jobs.size(); j++) {
		const compose_batch_job &d = p.jobs[j];
		const ct_program &prog = p.programs[p.job_program[j]];
		if (d.out_offset > out_len || d.out_elems > out_len - d.out_offset) return "a job's output leaves the arena";
		ranges.push_back(cb_range{out + 16 * d.out_offset, out + 16 * (d.out_offset + d.out_elems), true});
		for (size_t v = 0; v < prog.input_levels.size(); v++) {
			const uint64_t r = rows[d.first_row + v];
			if (!r || (r & 15)) return "null or misaligned row";
			const uint64_t bytes = 16 * cb_column_elems(p.job_n_vars[j], prog.input_levels[v]);
			if (bytes > ~(uint64_t)0 - r) return "a row leaves the address space";
			ranges.push_back(cb_range{r, r + bytes, false});
		}
	}
	// an output overlaps neither a row of any job nor another output (rows may overlap each other): one sweep over the sorted ranges
	std::sort(ranges.begin(), ranges.end(), [](const cb_range &x, const cb_range &y) { return x.begin < y.begin; });
	uint64_t end_in = 0, end_out = 0;
	for (const cb_range &r : ranges) {
		if (r.begin < end_out || (r.output && r.begin < end_in)) return "an output overlaps a row or another output";
		(r.output ? end_out : end_in) = std::max(r.output ? end_out : end_in, r.end);
	}
	return nullptr;
}

} // namespace bn
