// binius_amd/csrc/batch.hpp -- device side of "one launch serves a table of jobs": the host sorts the jobs of a call by the first
// unit (workgroup, wave or run) each owns, a unit finds its job by bisection and reads the job's fields into scalar registers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bn {

// the job of unit `u`: jobs[j].start <= u < jobs[j + 1].start (jobs[0].start == 0)
template <typename JOB>
__device__ __forceinline__ uint32_t find_job(const JOB *__restrict__ jobs, uint32_t n_jobs, uint32_t u)
{
	uint32_t lo = 0, hi = n_jobs;
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (jobs[mid].start <= u)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// A value (or pointer, as uint64_t) that is the same in every lane of the wave, moved to scalar registers: what is derived from it
// stays out of the vector registers.
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uni32((uint32_t)v) | ((uint64_t)uni32((uint32_t)(v >> 32)) << 32); }

} // namespace bn
