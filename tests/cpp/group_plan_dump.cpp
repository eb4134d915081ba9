// tests/cpp/group_plan_dump.cpp -- plans group launches on the CPU and prints the plans (tests/test_group_plan.py).  No HIP call.
//
//   group_plan_dump CASES            plan every case of the file, print every plan
//   group_plan_dump CASES loop N     N plans of every case, its lists in turn with one planner: plans per second
//
// A case:  case NAME n_cu n_slots pack_u n_lists, then per list its length and per job  kind n chain slot acquire one_array.
// The lists of a case are planned in order with ONE planner (its memo is part of what is tested); pack_u != 0 is BN_GROUP_PACK_U set.
// Job i of a list carries i in z.lo, which the planner copies untouched: a row names its source job.
// A plan:  list status grid full total_elems streams n_rows, the rows  source wg_begin wg_count chain,  head w[0 .. kGroupMaxGrid / 2).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../binius_amd/csrc/group_plan.hpp"

namespace {
struct plan_case {
	std::string name;
	int n_cu = 0, pack_u = 0;
	uint32_t n_slots = 0;
	std::vector<std::vector<bn::group_job>> lists;
};

bool read_cases(const char *path, std::vector<plan_case> &cases)
{
	FILE *f = fopen(path, "r");
	if (!f) return false;
	char word[64], name[192];
	while (fscanf(f, "%63s", word) == 1) {
		plan_case c;
		unsigned n_lists = 0;
		if (strcmp(word, "case") || fscanf(f, "%191s %d %u %d %u", name, &c.n_cu, &c.n_slots, &c.pack_u, &n_lists) != 5) return false;
		c.name = name;
		for (unsigned l = 0; l < n_lists; l++) {
			unsigned n_jobs = 0;
			if (fscanf(f, "%u", &n_jobs) != 1 || n_jobs > 4096) return false;
			std::vector<bn::group_job> jobs(n_jobs);
			for (unsigned i = 0; i < n_jobs; i++) {
				unsigned long long n = 0;
				unsigned one = 0;
				bn::group_job j{};
				if (fscanf(f, "%u %llu %u %u %u %u", &j.kind, &n, &j.chain, &j.slot, &j.acquire, &one) != 6) return false;
				j.n = n;
				j.x0[0] = &cases; // (placeholders: the planner only asks whether x0[1] is null)
				j.x0[1] = one ? nullptr : &cases;
				j.z.lo = i;
				jobs[i] = j;
			}
			c.lists.push_back(jobs);
		}
		cases.push_back(c);
	}
	fclose(f);
	return true;
}

int status_code(bn::group_plan::status_t s) { return s == bn::group_plan::ok ? 0 : s == bn::group_plan::invalid ? 1 : 801; }

void print_plan(const bn::group_plan &p)
{
	if (p.status != bn::group_plan::ok) {
		printf("list %d 0 0 0 0 0\n", status_code(p.status));
		return;
	}
	printf("list 0 %u %d %llu %d %u\n", p.grid, (int)p.full, (unsigned long long)p.total_elems, (int)bn::group_plan_streams(p, 25), p.n_jobs);
	for (uint32_t i = 0; i < p.n_jobs; i++) printf("%llu %u %u %u\n", (unsigned long long)p.table[i].z.lo, p.table[i].wg_begin, p.table[i].wg_count, p.table[i].chain);
	printf("head");
	for (int i = 0; i < bn::kGroupMaxGrid / 2; i++) printf(" %u", p.head_of_wg[i]);
	printf("\n");
}
} // namespace

int main(int argc, char **argv)
{
	std::vector<plan_case> cases;
	if (argc < 2 || !read_cases(argv[1], cases)) {
		fprintf(stderr, "usage: group_plan_dump CASES [loop N]\n");
		return 2;
	}
	const int reps = argc >= 4 && !strcmp(argv[2], "loop") ? atoi(argv[3]) : 0;
	for (const plan_case &c : cases) {
		bn::group_planner planner;
		if (reps <= 0) {
			printf("case %s\n", c.name.c_str());
			for (const auto &jobs : c.lists) print_plan(planner.plan(jobs.data(), (uint32_t)jobs.size(), c.n_slots, c.n_cu, c.pack_u != 0, c.pack_u));
			continue;
		}
		const auto t0 = std::chrono::steady_clock::now();
		uint64_t acc = 0;
		for (int r = 0; r < reps; r++) {
			const auto &jobs = c.lists[(size_t)r % c.lists.size()];
			acc += planner.plan(jobs.data(), (uint32_t)jobs.size(), c.n_slots, c.n_cu, c.pack_u != 0, c.pack_u).grid;
		}
		const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		printf("%s %.0f plans/s (%llu)\n", c.name.c_str(), reps / sec, (unsigned long long)acc);
	}
	return 0;
}
