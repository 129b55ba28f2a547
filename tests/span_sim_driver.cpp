// span_sim_driver.cpp -- stand-alone driver over vectorian_amd/csrc/vk_span_sim_host.h (tests/test_span_sim_host.py; CPU tier).
//   (no argument)   the streamed cell against vk_host::sim_src_cell, bit for bit: every width x every form x rows of three
//                   magnitudes, a zero row, a row equal to the query, a NaN row; "cells N mismatches M nan_ok K"
//   walk            the grid walk over a table of span counts and CU counts: every tile exactly once; "walks N violations M"
//   grid n cus      the grid
//   floor x         the selection's floor for min_score x
//   shape a l t u tagged submatch boost flow only rows     the refusal of a query ("ok": span-shaped)
//   lds d           bytes of the staged query
#include "vk_span_sim_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace vk_host;

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

static int run_cells() {
	const int widths[] = {1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 64, 67, 100, 300, 768, 1024};
	const sim_src sources[] = {{VK_SIMSRC_PNORM, 1.0f}, {VK_SIMSRC_PNORM, 2.0f}, {VK_SIMSRC_PNORM, 3.0f}, {VK_SIMSRC_PNORM, 0.5f}, {VK_SIMSRC_SQRT_COSINE, 0.0f}};
	long cells = 0, mismatches = 0, nan_ok = 0;
	std::mt19937 rng(17);
	std::normal_distribution<float> normal(0.0f, 1.0f);
	const float mags[3] = {1e-3f, 1.0f, 1e3f};
	for (const int d : widths) {
		std::vector<float> q((size_t)d);
		for (float &x : q) x = normal(rng) * mags[rng() % 3];
		std::vector<std::vector<float>> rows;
		for (int r = 0; r < 24; r++) {
			std::vector<float> a((size_t)d);
			for (float &x : a) x = normal(rng) * mags[rng() % 3];
			rows.push_back(a);
		}
		rows.push_back(std::vector<float>((size_t)d, 0.0f));   // a zero row
		rows.push_back(q);                                      // a row equal to the query
		std::vector<float> neg(q);                              // ... and its negative (no product is positive)
		for (float &x : neg) x = -x;
		rows.push_back(neg);
		const std::vector<float> nan_row((size_t)d, NAN);
		for (const sim_src &src : sources) {
			for (const auto &a : rows) {
				const float want = sim_src_cell(a.data(), q.data(), d, src), got = span_sim_cell_streamed(a.data(), q.data(), d, src);
				cells++;
				if (bits(want) != bits(got)) {
					mismatches++;
					printf("MISMATCH d %d kind %d p %g: %a != %a\n", d, src.kind, (double)src.arg, (double)got, (double)want);
				}
			}
			// a zero query against every row too (the sqrt-cosine's 0 / 0)
			const std::vector<float> zq((size_t)d, 0.0f);
			for (const auto &a : rows) {
				const float want = sim_src_cell(a.data(), zq.data(), d, src), got = span_sim_cell_streamed(a.data(), zq.data(), d, src);
				cells++;
				if (bits(want) != bits(got)) { mismatches++; printf("MISMATCH zero query d %d kind %d\n", d, src.kind); }
			}
			// a row of NaN: NaN under a p-norm; under the sqrt-cosine the header's nan_to_num rule, as written
			const float got = span_sim_cell_streamed(nan_row.data(), q.data(), d, src), want = sim_src_cell(nan_row.data(), q.data(), d, src);
			const bool ok = src.kind == VK_SIMSRC_PNORM ? (got != got && want != want) : bits(got) == bits(want);
			if (ok) nan_ok++; else printf("NAN ROW d %d kind %d p %g: %a (cell %a)\n", d, src.kind, (double)src.arg, (double)got, (double)want);
		}
	}
	printf("cells %ld mismatches %ld nan_ok %ld\n", cells, mismatches, nan_ok);
	return mismatches == 0 ? 0 : 1;
}

static long walk_one(int64_t n, int cus, std::vector<uint8_t> &seen) {
	const int64_t tiles = span_sim_tiles(n);
	const int grid = span_sim_grid(n, cus);
	long violations = 0;
	if (grid < 1 || grid > cus * kSpanSimBlocksPerCu) violations++;
	seen.assign((size_t)tiles, 0);
	for (int64_t block = 0; block < grid; block++)
		for (int wave = 0; wave < kSpanSimWaves; wave++)
			for (int64_t run = span_sim_first_run(block, wave); span_sim_run_begin(run) < tiles; run += span_sim_run_stride(grid))
				for (int64_t tile = span_sim_run_begin(run); tile < span_sim_run_end(run, tiles); tile++) {
					if (tile < 0 || tile >= tiles) { violations++; continue; }
					seen[(size_t)tile]++;
				}
	for (int64_t t = 0; t < tiles; t++) if (seen[(size_t)t] != 1) violations++;
	if (violations) printf("VIOLATED n %lld cus %d grid %d\n", (long long)n, cus, grid);
	return violations;
}

static int run_walk() {
	std::vector<int64_t> counts;
	for (int64_t n = 1; n <= 2100; n++) counts.push_back(n);
	for (int s = 11; s <= 20; s++) for (int64_t dlt = -17; dlt <= 17; dlt++) if (((int64_t)1 << s) + dlt <= ((int64_t)1 << 20)) counts.push_back(((int64_t)1 << s) + dlt);
	const int cu_counts[] = {1, 2, 7, 64, 256, 304};
	// one tile more than one full sweep of the grid, and around it
	for (const int cus : cu_counts) {
		const int64_t sweep = (int64_t)cus * kSpanSimBlocksPerCu * kSpanSimWaves * kSpanSimRun;
		for (int64_t t = sweep - 1; t <= sweep + 1; t++) if (t >= 1 && t * 16 <= ((int64_t)1 << 20)) { counts.push_back(t * 16); counts.push_back(t * 16 - 15); }
	}
	long walks = 0, violations = 0;
	std::vector<uint8_t> seen;
	for (const int cus : cu_counts)
		for (const int64_t n : counts) { violations += walk_one(n, cus, seen); walks++; }
	printf("walks %ld violations %ld\n", walks, violations);
	return violations == 0 ? 0 : 1;
}

int main(int argc, char **argv) {
	if (argc < 2) return run_cells();
	if (!strcmp(argv[1], "walk")) return run_walk();
	if (!strcmp(argv[1], "grid") && argc == 4) { printf("%d\n", span_sim_grid(atoll(argv[2]), atoi(argv[3]))); return 0; }
	if (!strcmp(argv[1], "floor") && argc == 3) { printf("%a\n", (double)span_sim_floor(strtof(argv[2], nullptr))); return 0; }
	if (!strcmp(argv[1], "lds") && argc == 3) { printf("%zu %d\n", span_sim_lds_bytes(atoi(argv[2])), span_sim_raw_tile_bytes(atoi(argv[2]))); return 0; }
	if (!strcmp(argv[1], "shape") && argc == 12) {
		span_sim_query q;
		q.algorithm = atoi(argv[2]); q.locality = atoi(argv[3]); q.len_t = atoi(argv[4]); q.uniform_len = atoi(argv[5]);
		q.tagged = atoi(argv[6]); q.submatch = atoi(argv[7]); q.boost = atoi(argv[8]); q.want_flow = atoi(argv[9]); q.only = atoi(argv[10]); q.sim_rows = atoi(argv[11]);
		const char *why = span_sim_refusal(q);
		printf("%s\n", why ? why : "ok");
		return span_sim_shaped(q) == (why == nullptr) ? 0 : 1;
	}
	fprintf(stderr, "usage\n");
	return 2;
}
