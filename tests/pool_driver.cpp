// Driver of tests/test_pool_host.py: the pooled span vectors of vectorian_amd/csrc/vk_pool_host.h on the host.
//   pool <bf16> <d> <n_rows> <n_ids> <n_spans> <in> <out>   reads rows [n_rows x d] (float, or uint16 when bf16), n_ids int32 ids (0: the
//       spans index the rows), start and end (int64 each) from <in>; writes the MEAN, MIN and MAX aggregates, [n_spans x d] floats
//       each, to <out> -- pool_spans(), what the kernel computes cell by cell
//   check <n_rows> <n_ids> <n_spans> <in>                    pool_check_spans() on ids, start, end read from <in>; prints its status
//   geometry                                                 walks the grid of vk_pool_spans_kernel over a table of (d, n_spans, vec):
//       every span and every feature covered exactly once, by lanes of live chunks only
#include "vk_pool_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace vk_host;

template <typename T> static bool read_n(FILE *f, std::vector<T> &v, size_t n) {
	v.resize(n);
	return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run_pool(char **a) {
	const bool bf16 = atoi(a[0]) != 0;
	const int d = atoi(a[1]);
	const long long n_rows = atoll(a[2]), n_ids = atoll(a[3]), n_spans = atoll(a[4]);
	FILE *f = fopen(a[5], "rb");
	if (!f) return 2;
	std::vector<uint8_t> rows;
	std::vector<int32_t> ids;
	std::vector<int64_t> start, end;
	const bool ok = read_n(f, rows, (size_t)n_rows * d * (bf16 ? 2 : 4)) && read_n(f, ids, (size_t)n_ids) && read_n(f, start, (size_t)n_spans) && read_n(f, end, (size_t)n_spans);
	fclose(f);
	if (!ok) return 3;
	const char *why = "";
	if (pool_check_spans(n_rows, n_ids ? ids.data() : nullptr, n_ids, start.data(), end.data(), n_spans, &why) != POOL_OK) { printf("%s\n", why); return 4; }
	// (exactly sized: an index outside the rows is the sanitizer's to find)
	std::vector<float> out((size_t)n_spans * d);
	FILE *g = fopen(a[6], "wb");
	if (!g) return 2;
	for (const int agg : {POOL_MEAN, POOL_MIN, POOL_MAX}) {
		pool_spans(agg, rows.data(), bf16, d, n_ids ? ids.data() : nullptr, start.data(), end.data(), n_spans, out.data());
		if (!out.empty() && fwrite(out.data(), 4, out.size(), g) != out.size()) return 5;
	}
	fclose(g);
	return 0;
}

static int run_check(char **a) {
	const long long n_rows = atoll(a[0]), n_ids = atoll(a[1]), n_spans = atoll(a[2]);
	FILE *f = fopen(a[3], "rb");
	if (!f) return 2;
	std::vector<int32_t> ids;
	std::vector<int64_t> start, end;
	const bool ok = read_n(f, ids, (size_t)n_ids) && read_n(f, start, (size_t)n_spans) && read_n(f, end, (size_t)n_spans);
	fclose(f);
	if (!ok) return 3;
	const char *why = "";
	printf("%d %s\n", pool_check_spans(n_rows, n_ids ? ids.data() : nullptr, n_ids, start.data(), end.data(), n_spans, &why), why);
	return 0;
}

static int run_geometry() {
	const int ds[] = {1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 768, 1024, 1025, 4096, 8191, 8192};
	const long long ns[] = {0, 1, 2, 3, 4, 5, 8, 9, 33, 64, 65, 513};
	long long points = 0, violations = 0;
	for (const int d : ds)
		for (const long long n : ns)
			for (const int vec : {1, 4}) {
				if (vec == 4 && pool_vec(d, 4, 0) != 4) continue;   // 16-byte pieces: only where every row starts on one
				if (pool_vec(d, 4, 4) != 1 || pool_vec(d, 2, 2) != 1) { violations++; printf("VIOLATED a base off the boundary takes pieces: d %d\n", d); }
				points++;
				std::vector<int> seen((size_t)n * d, 0);
				long long stray = 0;
				const long long grid = pool_grid(n);
				for (long long block = 0; block < grid; block++)
					for (int wave = 0; wave < kPoolSpansPerBlock; wave++) {
						const long long span = pool_span_of(block, wave);
						if (span >= n) continue;   // (the wave returns)
						for (int pass = 0; pass < pool_passes(d, vec); pass++)
							for (int chunk = 0; chunk < kPoolChunksPerPass; chunk++)
								for (int lane = 0; lane < 64; lane++) {
									const int f0 = pool_feature_of(pass, chunk, lane, vec);
									if (f0 >= d) continue;   // (the lane loads and stores nothing)
									if (pass * kPoolChunksPerPass + chunk >= pool_chunks(d, vec)) stray++;
									for (int e = 0; e < vec; e++) {
										if (f0 + e >= d) stray++;
										else seen[(size_t)span * d + f0 + e]++;
									}
								}
					}
				bool once = stray == 0 && grid * kPoolSpansPerBlock >= n && (grid - 1) * kPoolSpansPerBlock < n + (n == 0);
				for (const int s : seen) once = once && s == 1;
				if (!once) { violations++; printf("VIOLATED coverage: d %d n_spans %lld vec %d stray %lld\n", d, n, vec, stray); }
			}
	printf("points %lld violations %lld\n", points, violations);
	return violations ? 1 : 0;
}

int main(int argc, char **argv) {
	if (argc == 9 && !strcmp(argv[1], "pool")) return run_pool(argv + 2);
	if (argc == 6 && !strcmp(argv[1], "check")) return run_check(argv + 2);
	if (argc == 2 && !strcmp(argv[1], "geometry")) return run_geometry();
	fprintf(stderr, "usage: pool_driver pool|check|geometry ...\n");
	return 64;
}
