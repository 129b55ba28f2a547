// saliency_driver.cpp -- vk_saliency_host.h on the host (tests/test_saliency_host.py builds this with g++, plain and under
// AddressSanitizer / UBSan, and runs it as a stand-alone program).  Every command reads its arrays from a binary file, one after the
// other, and writes float32 results to another:
//   keywords V max_count n_tokens n_slices n_kw in out   in: ids int32, start int64, end int64, keyword ids int32
//   filter kind width n_docs n_slices in out             in: x float32, doc_off int64 [n_docs + 1], pulse float64 [width] (kind 1)
//   average n_signals n_slices in out                    in: weights float64 [n_signals + 1], signals float32 [n_signals x n_slices]
//   geometry                                             walks the grids of the three kernels
#include "vk_saliency_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct reader {
	FILE *f;
	explicit reader(const char *path) : f(fopen(path, "rb")) { if (!f) { perror(path); exit(2); } }
	~reader() { fclose(f); }
	template <typename T> std::vector<T> take(size_t n) {
		std::vector<T> v(n);
		if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
		return v;
	}
};

void write_floats(const char *path, const std::vector<float> &v) {
	FILE *f = fopen(path, "wb");
	if (!f) { perror(path); exit(2); }
	if (!v.empty() && fwrite(v.data(), 4, v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(2); }
	fclose(f);
}

int keywords(char **a) {
	const int64_t V = atoll(a[0]);
	const int32_t max_count = atoi(a[1]);
	const size_t n_tokens = (size_t)atoll(a[2]), n_slices = (size_t)atoll(a[3]), n_kw = (size_t)atoll(a[4]);
	reader in(a[5]);
	const auto ids = in.take<int32_t>(n_tokens);
	const auto start = in.take<int64_t>(n_slices), end = in.take<int64_t>(n_slices);
	const auto kw = in.take<int32_t>(n_kw);
	std::vector<uint32_t> bitmap((size_t)vk_host::sal_bitmap_words(V), 0u);
	for (int32_t k : kw) vk_host::sal_bitmap_set(bitmap.data(), k);
	std::vector<float> out(n_slices);
	for (size_t s = 0; s < n_slices; s++) out[s] = vk_host::sal_keyword_signal(ids.data(), start[s], end[s], bitmap.data(), V, max_count);
	write_floats(a[6], out);
	return 0;
}

int filter(char **a) {
	const int32_t kind = atoi(a[0]), width = atoi(a[1]);
	const int64_t n_docs = atoll(a[2]);
	const size_t n = (size_t)atoll(a[3]);
	reader in(a[4]);
	const auto x = in.take<float>(n);
	const auto doc_off = in.take<int64_t>((size_t)n_docs + 1);
	const auto pulse = in.take<double>(kind == vk_host::SAL_FILTER_CONV ? (size_t)width : 0);
	const char *why = "";
	if (vk_host::sal_check_docs(doc_off.data(), n_docs, (int64_t)n, &why)) { fprintf(stderr, "%s\n", why); return 3; }
	std::vector<float> y(n);
	vk_host::sal_filter(kind, x.data(), y.data(), doc_off.data(), n_docs, width, pulse.data());
	// the kernel's walk: a slice finds its document by bisection
	for (size_t s = 0; s < n; s++) {
		const int64_t d = vk_host::sal_doc_of(doc_off.data(), n_docs, (int64_t)s);
		if (!(doc_off[(size_t)d] <= (int64_t)s && (int64_t)s < doc_off[(size_t)d + 1])) { fprintf(stderr, "slice %zu: document %lld\n", s, (long long)d); return 4; }
	}
	write_floats(a[5], y);
	return 0;
}

int average(char **a) {
	const int32_t m = atoi(a[0]);
	const size_t n = (size_t)atoll(a[1]);
	if (m < 0 || m > vk_host::kSalMaxSignals) return 3;
	reader in(a[2]);
	const auto w = in.take<double>((size_t)m + 1);
	const auto sig = in.take<float>((size_t)m * n);
	const float *signals[vk_host::kSalMaxSignals] = {};
	double weights[vk_host::kSalMaxSignals + 1] = {};
	for (int k = 0; k < m; k++) signals[k] = sig.data() + (size_t)k * n;
	for (int k = 0; k <= m; k++) weights[k] = w[(size_t)k];
	const double wsum = vk_host::sal_numpy_sum(w.data(), (int64_t)m + 1);
	std::vector<float> out(n);
	for (size_t s = 0; s < n; s++) out[s] = vk_host::sal_boost_cell(signals, m, weights, wsum, (int64_t)s);
	write_floats(a[3], out);
	return 0;
}

int geometry() {
	long long points = 0, violations = 0;
	const int64_t sizes[] = {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4095, 4096, 4097, 65535, 65536, 1000003, (int64_t)1 << 20};
	for (int64_t n : sizes) {
		std::vector<uint8_t> seen((size_t)n, 0);
		const int64_t grid = vk_host::sal_keyword_grid(n);
		if (grid < 1 || grid > vk_host::kSalMaxKeywordBlocks) { printf("VIOLATED keyword grid %lld for %lld\n", (long long)grid, (long long)n); violations++; }
		for (int64_t b = 0; b < grid; b++)
			for (int w = 0; w < vk_host::kSalWavesPerBlock; w++)
				for (int64_t s = vk_host::sal_keyword_first(b, w); s < n; s += vk_host::sal_keyword_stride(grid)) seen[(size_t)s]++;
		for (int64_t s = 0; s < n; s++) if (seen[(size_t)s] != 1) { printf("VIOLATED keyword slice %lld of %lld seen %d\n", (long long)s, (long long)n, seen[(size_t)s]); violations++; break; }
		std::fill(seen.begin(), seen.end(), 0);
		const int64_t cells = vk_host::sal_cell_grid(n);
		for (int64_t b = 0; b < cells; b++)
			for (int t = 0; t < vk_host::kSalThreads; t++) {
				const int64_t s = vk_host::sal_cell_of(b, t);
				if (s < n) seen[(size_t)s]++;
			}
		for (int64_t s = 0; s < n; s++) if (seen[(size_t)s] != 1) { printf("VIOLATED cell %lld of %lld seen %d\n", (long long)s, (long long)n, seen[(size_t)s]); violations++; break; }
		points += 2;
	}
	// the bitmap of the largest staged vocabulary fills 64 KiB of LDS exactly, the next one is read from global memory
	if (vk_host::sal_bitmap_words(vk_host::kSalLdsVocab) * 4 != 65536) { printf("VIOLATED staged bitmap bytes\n"); violations++; }
	printf("points %lld violations %lld\n", points, violations);
	return violations ? 1 : 0;
}

} // namespace

int main(int argc, char **argv) {
	const std::string cmd = argc > 1 ? argv[1] : "";
	if (cmd == "keywords" && argc == 9) return keywords(argv + 2);
	if (cmd == "filter" && argc == 8) return filter(argv + 2);
	if (cmd == "average" && argc == 6) return average(argv + 2);
	if (cmd == "geometry" && argc == 2) return geometry();
	fprintf(stderr, "usage: saliency_driver keywords|filter|average|geometry ...\n");
	return 2;
}
