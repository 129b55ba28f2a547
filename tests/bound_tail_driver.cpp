// Driver of tests/test_bound_tail_host.py: the flat tail of the slice-gap table as the host computes it (vk_bound_host.h and nothing
// else).
//   bound_tail_driver cost    "K rows n w[0] .. w[n-1]" per line on stdin (entries beyond n: +inf, as vk_host::gap_cost reads a short
//                             table) -> the bits of bound_tail_cost(w, K, rows), one line each
//   bound_tail_driver choice  "env mode" per line (env: 0, 1, x for another value, - for unset; mode: -1 off, 0 by size, 1 force) -> 0 / 1
#include "vk_bound_host.h"

#include <cstdio>
#include <string>
#include <vector>

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "cost") {
		int k, rows, n;
		while (scanf("%d %d %d", &k, &rows, &n) == 3) {
			std::vector<float> w((size_t)rows + 1, INFINITY);   // exactly rows + 1 entries: a read past them is the sanitizer's
			for (int i = 0; i < n; i++) {
				float x;
				if (scanf("%f", &x) != 1) return 2;
				if (i <= rows) w[(size_t)i] = x;
			}
			const float c = vk_host::bound_tail_cost(w.data(), k, rows);
			uint32_t u;
			memcpy(&u, &c, 4);
			printf("%08x\n", u);
		}
		return 0;
	}
	if (what == "choice") {
		char env[16];
		int mode;
		while (scanf("%15s %d", env, &mode) == 2) {
			const std::string e = env;
			printf("%d\n", (int)vk_host::bound_tail_choice(e == "-" ? nullptr : e == "x" ? "yes" : env, mode));
		}
		return 0;
	}
	return 2;
}
