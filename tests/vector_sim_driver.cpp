// vector_sim_driver.cpp -- a stand-alone driver of vectorian_amd/csrc/vk_sim_src_host.h for tests/test_vector_sim_host.py (CPU tier).
//   cells:  stdin "kind argbits d n m", then the n rows of A and the m rows of B, one float per token as the hex of its bits; prints
//           vk_host::sim_src_cell of every row of A against every row of B the same way, row-major
//   check:  stdin "kind argbits"; prints the status of vk_host::sim_src_check
// Host only; built with g++, plain and under AddressSanitizer and UBSan.
#include "vk_sim_src_host.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	int kind = 0;
	uint32_t bits = 0;
	if (scanf("%d %x", &kind, &bits) != 2) return 2;
	const vk_host::sim_src src{kind, from_bits(bits)};
	if (what == "check") {
		printf("%d\n", vk_host::sim_src_check(src.kind, src.arg));
		return 0;
	}
	int d = 0, n = 0, m = 0;
	if (what != "cells" || scanf("%d %d %d", &d, &n, &m) != 3 || d < 1 || n < 0 || m < 0) return 2;
	if (vk_host::sim_src_check(src.kind, src.arg) != VK_OK || src.kind == VK_SIMSRC_COSINE) return 2;
	// every row in a vector of exactly d floats: a read past a row is a read past an allocation
	std::vector<std::vector<float>> rows((size_t)n + (size_t)m, std::vector<float>((size_t)d));
	for (auto &row : rows)
		for (int k = 0; k < d; k++) {
			uint32_t u;
			if (scanf("%x", &u) != 1) return 2;
			row[(size_t)k] = from_bits(u);
		}
	for (int i = 0; i < n; i++)
		for (int j = 0; j < m; j++)
			printf("%08x\n", to_bits(vk_host::sim_src_cell(rows[(size_t)i].data(), rows[(size_t)n + (size_t)j].data(), d, src)));
	return 0;
}
