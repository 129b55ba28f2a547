// sim_mix_driver.cpp -- a stand-alone driver of vectorian_amd/csrc/vk_sim_mix_host.h for tests/test_sim_mix_host.py (CPU tier).
//   cell:   stdin "kind n wbits_0 .. wbits_{n-1}" (the weights as the hex of their float64 bits), then per line the n cells of one
//           position as the hex of their float32 bits; prints vk_host::sim_mix_cell the same way
//   check:  stdin "kind n has_weights wbits ..." (with has_weights: as many weights as max(n, 0), at most 16); prints the status of vk_host::sim_mix_check
// Host only; built with g++ under AddressSanitizer and UBSan.
#include "vk_sim_mix_host.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static double from_bits64(uint64_t u) { double f; memcpy(&f, &u, 8); return f; }

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	int kind = 0, n = 0;
	if (scanf("%d %d", &kind, &n) != 2) return 2;
	if (what == "check") {
		int has = 0;
		if (scanf("%d", &has) != 1) return 2;
		// more weights than the struct holds are legal input here: the check must refuse the count without reading past anything
		double w[16];
		const int nw = n < 0 ? 0 : n;
		if (nw > 16) return 2;
		for (int i = 0; has && i < nw; i++) {
			uint64_t bits;
			if (scanf("%" SCNx64, &bits) != 1) return 2;
			w[i] = from_bits64(bits);
		}
		const char *why = nullptr;
		const int rc = vk_host::sim_mix_check(kind, n, has ? w : nullptr, &why);
		printf("%d %s\n", rc, why && *why ? "refused" : "-");
		return 0;
	}
	if (what != "cell" || n < 2 || n > VK_MAX_SIM_OPERANDS) return 2;
	vk_host::sim_mix mix{};
	mix.kind = kind; mix.n = n;
	for (int i = 0; i < n; i++) {
		uint64_t bits;
		if (scanf("%" SCNx64, &bits) != 1) return 2;
		mix.w[i] = from_bits64(bits);
	}
	for (;;) {
		float cells[VK_MAX_SIM_OPERANDS] = {0.0f, 0.0f, 0.0f, 0.0f};
		for (int i = 0; i < n; i++) {
			uint32_t u;
			if (scanf("%x", &u) != 1) return 0;
			cells[i] = from_bits(u);
		}
		printf("%08x\n", to_bits(vk_host::sim_mix_cell(cells, mix)));
	}
}
