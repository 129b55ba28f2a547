// sim_ops_driver.cpp -- a stand-alone driver of vectorian_amd/csrc/vk_sim_ops_host.h for tests/test_sim_ops_host.py (CPU tier).
//   apply:  stdin "n kind arg kind arg ...", then one float per line as the hex of its bits; prints the chain's value the same way
//   check:  stdin "n kind argbits kind argbits ..."; prints the status of vk_host::sim_ops_check and the offending operator
// Host only; built with g++ under AddressSanitizer and UBSan.
#include "vk_sim_ops_host.h"

#include <cstdio>
#include <cstring>
#include <string>

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	int n = 0;
	if (scanf("%d", &n) != 1) return 2;
	if (what == "check") {
		// more operators than the struct holds are legal input here: the check must refuse them without reading past anything
		int32_t kinds[64];
		float args[64];
		if (n > 64) return 2;
		for (int i = 0; i < n; i++) {
			uint32_t bits;
			if (scanf("%d %x", &kinds[i], &bits) != 2) return 2;
			args[i] = from_bits(bits);
		}
		int bad = 0;
		const int rc = vk_host::sim_ops_check(kinds, args, n, &bad);
		printf("%d %d\n", rc, bad);
		return 0;
	}
	if (what != "apply" || n < 0 || n > VK_MAX_SIM_OPS) return 2;
	vk_host::sim_ops ops{};
	ops.n = n;
	for (int i = 0; i < n; i++) {
		uint32_t bits;
		if (scanf("%d %x", &ops.kind[i], &bits) != 2) return 2;
		ops.arg[i] = from_bits(bits);
	}
	uint32_t u;
	while (scanf("%x", &u) == 1) printf("%08x\n", to_bits(vk_host::sim_ops_apply(from_bits(u), ops)));
	return 0;
}
