// Driver of tests/test_contextual_cell_host.py: vk_host::contextual_cell (vectorian_amd/csrc/vk_sim_ops_host.h) and nothing else -- the
// similarity cell of a contextual handle under an operator chain, as the scoring epilogues and the restatement sites
// compile it for the device.
//   contextual_cell_driver cell   stdin: "n kind argbits ..." then lines of "in_query bits" (hex) -> the cell's bits, one per line
#include "vk_sim_ops_host.h"

#include <cstdio>
#include <cstring>
#include <string>

using namespace vk_host;

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv) {
	if (argc < 2 || std::string(argv[1]) != "cell") return 2;
	int n = 0;
	if (scanf("%d", &n) != 1 || n < 0 || n > VK_MAX_SIM_OPS) return 3;
	sim_ops ops{};
	ops.n = n;
	for (int i = 0; i < n; i++) {
		unsigned bits = 0;
		if (scanf("%d %x", &ops.kind[i], &bits) != 2) return 3;
		ops.arg[i] = from_bits(bits);
	}
	int in_query = 0;
	unsigned bits = 0;
	while (scanf("%d %x", &in_query, &bits) == 2) printf("%x\n", to_bits(contextual_cell(from_bits(bits), in_query != 0, ops)));
	return 0;
}
