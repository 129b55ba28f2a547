// Driver of tests/test_bound6_host.py: the host side of the 6-bit bound pass (vk_bound_host.h: the E2M3 quantizer and the packer of a
// lane's operand, which vk_pack_query calls for the query's rows) and nothing else.  stdin: whitespace-separated numbers, floats as the
// hexadecimal of their bits; stdout the same.  The expected values are computed in the test, never here.
#include "bound_driver.h"

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "decode") {   // 8 x the value of each of the 64 codes
		for (int code = 0; code < 64; code++) printf("%d\n", vk_host::e2m3_eighths(code));
	} else if (what == "quantize") {   // n, d, then n rows of d floats: per row "s e n a" and the d codes
		const int n = (int)read_i64(), d = (int)read_i64();
		std::vector<float> x((size_t)d);
		std::vector<uint8_t> xq((size_t)d);
		for (int r = 0; r < n; r++) {
			for (auto &v : x) v = read_f32();
			const vk_host::quant_meta m = vk_host::quantize_row_e2m3(x.data(), d, xq.data());
			printf("%08x %08x %08x %08x", bits_of(m.s), bits_of(m.e), bits_of(m.n), bits_of(m.a));
			for (const uint8_t v : xq) printf(" %d", (int)v);
			printf("\n");
		}
	} else if (what == "pack") {   // live6, d, then 16 rows of d codes: the bytes of the tile's K-steps (2 x 1536 + 384 live6)
		const int live6 = (int)read_i64(), d = (int)read_i64();
		if (live6 < 1 || live6 > 4 || d < 0 || d > 256 + 32 * live6) return 2;
		std::vector<uint8_t> tile((size_t)(2 * 1536 + 384 * live6), 0), codes((size_t)d);
		for (int i = 0; i < 16; i++) {
			for (auto &v : codes) v = (uint8_t)read_i64();
			vk_host::fp6_put_row(tile.data(), live6, i, codes.data(), d);
		}
		for (const uint8_t b : tile) printf("%d ", (int)b);
		printf("\n");
	} else {
		const int rc = format_commands(what);   // "format", "query_tile" (bound_driver.h)
		return rc < 0 ? 1 : rc;
	}
	return 0;
}
