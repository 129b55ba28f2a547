// Driver of tests/test_bound_compact_host.py: the host side of the compact 6-bit shadow (vk_bound_host.h: the format, the quantizer
// under bf16_meta, the packer of a compact tile) and nothing else.  stdin: whitespace-separated numbers, floats as the hexadecimal of
// their bits; stdout the same.  The expected values are computed in the test, never here.
#include "bound_driver.h"

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "quantize") {   // n, d, then n rows of d floats: per row "s e n a" and the d codes, under bf16_meta
		const int n = (int)read_i64(), d = (int)read_i64();
		std::vector<float> x((size_t)d);
		std::vector<uint8_t> xq((size_t)d);
		for (int r = 0; r < n; r++) {
			for (auto &v : x) v = read_f32();
			const vk_host::quant_meta m = vk_host::quantize_row_e2m3(x.data(), d, xq.data(), true);
			printf("%08x %08x %08x %08x", bits_of(m.s), bits_of(m.e), bits_of(m.n), bits_of(m.a));
			for (const uint8_t v : xq) printf(" %d", (int)v);
			printf("\n");
		}
	} else if (what == "tile") {   // the factory's arguments, then 16 rows of d floats: the bytes of the compact tile; then "N X"
		const vk_host::shadow_format f = read_format();
		if (!f.compact) return 2;
		std::vector<float> x((size_t)f.d);
		std::vector<uint8_t> xq((size_t)f.d), tile((size_t)f.tile_bytes(), 0xa5);   // every byte is stored: none of these may be left
		float N = 0.0f, X = 0.0f;
		for (int i = 0; i < 16; i++) {
			for (auto &v : x) v = read_f32();
			const vk_host::quant_meta m = vk_host::quantize_row_e2m3(x.data(), f.d, xq.data(), true);
			vk_host::fp6c_put_row(tile.data(), i, xq.data(), f.d);
			const uint32_t w = vk_host::fp6c_meta(m.s, m.e);
			memcpy(tile.data() + f.meta_offset() + 4 * i, &w, 4);
			N = m.n > N ? m.n : N; X = m.a > X ? m.a : X;
		}
		for (const uint8_t b : tile) printf("%d ", (int)b);
		printf("\n%08x %08x\n", bits_of(N), bits_of(X));
	} else {
		const int rc = format_commands(what);   // "format", "query_tile" (bound_driver.h)
		return rc < 0 ? 1 : rc;
	}
	return 0;
}
