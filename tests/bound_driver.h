// Shared by tests/bound_pass_driver.cpp and tests/bound6_driver.cpp: reading numbers from stdin (floats as the hexadecimal of their
// bits) and the two commands both drivers answer -- the format of a shadow and the query's bound tile (vk_bound_host.h).
#include "vk_bound_host.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>

static uint32_t read_u32() { uint32_t u = 0; if (scanf("%" SCNx32, &u) != 1) exit(2); return u; }
static int64_t read_i64() { int64_t v = 0; if (scanf("%" SCNd64, &v) != 1) exit(2); return v; }
static float read_f32() { const uint32_t u = read_u32(); float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
// d, nk32, tail, precision, layout, bits wanted: the arguments of the factory
static vk_host::shadow_format read_format() {
	const int d = (int)read_i64(), nk32 = (int)read_i64(), tail = (int)read_i64(), prec = (int)read_i64(), layout = (int)read_i64();
	return vk_host::shadow_format_of(d, nk32, tail, prec, layout, (int)read_i64());
}

// "format": n, then n x the factory's arguments: bits steps step_features live tile_bytes meta_offset qtile_bytes gamma_width, or "none"
// "query_tile": the factory's arguments, len_t, N, X, then len_t rows of d floats: "none", or the tile's bytes and cs[16] ca[16] cb[16]
// Returns -1 when `what` is neither, else the exit code.
static int format_commands(const std::string &what) {
	if (what == "format") {
		const int n = (int)read_i64();
		for (int r = 0; r < n; r++) {
			const vk_host::shadow_format f = read_format();
			if (f.bits == 0) printf("none\n");
			else printf("%d %d %d %d %d %d %d %d\n", f.bits, f.steps, f.step_features, f.live, f.tile_bytes(), f.meta_offset(), f.qtile_bytes(), f.gamma_width);
		}
		return 0;
	}
	if (what != "query_tile") return -1;
	const vk_host::shadow_format f = read_format();
	const int len_t = (int)read_i64();
	const float N = read_f32(), X = read_f32();
	if (f.bits == 0 || len_t < 0 || len_t > 16) return 2;
	std::vector<float> rows((size_t)len_t * f.d);
	for (auto &v : rows) v = read_f32();
	std::vector<uint8_t> out;
	if (!vk_host::pack_bound_query(f, rows.data(), len_t, N, X, out)) {
		printf("none\n");
		return out.empty() ? 0 : 3;
	}
	if (out.size() != (size_t)f.qtile_bytes() + 192) return 3;
	for (int b = 0; b < f.qtile_bytes(); b++) printf("%d ", (int)out[(size_t)b]);
	printf("\n");
	for (int j = 0; j < 48; j++) {
		float v;
		memcpy(&v, &out[(size_t)f.qtile_bytes() + 4 * (size_t)j], 4);
		printf("%08x ", bits_of(v));
	}
	printf("\n");
	return 0;
}
