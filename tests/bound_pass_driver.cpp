// Driver of tests/test_bound_pass_host.py: the host quantizer of the 8-bit bound pass (vk_bound_host.h, which vk_pack_query calls for
// the query's rows) and nothing else.  stdin: whitespace-separated numbers, floats as the hexadecimal of their bits; stdout the same.
// The expected values are computed in the test, never here.
#include "bound_driver.h"

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "quantize") {   // n, d, then n rows of d floats: per row "s e n a" and the d quantized values
		const int n = (int)read_i64(), d = (int)read_i64();
		std::vector<float> x((size_t)d);
		std::vector<int8_t> xq((size_t)d);
		for (int r = 0; r < n; r++) {
			for (auto &v : x) v = read_f32();
			const vk_host::quant_meta m = vk_host::quantize_row_i8(x.data(), d, xq.data());
			printf("%08x %08x %08x %08x", bits_of(m.s), bits_of(m.e), bits_of(m.n), bits_of(m.a));
			for (const int8_t v : xq) printf(" %d", (int)v);
			printf("\n");
		}
	} else if (what == "constants") {   // n, then n x (s e n a N X d_pad): cs ca cb
		const int n = (int)read_i64();
		for (int r = 0; r < n; r++) {
			vk_host::quant_meta m;
			m.s = read_f32(); m.e = read_f32(); m.n = read_f32(); m.a = read_f32();
			const float N = read_f32(), X = read_f32();
			const int d_pad = (int)read_i64();
			float cs, ca, cb;
			vk_host::bound_cell_constants(m, N, X, d_pad, &cs, &ca, &cb);
			printf("%08x %08x %08x\n", bits_of(cs), bits_of(ca), bits_of(cb));
		}
	} else if (what == "backoff") {   // n, then n flags "this query's bound pass falls back (if it runs)": per query 1 = a bound pass ran
		const int n = (int)read_i64();
		vk_host::bound_backoff b;
		for (int i = 0; i < n; i++) {
			const bool fell = read_i64() != 0;
			const bool took = b.take();
			if (took) b.record(fell);
			printf("%d\n", took ? 1 : 0);
		}
	} else {
		const int rc = format_commands(what);   // "format", "query_tile" (bound_driver.h)
		return rc < 0 ? 1 : rc;
	}
	return 0;
}
