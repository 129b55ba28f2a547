// Driver of tests/test_result_host.py: vk_result_host.h (vectorian_amd/csrc) and nothing else.  argv[1] names the rule; the inputs come
// on stdin as whitespace-separated numbers, floats as the hexadecimal of their bits, and the answers go to stdout the same way, so that
// the test compares bit patterns.  The expected values are computed in the test, never here.
#include "vk_result_host.h"

#include <cinttypes>
#include <cstdio>
#include <string>

static uint32_t read_u32() { uint32_t u = 0; if (scanf("%" SCNx32, &u) != 1) exit(2); return u; }
static uint64_t read_u64() { uint64_t v = 0; if (scanf("%" SCNu64, &v) != 1) exit(2); return v; }
static int64_t read_i64() { int64_t v = 0; if (scanf("%" SCNd64, &v) != 1) exit(2); return v; }
static float read_f32() { const uint32_t u = read_u32(); float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "codec") {   // n, then n keys (decimal): score bits and row of each; then the count up to the first 0; then the key of each row
		const int n = (int)read_i64();
		std::vector<uint64_t> keys((size_t)n);
		for (auto &k : keys) k = read_u64();
		for (const uint64_t k : keys) printf("%08x %u\n", bits_of(vk_host::key_score(k)), vk_host::key_row(k));
		printf("count %d\n", vk_host::count_keys(keys.data(), n));
		for (const uint64_t k : keys) printf("%" PRIu64 "\n", vk_host::key_of_row((int64_t)vk_host::key_row(k)));
	} else if (what == "rank") {   // min_score, n, then n (score, slice): the positions in the order of the result set
		const float min_score = read_f32();
		const int n = (int)read_i64();
		std::vector<float> score((size_t)n);
		std::vector<int64_t> slice((size_t)n);
		std::vector<int> order((size_t)n);
		for (int i = 0; i < n; i++) { score[(size_t)i] = read_f32(); slice[(size_t)i] = read_i64(); order[(size_t)i] = i; }
		vk_host::rank_above(order, min_score, [&](int i) { return score[(size_t)i]; }, [&](int i) { return slice[(size_t)i]; });
		for (const int i : order) printf("%d\n", i);
	} else if (what == "score") {   // n cases: raw, total, submatch weight, boost, len_t, tag weights? (0 / 1), len_t mappings, len_t weights
		const int n = (int)read_i64();
		for (int c = 0; c < n; c++) {
			const float raw = read_f32(), total = read_f32(), w = read_f32(), boost = read_f32();
			const int len_t = (int)read_i64(), tagged = (int)read_i64();
			std::vector<int16_t> map((size_t)len_t);
			std::vector<float> tw((size_t)len_t);
			for (auto &m : map) m = (int16_t)read_i64();
			for (auto &t : tw) t = read_f32();
			printf("%08x\n", bits_of(vk_host::reference_score(raw, map.data(), len_t, tagged ? tw.data() : nullptr, total, w, boost)));
		}
	} else if (what == "no_flow") {   // len_t: a winner's rows filled over junk, with a guard element on either side
		const int len_t = (int)read_i64();
		std::vector<int16_t> map((size_t)len_t + 2, 7);
		std::vector<float> sim((size_t)len_t + 2, 7.0f);
		vk_host::no_flow(map.data() + 1, sim.data() + 1, len_t);
		for (int j = 0; j < len_t + 2; j++) printf("%d %08x\n", map[(size_t)j], bits_of(sim[(size_t)j]));
	} else if (what == "gaps") {   // n pairs: (kind, u, v) of s and of t
		const int n = (int)read_i64();
		for (int c = 0; c < n; c++) {
			vk_gap g[2] = {};
			for (auto &x : g) { x.kind = (int32_t)read_i64(); x.u = read_f32(); x.v = read_f32(); }
			const vk_host::gap_form f = vk_host::classify_gaps(g[0], g[1]);
			printf("%d %08x %08x %08x %08x %08x %08x\n", f.gap_mode, bits_of(f.gs), bits_of(f.gt), bits_of(f.a_s), bits_of(f.a_t), bits_of(f.open_s), bits_of(f.open_t));
		}
	} else if (what == "closure") {   // len_t, is_align, n_table, the table: wt[0..159]
		const int len_t = (int)read_i64(), is_align = (int)read_i64(), n_table = (int)read_i64();
		std::vector<float> table((size_t)n_table);
		for (auto &t : table) t = read_f32();
		vk_gap g = {};
		g.kind = VK_GAP_TABLE; g.table = table.data(); g.n_table = n_table;
		float wt[160];
		vk_host::wt_with_closure(wt, g, len_t, is_align != 0);
		for (const float x : wt) printf("%08x\n", bits_of(x));
	} else return 2;
	return 0;
}
