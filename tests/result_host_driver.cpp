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

// A caller's result set: `capacity` winners of len_t columns, every array (those the case leaves out: null) filled with 7s and with a
// guard element on either side.  print(): n_out, then every element of every array, guards included, one array per line.
struct out_arrays {
	std::vector<float> score, raw, sim;
	std::vector<int64_t> sentence;
	std::vector<int16_t> map;
	vk_topk_out out = {};
	out_arrays(int capacity, int len_t, bool has_raw, bool has_map, bool has_sim)
		: score((size_t)capacity + 2, 7.0f), raw((size_t)capacity + 2, 7.0f), sim((size_t)capacity * len_t + 2, 7.0f), sentence((size_t)capacity + 2, 7),
		  map((size_t)capacity * len_t + 2, 7) {
		out.capacity = capacity; out.n_out = -1;
		out.score = score.data() + 1; out.sentence = sentence.data() + 1;
		out.raw_score = has_raw ? raw.data() + 1 : nullptr; out.mapping = has_map ? map.data() + 1 : nullptr; out.edge_sim = has_sim ? sim.data() + 1 : nullptr;
	}
	void print() const {
		printf("%d\n", out.n_out);
		for (const float x : score) printf("%08x ", bits_of(x));
		printf("\n");
		for (const int64_t x : sentence) printf("%" PRId64 " ", x);
		printf("\n");
		for (const float x : raw) printf("%08x ", bits_of(x));
		printf("\n");
		for (const int16_t x : map) printf("%d ", x);
		printf("\n");
		for (const float x : sim) printf("%08x ", bits_of(x));
		printf("\n");
	}
};
static std::vector<float> read_floats(size_t n) { std::vector<float> v(n); for (auto &x : v) x = read_f32(); return v; }
static std::vector<int32_t> read_table() { std::vector<int32_t> t((size_t)read_i64()); for (auto &x : t) x = (int32_t)read_i64(); return t; }

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "unboosted") {   // n, len_t, n boosts (0: none), then n x (score, slice): the aligner score behind each score of the batched pass
		const int n = (int)read_i64(), len_t = (int)read_i64();
		const std::vector<float> boost = read_floats((size_t)read_i64());
		for (int i = 0; i < n; i++) {
			const float s = read_f32();
			printf("%08x\n", bits_of(vk_host::unboosted_sum(s, boost.empty() ? nullptr : boost.data(), read_i64(), len_t)));
		}
		return 0;
	}
	if (what == "floor") {   // n, then n min_scores: the margin, then the lowered floor of each
		const int n = (int)read_i64();
		printf("%d\n", vk_host::kCanonMargin);
		for (int i = 0; i < n; i++) printf("%08x\n", bits_of(vk_host::restated_floor(read_f32())));
		return 0;
	}
	if (what == "result") {
		// capacity len_t has_raw has_map has_sim flows | listed limit min_score | the row -> slice table (n, entries; 0: rows are slices) |
		// cap, then cap keys | restate: 0 as selected, 1 by traceback, 2 given | stride (0: no traceback came back)
		// stride > 0: cap raw, cap x stride map, cap x stride sim
		// restate 1: total, submatch weight, n tag weights + them (0: none), n boosts + them (0: none);  restate 2: cap raw, cap val
		// n_override, then that many aligner scores the caller states for the winners in place of the scored ones
		// -> n_out of score_selected, the order, then the arrays after write_result_set
		const int capacity = (int)read_i64(), len_t = (int)read_i64(), has_raw = (int)read_i64(), has_map = (int)read_i64(), has_sim = (int)read_i64(), flows = (int)read_i64();
		const int listed = (int)read_i64(), limit = (int)read_i64();
		const float min_score = read_f32();
		const std::vector<int32_t> table = read_table();
		const int cap = (int)read_i64();
		std::vector<uint64_t> keys((size_t)cap);
		for (auto &k : keys) k = read_u64();
		const int restate = (int)read_i64(), stride = (int)read_i64();
		vk_host::selected sel;
		sel.keys = keys.data(); sel.cap = cap; sel.slice_of_row = table.empty() ? nullptr : table.data();
		std::vector<float> raw, sim, given_raw, given_val, tw, boost;
		std::vector<int16_t> map;
		if (stride > 0) {
			raw = read_floats((size_t)cap);
			map.resize((size_t)cap * stride);
			for (auto &m : map) m = (int16_t)read_i64();
			sim = read_floats((size_t)cap * stride);
			sel.raw = raw.data(); sel.map = map.data(); sel.sim = sim.data(); sel.stride = stride;
		}
		out_arrays o(capacity, len_t, has_raw, has_map, has_sim);
		vk_host::result_set rs;
		int n_out;
		if (restate == 1) {
			const float total = read_f32(), w = read_f32();
			tw = read_floats((size_t)read_i64());
			boost = read_floats((size_t)read_i64());
			n_out = vk_host::score_selected(sel, rs, min_score, limit, listed != 0,
				vk_host::by_traceback{sel, len_t, tw.empty() ? nullptr : tw.data(), total, w, boost.empty() ? nullptr : boost.data()});
		} else if (restate == 2) {
			given_raw = read_floats((size_t)cap);
			given_val = read_floats((size_t)cap);
			n_out = vk_host::score_selected(sel, rs, min_score, limit, listed != 0, [&](int i) { return std::make_pair(given_raw[(size_t)i], given_val[(size_t)i]); });
		} else n_out = vk_host::score_selected(sel, rs, min_score, limit, listed != 0);
		const std::vector<float> stated = read_floats((size_t)read_i64());
		for (size_t j = 0; j < stated.size(); j++) rs.raw[(size_t)rs.order[j]] = stated[j];
		printf("%d\n", n_out);
		for (int i = 0; i < n_out; i++) printf("%d ", rs.order[(size_t)i]);
		printf("\n");
		vk_host::write_result_set(&o.out, sel, rs, len_t, flows != 0);
		o.print();
		return 0;
	}
	if (what == "keep_best") {
		// capacity len_t has_raw has_map has_sim flows | k min_score | table | n_rounds, each: n, then n x (val, raw, row, n_trace, n_trace map,
		// n_trace sim) -> after each round the rows kept, in order; then the arrays after write_best
		const int capacity = (int)read_i64(), len_t = (int)read_i64(), has_raw = (int)read_i64(), has_map = (int)read_i64(), has_sim = (int)read_i64(), flows = (int)read_i64();
		const int k = (int)read_i64();
		const float min_score = read_f32();
		const std::vector<int32_t> table = read_table();
		std::vector<vk_host::candidate> best, round;
		const int n_rounds = (int)read_i64();
		for (int r = 0; r < n_rounds; r++) {
			const int n = (int)read_i64();
			for (int i = 0; i < n; i++) {
				vk_host::candidate cd{};
				cd.val = read_f32(); cd.raw = read_f32(); cd.row = read_i64();
				const int n_trace = (int)read_i64();
				for (int j = 0; j < n_trace; j++) cd.map.push_back((int16_t)read_i64());
				cd.sim = read_floats((size_t)n_trace);
				round.push_back(std::move(cd));
			}
			vk_host::keep_best(best, round, min_score, k);
			if (!round.empty()) return 3;
			for (const auto &b : best) printf("%" PRId64 " ", b.row);
			printf("\n");
		}
		out_arrays o(capacity, len_t, has_raw, has_map, has_sim);
		vk_host::write_best(&o.out, best, table.empty() ? nullptr : table.data(), len_t, flows != 0);
		o.print();
		return 0;
	}
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
