// Driver of tests/test_route_chain_host.py: vk_route_host.h (vectorian_amd/csrc) under route_facts::chained -- a contextual handle under
// an operator chain.  The facts are enumerated as tests/route_driver.cpp enumerates them (contextual layout only), every
// switch on its own; the three LDS questions are restated as there.
//   route_chain_driver enumerate   every violated rule on a line of its own, then "points N refused M fused F multi_block B dropped_bound X dropped_span Y violations V"
#include "vk_route_host.h"

#include <cstdio>
#include <cstring>
#include <string>

using namespace vk_host;

static size_t score32_lds_bytes(int nk32, int tail, int tiles, int len_t, int gap_mode, int waves) {
	const int nb = len_t <= 32 ? 2 : 4, stride = (len_t + 3) / 4 * 4;
	const int slack = gap_mode == 7 ? 144 : (gap_mode == 3 || gap_mode == 6) ? 64 : 16;
	return (size_t)nb * (nk32 * 1024 - (tail && nk32 > 0 ? 512 : 0)) + (size_t)waves * ((size_t)tiles * 16 * stride + slack) * 4;
}
static int32_t score32_waves(int32_t nk32, int32_t tail, int32_t tiles, int32_t len_t, int32_t gap_mode) {
	for (int w = 4; w >= 1; w >>= 1)
		if (score32_lds_bytes(nk32, tail, tiles, len_t, gap_mode, w) <= 160 * 1024) return w;
	return 0;
}
static int32_t wide_ring_rows(int32_t nq, int32_t gap_mode, int32_t ws_tail) {
	if (gap_mode != 2 || ws_tail < 1) return 0;
	int ring = 16;
	while (ring < ws_tail + 1) ring <<= 1;
	return (size_t)ring * (16 * (size_t)nq + 2) * 4 <= 40 * 1024 ? ring : 0;
}
static size_t wide_lds_demand(int32_t max_len, int32_t nq, int32_t gap_mode, int32_t tagged, int32_t flow) {
	const size_t LQ = (size_t)nq * 16, W = LQ + 1, rows = (size_t)max_len + 1;
	size_t fl = 16 * LQ * (tagged ? 2 : 1) + (rows + 3) / 4 * 4 + LQ + 4 + 64 + 64;
	if (gap_mode == 2) fl += rows * W;
	size_t b = fl * 4;
	if (flow) b += 64 * 2 + rows * W * 2 + rows * W;
	b = (b + 15) / 16 * 16;
	if (flow) b += 8192;
	return b;
}
static const route_fits kFits{score32_waves, wide_ring_rows, wide_lds_demand};

static bool *switch_by_index(route_switches &s, int i) {
	bool *all[] = {&s.long_linear, &s.long_pass, &s.no_doc_mid, &s.no_doc_kernel, &s.no_doc_flow, &s.no_docw, &s.no_docg, &s.no_doc_rwmd,
		&s.no_doc_general, &s.keep_raw, &s.no_apart, &s.no_score32};
	return i >= 0 && i < 12 ? all[i] : nullptr;
}

static bool same(const query_route &a, const query_route &b) {
	return a.status == b.status && a.fits32 == b.fits32 && a.gap_mode == b.gap_mode && a.wide_gap_mode == b.wide_gap_mode && a.score32_gap_mode == b.score32_gap_mode &&
		a.wave_tiles == b.wave_tiles && a.plan == b.plan && a.pass[0] == b.pass[0] && a.pass[1] == b.pass[1] && a.pass[2] == b.pass[2] && a.wide_pass == b.wide_pass &&
		a.list == b.list && a.ring_rows == b.ring_rows && a.wide_lds_score == b.wide_lds_score && a.wide_lds_flow == b.wide_lds_flow && a.flow == b.flow &&
		a.ostride == b.ostride && a.raw == b.raw && a.span_skip_raw == b.span_skip_raw;
}

static long violations = 0;
static void violated(const char *what, const route_facts &f, int sw, const query_route &r) {
	if (++violations > 40) return;
	printf("VIOLATED %s: prec %d nk32 %d max_len %d mid %d alg %d full %d inj %d len_t %d gap %d a_t %g only %d flow %d bound %d uniform %d switch %d -> plan %d pass %d %d %d status %d\n",
		what, f.prec, f.nk32, f.max_len, f.n_long_groups, f.algorithm, (int)f.wmd_full, (int)f.rwmd_injective, f.len_t, f.gaps.gap_mode, f.gaps.a_t,
		(int)f.only, (int)f.want_flow, (int)f.bound_pass, f.uniform_len, sw, r.plan, r.pass[0], r.pass[1], r.pass[2], r.status);
}

int main(int argc, char **argv) {
	if (argc < 2 || std::string(argv[1]) != "enumerate") return 2;
	struct shape { int max_len, max_short_len, n_long_groups; bool apart, xlong; int pair, short_pair, uniform; };
	const shape shapes[] = {{64, 64, 0, false, false, 9, 9, 0}, {30, 30, 0, false, false, 5, 5, 0}, {512, 64, 3, true, false, 33, 9, 0}, {5000, 64, 3, true, true, 314, 9, 0},
		{600, 64, 0, true, true, 39, 9, 0}, {1, 1, 0, false, false, 1, 1, 1}};
	const int widths[][2] = {{2, 0}, {10, 1}, {19, 0}, {24, 0}, {48, 0}}, lens[] = {1, 16, 17, 32, 33, 48, 64};
	struct form { int algorithm; bool full, inj; };
	const form forms[] = {{VK_ALG_ALIGN, false, false}, {VK_ALG_RWMD, false, true}, {VK_ALG_RWMD, false, false}, {VK_ALG_RWMD, true, false}, {VK_ALG_WRD, false, false}};
	struct gaps { int mode; float a_t; int tail; };
	const gaps families[] = {{0, 0.0f, 0}, {1, 0.2f, 0}, {1, -0.05f, 0}, {2, 0.0f, 0}, {2, 0.0f, 1}, {2, 0.0f, 126}, {2, 0.0f, 127}};
	long points = 0, refused = 0, fused = 0, multi = 0, dropped_bound = 0, dropped_span = 0;
	for (int prec = 0; prec < 2; prec++) for (const auto &w : widths) for (const shape &sh : shapes)
	for (const int len_t : lens) for (const form &fo : forms) for (const gaps &g : families) for (int flags = 0; flags < 32; flags++) {
		if (fo.algorithm != VK_ALG_ALIGN && &g != &families[0]) continue;
		route_facts f;
		f.layout = VK_LAYOUT_CONTEXTUAL; f.prec = prec; f.nk32 = w[0]; f.tail = w[1];
		f.max_len = sh.max_len; f.max_short_len = sh.max_short_len; f.n_long_groups = sh.n_long_groups; f.has_apart = sh.apart; f.has_xlong = sh.xlong;
		f.max_pair_tiles = sh.pair; f.max_short_pair_tiles = sh.short_pair; f.uniform_len = sh.uniform; f.has_pos = true; f.n_sentences = 1000;
		f.algorithm = fo.algorithm; f.wmd_full = fo.full; f.rwmd_injective = fo.inj; f.len_t = len_t;
		if (fo.algorithm == VK_ALG_ALIGN) { f.gaps.gap_mode = g.mode; f.gaps.a_t = g.a_t; f.ws_tail = g.tail < sh.max_len ? g.tail : 0; }
		f.only = flags & 1; f.want_flow = flags & 2; f.submatch = flags & 4; f.tagged = flags & 8; f.bound_pass = flags & 16;
		f.kk = 10; f.raw_score = true; f.locality = VK_LOCAL;
		if (sh.xlong && !(fo.algorithm == VK_ALG_ALIGN || (fo.algorithm == VK_ALG_RWMD && !fo.full && fo.inj))) continue;
		if (f.only && !f.want_flow) continue;
		if (f.submatch && fo.algorithm != VK_ALG_ALIGN) continue;
		for (int sw = -1; sw < 12; sw++) {
			route_switches s;
			if (sw >= 0) *switch_by_index(s, sw) = true;
			route_facts fc = f; fc.chained = true;
			const query_route r = route_query(fc, s, kFits);
			const query_route plain = route_query(f, s, kFits);
			// what the scoring passes of this shape would be, only_slices aside: the rule of the refusal reads these
			route_facts fs = f; fs.only = false;
			const query_route scored = route_query(fs, s, kFits);
			points++;
			bool expect = scored.status != VK_OK;
			for (int k = 0; k < 3 && !expect; k++)
				expect = scored.pass[k] != PASS_NONE && scored.pass[k] != PASS_FUSED && scored.pass[k] != PASS_SCORE32 && scored.pass[k] != PASS_SPAN;
			if ((r.status != VK_OK) != expect) violated("refusal", fc, sw, r);
			if (r.status != VK_OK) {
				refused++;
				if (r.status != VK_ERR_UNSUPPORTED || !r.message || !strstr(r.message, "operator chain") || !strstr(r.message, "vk_corpus_set_contextual_sim_ops")) violated("message", fc, sw, r);
				continue;
			}
			if (r.plan == PLAN_BOUNDED || r.plan == PLAN_SPAN) violated("plan", fc, sw, r);
			for (int k = 0; k < 3; k++)
				if (r.pass[k] != PASS_NONE && r.pass[k] != PASS_FUSED && r.pass[k] != PASS_SCORE32) violated("pass", fc, sw, r);
			if (r.wide_pass != PASS_NONE || r.list != LIST_NONE) violated("list pass", fc, sw, r);
			// every field is the unchained answer's, but for the plan where the bound pass or the span kernel was dropped
			query_route x = plain;
			if (x.plan == PLAN_BOUNDED) { x.plan = PLAN_FUSED; dropped_bound++; }
			if (x.plan == PLAN_SPAN) { x.plan = PLAN_FUSED; x.pass[CLASS_SHORT] = PASS_FUSED; dropped_span++; }
			x.span_skip_raw = false;   // (the span kernel's own field: read by nothing else, set for a span-shaped query even under only_slices)
			if (!same(r, x)) violated("fields", fc, sw, r);
			if (r.plan == PLAN_FUSED) fused++;
			if (r.plan == PLAN_MULTI_BLOCK) multi++;
		}
	}
	// a query of more than VK_MAX_QUERY_LEN tokens (vk_validate_query asks for such a handle): refused by name; without a chain never asked
	{
		route_facts f; f.chained = true; f.len_t = VK_MAX_QUERY_LEN + 1; f.max_len = 30; f.max_short_len = 30; f.nk32 = 2;
		const query_route r = route_query(f, route_switches{}, kFits);
		if (r.status != VK_ERR_UNSUPPORTED || !strstr(r.message, "more than 64 tokens")) violated("long query", f, -1, r);
	}
	printf("points %ld refused %ld fused %ld multi_block %ld dropped_bound %ld dropped_span %ld violations %ld\n", points, refused, fused, multi, dropped_bound, dropped_span, violations);
	return 0;
}
