// Driver of tests/test_route_host.py: vk_route_host.h (vectorian_amd/csrc) and nothing else.  The three LDS questions are restated here
// from vk_score32_lds_bytes (vk_score32.hip) and vk_wide_ring_rows / vk_wide_lds_bytes (vk_flow.hip); tests/test_abi.py holds the
// library's own exports.
//   route_driver route      facts and switches of one query per line on stdin -> its route, one line each
//   route_driver enumerate  a grid of facts; every violated invariant on a line of its own, then "points N refused M"
#include "vk_route_host.h"

#include <cstdio>
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
	if (flow) b += 8192;   // VK_CANON_LDS
	return b;
}
static const route_fits kFits{score32_waves, wide_ring_rows, wide_lds_demand};

static bool *switch_by_index(route_switches &s, int i) {
	bool *all[] = {&s.long_linear, &s.long_pass, &s.no_doc_mid, &s.no_doc_kernel, &s.no_doc_flow, &s.no_docw, &s.no_docg, &s.no_doc_rwmd,
		&s.no_doc_general, &s.keep_raw, &s.no_apart, &s.no_score32};
	return i >= 0 && i < 12 ? all[i] : nullptr;
}
enum { SW_LONG_LINEAR, SW_LONG_PASS, SW_NO_DOC_MID, SW_NO_DOC_KERNEL, SW_NO_DOC_FLOW, SW_NO_DOCW, SW_NO_DOCG, SW_NO_DOC_RWMD, SW_NO_DOC_GENERAL,
	SW_KEEP_RAW, SW_NO_APART, SW_NO_SCORE32, SW_COUNT };

static void print_route(const query_route &r) {
	printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d status %d fits32 %d wide_pass %d\n", r.plan, r.gap_mode, r.wide_gap_mode, r.score32_gap_mode, r.wave_tiles,
		r.pass[0], r.pass[1], r.pass[2], r.list, r.ring_rows, r.flow, r.ostride, (int)r.raw, (int)r.span_skip_raw, r.status, (int)r.fits32, r.wide_pass);
}

static bool same(const query_route &a, const query_route &b) {
	return a.status == b.status && a.fits32 == b.fits32 && a.gap_mode == b.gap_mode && a.wide_gap_mode == b.wide_gap_mode && a.score32_gap_mode == b.score32_gap_mode &&
		a.wave_tiles == b.wave_tiles && a.plan == b.plan && a.pass[0] == b.pass[0] && a.pass[1] == b.pass[1] && a.pass[2] == b.pass[2] && a.wide_pass == b.wide_pass &&
		a.list == b.list && a.ring_rows == b.ring_rows && a.wide_lds_score == b.wide_lds_score && a.wide_lds_flow == b.wide_lds_flow && a.flow == b.flow &&
		a.ostride == b.ostride && a.raw == b.raw && a.span_skip_raw == b.span_skip_raw;
}
static bool names(const query_route &r, route_pass pass, route_flow flow) {
	return r.pass[0] == pass || r.pass[1] == pass || r.pass[2] == pass || r.wide_pass == pass || r.flow == flow;
}
static bool is_wide_family(route_pass p) { return p == PASS_DOC || p == PASS_DOCW || p == PASS_DOCG || p == PASS_WIDE; }

// vk_validate_query's rule before the route existed (score32_plan of the parent commit, restated): the shapes it refused for their LDS
static bool parent_refuses(const route_facts &f, bool no_apart) {
	const bool exact = f.algorithm == VK_ALG_WRD || (f.algorithm == VK_ALG_RWMD && f.wmd_full);
	const bool in_lds = exact || (f.algorithm == VK_ALG_RWMD && !f.rwmd_injective);
	if (!(f.len_t > VK_FAST_QUERY_LEN && in_lds)) return false;
	const bool fill = f.algorithm == VK_ALG_RWMD && !f.wmd_full && !f.rwmd_injective;
	int gm = exact ? 5 : fill ? 7 : f.algorithm == VK_ALG_RWMD ? 4 : f.gaps.gap_mode == 2 ? -1 : f.gaps.gap_mode;
	const bool apart = (f.algorithm == VK_ALG_ALIGN || gm == 4) && f.has_apart && !no_apart;
	if (gm < 0) gm = (apart ? f.max_short_len : f.max_len) <= 32 ? 3 : 6;
	const bool long_apart = ((exact || fill) && f.n_long_groups > 0) || apart;
	const int wave_tiles = long_apart ? (f.len_t <= 32 ? f.max_short_pair_tiles : (f.max_short_len + 15) / 16 + 1) : (f.len_t <= 32 ? f.max_pair_tiles : (f.max_len + 15) / 16 + 1);
	return score32_waves(f.layout == VK_LAYOUT_STATIC ? 0 : f.nk32, f.tail, wave_tiles, f.len_t, gm) < 1;
}

static long violations = 0;
static void violated(const char *what, const route_facts &f, int sw, const query_route &r) {
	if (++violations > 40) return;
	printf("VIOLATED %s: layout %d prec %d nk32 %d max_len %d mid %d alg %d full %d inj %d len_t %d gap %d a_t %g tail %d only %d flow %d sub %d tagged %d switch %d -> ",
		what, f.layout, f.prec, f.nk32, f.max_len, f.n_long_groups, f.algorithm, (int)f.wmd_full, (int)f.rwmd_injective, f.len_t, f.gaps.gap_mode, f.gaps.a_t, f.ws_tail,
		(int)f.only, (int)f.want_flow, (int)f.submatch, (int)f.tagged, sw);
	print_route(r);
}

static void check_point(const route_facts &f, long &points, long &refused) {
	const query_route r0 = route_query(f, route_switches{}, kFits);
	const bool exact = exact_transport(f.algorithm, f.wmd_full), fill = f.algorithm == VK_ALG_RWMD && !f.wmd_full && !f.rwmd_injective;
	const bool rwmd = f.algorithm == VK_ALG_RWMD, wide_query = f.len_t > VK_FAST_QUERY_LEN;
	for (int sw = -1; sw < SW_COUNT; sw++) {
		route_switches s;
		if (sw >= 0) *switch_by_index(s, sw) = true;
		const query_route r = route_query(f, s, kFits);
		points++;
		// (c) the refusal is the validator's
		if ((r.status != VK_OK) != parent_refuses(f, s.no_apart)) violated("c refusal", f, sw, r);
		if (r.status != VK_OK) { refused++; if (r.status != VK_ERR_UNSUPPORTED || r.fits32) violated("c status", f, sw, r); continue; }
		// (a) one scoring plan, and the pass of the slices of at most 64 tokens is that plan's kernel
		const route_pass of_plan[] = {PASS_NONE, PASS_SPAN, PASS_FUSED, PASS_FUSED, PASS_SCORE32, PASS_DOCW, PASS_DOCG, PASS_WIDE};
		if (r.pass[CLASS_SHORT] != of_plan[r.plan] || (r.plan == PLAN_LISTED) != f.only) violated("a plan", f, sw, r);
		if ((r.plan == PLAN_FUSED || r.plan == PLAN_BOUNDED || r.plan == PLAN_SPAN) && wide_query) violated("a fused kernel, wide query", f, sw, r);
		if (r.plan >= PLAN_MULTI_BLOCK && !wide_query) violated("a wide plan, short query", f, sw, r);
		// (b) every class of slices the corpus holds has one pass, no other class has one
		const bool present[3] = {true, f.n_long_groups > 0, f.max_len > VK_MAX_SENT_LEN};
		bool any_wide = false;
		for (int k = 0; k < 3; k++) {
			if ((r.pass[k] != PASS_NONE) != (present[k] && !f.only)) violated("b class", f, sw, r);
			if (is_wide_family(r.pass[k])) { any_wide = true; if (r.pass[k] != r.wide_pass) violated("b two kernels over one list", f, sw, r); }
		}
		if (any_wide != (r.wide_pass != PASS_NONE)) violated("b wide pass", f, sw, r);
		if ((r.list == LIST_APART && !f.has_apart) || (r.list == LIST_XLONG && !f.has_xlong) || (r.list != LIST_NONE && !any_wide)) violated("b list", f, sw, r);
		if (r.list == LIST_XLONG && is_wide_family(r.pass[CLASS_MID])) violated("b mid slices on the list of documents", f, sw, r);
		if (any_wide && r.plan < PLAN_DOCW_ALL && r.list != LIST_APART && r.list != LIST_XLONG) violated("b pass without its list", f, sw, r);
		if (r.plan >= PLAN_DOCW_ALL && (r.list == LIST_APART || r.list == LIST_XLONG)) violated("b every row, but a list", f, sw, r);
		if (r.pass[CLASS_MID] == PASS_LONG_RWMD_FILL && !fill) violated("b fill", f, sw, r);
		if (r.pass[CLASS_MID] == PASS_LONG_BOUND && !exact) violated("b bound", f, sw, r);
		// (e) the stride of the winners' arrays
		if ((r.ostride == 64) != (r.flow != FLOW_NARROW) || (r.ostride != 64 && r.ostride != 16)) violated("e ostride", f, sw, r);
		// gap modes: the register-history forms belong to the fused and the multi-block kernel
		if (r.wide_gap_mode == 3 || r.wide_gap_mode == 6 || ((r.gap_mode == 3 || r.gap_mode == 6) && wide_query)) violated("gap mode", f, sw, r);
		// (d) a switch takes its kernel out and leaves the rest
		if (sw < 0) continue;
		if (r.gap_mode != r0.gap_mode || r.wide_gap_mode != r0.wide_gap_mode || r.status != r0.status) violated("d gap modes", f, sw, r);
		if (sw != SW_NO_APART && (r.score32_gap_mode != r0.score32_gap_mode || r.wave_tiles != r0.wave_tiles || r.fits32 != r0.fits32)) violated("d score32", f, sw, r);
		if (sw != SW_KEEP_RAW && (r.raw != r0.raw || r.span_skip_raw != r0.span_skip_raw)) violated("d raw", f, sw, r);
		const bool doc0 = names(r0, PASS_DOC, FLOW_DOC), docw0 = names(r0, PASS_DOCW, FLOW_DOCW), docg0 = names(r0, PASS_DOCG, FLOW_DOCG);
		switch (sw) {
		case SW_NO_DOCW: if (names(r, PASS_DOCW, FLOW_DOCW) || (!docw0 && !same(r, r0))) violated("d VK_NO_DOCW", f, sw, r); break;
		case SW_NO_DOCG: if (names(r, PASS_DOCG, FLOW_DOCG) || (!docg0 && !same(r, r0))) violated("d VK_NO_DOCG", f, sw, r); break;
		case SW_NO_DOC_KERNEL: if (names(r, PASS_DOC, (route_flow)-1) || (!doc0 && !same(r, r0))) violated("d VK_NO_DOC_KERNEL", f, sw, r); break;
		case SW_NO_DOC_FLOW: if ((r.flow == FLOW_DOC && r.wide_pass != PASS_DOC && !f.only && f.max_len <= VK_MAX_SENT_LEN) || (!doc0 && !same(r, r0))) violated("d VK_NO_DOC_FLOW", f, sw, r); break;
		case SW_NO_DOC_MID: if (r.pass[CLASS_MID] == PASS_DOC && !rwmd && f.max_len <= VK_MAX_SENT_LEN) violated("d VK_NO_DOC_MID", f, sw, r); if (!doc0 && !same(r, r0)) violated("d VK_NO_DOC_MID rest", f, sw, r); break;
		case SW_NO_DOC_RWMD: if ((rwmd && names(r, PASS_DOC, FLOW_DOC)) || (!rwmd && !same(r, r0))) violated("d VK_NO_DOC_RWMD", f, sw, r); break;
		case SW_NO_DOC_GENERAL: if ((r.wide_gap_mode == 2 && names(r, PASS_DOC, FLOW_DOC)) || (r.wide_gap_mode != 2 && !same(r, r0))) violated("d VK_NO_DOC_GENERAL", f, sw, r); break;
		case SW_NO_SCORE32: if ((r.plan == PLAN_MULTI_BLOCK && !exact && !fill) || (r0.plan != PLAN_MULTI_BLOCK && !same(r, r0))) violated("d VK_NO_SCORE32", f, sw, r); break;
		case SW_NO_APART: {   // (the multi-block kernel's strips and history are sized by the slices it would take: read under PLAN_MULTI_BLOCK only)
			query_route x = r;
			if (r.plan != PLAN_MULTI_BLOCK && r0.plan != PLAN_MULTI_BLOCK) { x.score32_gap_mode = r0.score32_gap_mode; x.wave_tiles = r0.wave_tiles; x.fits32 = r0.fits32; }
			if ((wide_query && r.list == LIST_APART) || (!(wide_query && r0.list == LIST_APART) && !same(x, r0))) violated("d VK_NO_APART", f, sw, r);
			break;
		}
		case SW_LONG_PASS: if ((!wide_query && is_wide_family(r.pass[CLASS_MID])) || (wide_query && !same(r, r0))) violated("d VK_LONG_PASS", f, sw, r); break;
		case SW_LONG_LINEAR: if ((!wide_query && r.wide_gap_mode <= 1 && is_wide_family(r.pass[CLASS_MID])) || ((wide_query || r.wide_gap_mode > 1) && !same(r, r0))) violated("d VK_LONG_LINEAR", f, sw, r); break;
		case SW_KEEP_RAW: { query_route x = r; x.raw = r0.raw; if (!r.raw || !same(x, r0)) violated("d VK_KEEP_RAW", f, sw, r); break; }
		}
	}
}

static void enumerate() {
	struct shape { int max_len, max_short_len, n_long_groups; bool apart, xlong; int pair, short_pair, uniform; };
	const shape shapes[] = {{64, 64, 0, false, false, 9, 9, 0}, {30, 30, 0, false, false, 5, 5, 0}, {512, 64, 3, true, false, 33, 9, 0}, {5000, 64, 3, true, true, 314, 9, 0},
		{600, 64, 0, true, true, 39, 9, 0}, {1, 1, 0, false, false, 1, 1, 1}};
	// 64-d, 300-d (a half K-step), 300-d fp32 blocks, 768-d, and 768-d as fp32 blocks: four query tiles of those exceed the LDS
	const int widths[][2] = {{2, 0}, {10, 1}, {19, 0}, {24, 0}, {48, 0}}, lens[] = {1, 16, 17, 32, 33, 48, 64};
	struct form { int algorithm; bool full, inj; };
	const form forms[] = {{VK_ALG_ALIGN, false, false}, {VK_ALG_RWMD, false, true}, {VK_ALG_RWMD, false, false}, {VK_ALG_RWMD, true, false}, {VK_ALG_WRD, false, false}};
	struct gaps { int mode; float a_t; int tail; };
	const gaps families[] = {{0, 0.0f, 0}, {1, 0.2f, 0}, {1, -0.05f, 0}, {2, 0.0f, 0}, {2, 0.0f, 1}, {2, 0.0f, 126}, {2, 0.0f, 127}};
	long points = 0, refused = 0;
	for (int layout = 0; layout < 2; layout++) for (int prec = 0; prec < 2; prec++) for (const auto &w : widths) for (const shape &sh : shapes)
	for (const int len_t : lens) for (const form &fo : forms) for (const gaps &g : families) for (int flags = 0; flags < 32; flags++) {
		if (fo.algorithm != VK_ALG_ALIGN && &g != &families[0]) continue;   // gap costs: alignments
		route_facts f;
		f.layout = layout ? VK_LAYOUT_STATIC : VK_LAYOUT_CONTEXTUAL; f.prec = prec; f.nk32 = w[0]; f.tail = w[1];
		f.max_len = sh.max_len; f.max_short_len = sh.max_short_len; f.n_long_groups = sh.n_long_groups; f.has_apart = sh.apart; f.has_xlong = sh.xlong;
		f.max_pair_tiles = sh.pair; f.max_short_pair_tiles = sh.short_pair; f.uniform_len = sh.uniform; f.has_pos = true; f.n_sentences = 1000;
		f.algorithm = fo.algorithm; f.wmd_full = fo.full; f.rwmd_injective = fo.inj; f.len_t = len_t;
		if (fo.algorithm == VK_ALG_ALIGN) { f.gaps.gap_mode = g.mode; f.gaps.a_t = g.a_t; f.ws_tail = g.tail < sh.max_len ? g.tail : 0; }
		f.only = flags & 1; f.want_flow = flags & 2; f.submatch = flags & 4; f.tagged = flags & 8; f.bound_pass = flags & 16;
		f.kk = 10; f.raw_score = true; f.locality = VK_LOCAL;
		// what vk_validate_query accepts: whole documents under alignments and the relaxed 1:1 WMD; listed slices with their flows
		if (sh.xlong && !(fo.algorithm == VK_ALG_ALIGN || (fo.algorithm == VK_ALG_RWMD && !fo.full && fo.inj))) continue;
		if (f.only && !f.want_flow) continue;
		if (f.submatch && fo.algorithm != VK_ALG_ALIGN) continue;
		check_point(f, points, refused);
	}
	printf("points %ld refused %ld violations %ld\n", points, refused, violations);
}

int main(int argc, char **argv) {
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "enumerate") { enumerate(); return 0; }
	if (what != "route") return 2;
	// layout prec nk32 tail max_len max_short_len n_long_groups has_apart has_xlong max_pair_tiles max_short_pair_tiles uniform_len bound_pass
	// algorithm wmd_full rwmd_injective len_t gap_mode a_t ws_tail submatch tagged only want_flow locality kk raw_score boost switch (-1: none)
	int v[29];
	float a_t;
	for (;;) {
		for (int i = 0; i < 29; i++) {
			if (i == 18) { if (scanf("%f", &a_t) != 1) return 0; continue; }
			if (scanf("%d", &v[i]) != 1) return 0;
		}
		route_facts f;
		f.layout = v[0]; f.prec = v[1]; f.nk32 = v[2]; f.tail = v[3]; f.max_len = v[4]; f.max_short_len = v[5]; f.n_long_groups = v[6]; f.has_apart = v[7]; f.has_xlong = v[8];
		f.max_pair_tiles = v[9]; f.max_short_pair_tiles = v[10]; f.uniform_len = v[11]; f.bound_pass = v[12];
		f.algorithm = v[13]; f.wmd_full = v[14]; f.rwmd_injective = v[15]; f.len_t = v[16]; f.gaps.gap_mode = v[17]; f.gaps.a_t = a_t; f.ws_tail = v[19];
		f.submatch = v[20]; f.tagged = v[21]; f.only = v[22]; f.want_flow = v[23]; f.locality = v[24]; f.kk = v[25]; f.raw_score = v[26]; f.boost = v[27];
		route_switches s;
		if (bool *b = switch_by_index(s, v[28])) *b = true;
		print_route(route_query(f, s, kFits));
	}
}
