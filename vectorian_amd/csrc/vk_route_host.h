// vk_route_host.h -- which kernels a query of at most VK_MAX_QUERY_LEN tokens runs on: decided once, on the host, from
// plain facts about the corpus and the query, before anything is enqueued.  vk_validate_query reads the refusal, query_run::route()
// and the stages after it (vk_query.cpp) the rest; no other code decides a route.  Host only, no HIP types: tests/test_route_host.py compiles it with g++ and
// enumerates the facts (CPU tier).  Integers a test reads (vk_query_route, vk_corpus.cpp) are the enums below.
#ifndef VK_ROUTE_HOST_H
#define VK_ROUTE_HOST_H

#include "vk_result_host.h"

#include <cstdlib>

namespace vk_host {

// ---- what the decision reads, and nothing else
struct route_facts {
	// the corpus
	int layout = VK_LAYOUT_CONTEXTUAL, prec = 0, nk32 = 0, tail = 0;
	int max_len = 0, max_short_len = 0, n_long_groups = 0;
	bool has_apart = false, has_xlong = false;   // the lists of slices of more than 64 / more than VK_MAX_SENT_LEN tokens are non-empty
	int max_pair_tiles = 0, max_short_pair_tiles = 0, uniform_len = 0;
	bool has_pos = false, has_tags = false;
	bool bound_pass = false;   // a shadow, and VK_BOUND_PASS, the corpus's size and the handle's back-off let this query try it
	int64_t n_sentences = 0;
	// the query and what the caller wants back
	int algorithm = VK_ALG_ALIGN;
	bool wmd_full = false, rwmd_injective = false;
	int len_t = 0;
	gap_form gaps;             // classify_gaps (alignments)
	int ws_tail = 0;           // ws_tail_of (general gaps)
	bool submatch = false, tagged = false, has_q_tags = false, has_q_ids = false, only = false, want_flow = false;
	int locality = VK_LOCAL, kk = 0;
	bool sim_rows = false, raw_score = false, boost = false;
	// a contextual handle under an operator chain (vk_corpus_set_contextual_sim_ops): only vk_score_kernel and
	// vk_score32_kernel have the chain in their epilogue -- no bound pass, no span kernel, and every other scoring pass is refused
	bool chained = false;
};

// From which k on the table w_s is constant up to the corpus's longest slice (a saturated table; 0: no such tail, or no table)
inline int ws_tail_of(const vk_gap &gap_s, int max_len) {
	if (max_len < 2) return 0;
	int kt = max_len;
	while (kt > 1 && gap_cost(gap_s, kt - 1) == gap_cost(gap_s, max_len)) kt--;
	return kt < max_len ? kt : 0;
}

// ---- the VK_* variables of a query, read once per query (the tests flip them between two queries of one process)
struct route_switches {
	bool long_linear = false, long_pass = false, no_doc_mid = false, no_doc_kernel = false, no_doc_flow = false, no_docw = false, no_docg = false;
	bool no_doc_rwmd = false, no_doc_general = false, keep_raw = false, no_apart = false, no_score32 = false;
	bool qlds = false, qreg = false, no_f32_special = false, no_qlds1 = false;   // the LDS carve-up of the fused launch (query_run::score_fused)
	bool wrd_turns = false, debug_candidates = false;                            // the exact transports' rounds (query_run::transport_rounds)
};
inline route_switches read_route_switches() {
	const auto on = [](const char *name) { return getenv(name) != nullptr; };
	route_switches s;
	s.long_linear = on("VK_LONG_LINEAR"); s.long_pass = on("VK_LONG_PASS"); s.no_doc_mid = on("VK_NO_DOC_MID");
	s.no_doc_kernel = on("VK_NO_DOC_KERNEL"); s.no_doc_flow = on("VK_NO_DOC_FLOW"); s.no_docw = on("VK_NO_DOCW"); s.no_docg = on("VK_NO_DOCG");
	s.no_doc_rwmd = on("VK_NO_DOC_RWMD"); s.no_doc_general = on("VK_NO_DOC_GENERAL"); s.keep_raw = on("VK_KEEP_RAW");
	s.no_apart = on("VK_NO_APART"); s.no_score32 = on("VK_NO_SCORE32");
	s.qlds = on("VK_QLDS"); s.qreg = on("VK_QREG"); s.no_f32_special = on("VK_NO_F32_SPECIAL"); s.no_qlds1 = on("VK_NO_QLDS1");
	s.wrd_turns = on("VK_WRD_TURNS"); s.debug_candidates = on("VK_DEBUG_CANDIDATES");
	return s;
}

// ---- the three questions about the LDS of a CU, answered by the kernels' units (vk_score32.hip, vk_flow.hip)
struct route_fits {
	int32_t (*score32_waves)(int32_t nk32, int32_t tail, int32_t wave_tiles, int32_t len_t, int32_t gap_mode);
	int32_t (*wide_ring_rows)(int32_t nq, int32_t gap_mode, int32_t ws_tail);
	size_t (*wide_lds_demand)(int32_t max_len, int32_t nq, int32_t gap_mode, int32_t tagged, int32_t flow);
};

// ---- the answer
// How the scores of all slices come about.  LISTED: no scoring pass (only_slices); SPAN: vk_span_kernel; FUSED: vk_score_kernel;
// BOUNDED: the bound pass and its rounds, then vk_score_kernel on the contenders; MULTI_BLOCK: vk_score32_kernel (and a pass over the
// slices it skips); DOCW / DOCG / WIDE_ALL: the one-wave-per-slice kernel over every row.
enum route_plan { PLAN_LISTED, PLAN_SPAN, PLAN_FUSED, PLAN_BOUNDED, PLAN_MULTI_BLOCK, PLAN_DOCW_ALL, PLAN_DOCG_ALL, PLAN_WIDE_ALL };
// The pass that scores a class of slices (PASS_NONE: the corpus holds none of them, or nothing is scored)
enum route_pass { PASS_NONE, PASS_SPAN, PASS_FUSED, PASS_FUSED_LONG, PASS_SCORE32, PASS_LONG_RWMD_FILL, PASS_LONG_BOUND, PASS_DOC, PASS_DOCW, PASS_DOCG, PASS_WIDE };
// The work list of the doc / docw / docg / wide pass: every non-empty row, the slices of more than 64 tokens, those beyond VK_MAX_SENT_LEN
enum route_list { LIST_NONE, LIST_ALL, LIST_APART, LIST_XLONG };
// The traceback kernel asked for first (launch_flow falls back from DOC / DOCW / DOCG to WIDE where rows or scratch did not come about)
enum route_flow { FLOW_NARROW, FLOW_WIDE, FLOW_DOC, FLOW_DOCW, FLOW_DOCG };
enum slice_class { CLASS_SHORT, CLASS_MID, CLASS_XLONG };   // at most 64 tokens, 65 .. VK_MAX_SENT_LEN, beyond

struct query_route {
	int status = VK_OK;          // the refusal, if any: nothing is enqueued then
	const char *message = "";
	bool fits32 = true;          // a query of 17 .. 64 tokens: the multi-block kernel's query tiles and one wave's strip fit the LDS
	int gap_mode = 0;            // vk_score_kernel (and what the narrow traceback kernel derives its own from)
	int wide_gap_mode = 0;       // the one-wave-per-slice family, scoring and traceback
	int score32_gap_mode = 0, wave_tiles = 0;   // vk_score32_kernel
	route_plan plan = PLAN_LISTED;
	route_pass pass[3] = {PASS_NONE, PASS_NONE, PASS_NONE};   // by slice_class
	route_pass wide_pass = PASS_NONE;   // the doc / docw / docg / wide pass that runs, over `list` (LIST_NONE: vk_wide_kernel walks the slice table itself)
	route_list list = LIST_NONE;
	int ring_rows = 0;           // vk_wide_ring_rows of this query; the pass over a list takes the ring form where it is > 0
	bool wide_lds_score = false, wide_lds_flow = false;   // vk_wide_kernel keeps a slice's state in LDS (else in global memory)
	route_flow flow = FLOW_NARROW;
	int ostride = 16;            // row stride of the winners' mapping / edge_sim device arrays
	bool raw = true;             // the scoring pass writes the aligner scores of all slices
	bool span_skip_raw = false;
};

// Exact transport (WRD, the non-relaxed WMD): a bound pass over all slices, then the exact solver on the candidates.
inline bool exact_transport(int algorithm, bool wmd_full) { return algorithm == VK_ALG_WRD || (algorithm == VK_ALG_RWMD && wmd_full); }

// What lets a query try the bound pass apart from the shadow, VK_BOUND_PASS and the back-off: an alignment of at most 16
// tokens, nothing that changes a cell or the reference score per slice, every slice scored, no slice of more than 64 tokens
inline bool bound_pass_takes(const route_facts &f) {
	return f.algorithm == VK_ALG_ALIGN && f.len_t <= VK_FAST_QUERY_LEN && !f.submatch && !f.tagged && !f.only && f.n_long_groups == 0 && f.max_len <= VK_FAST_SENT_LEN;
}

// The refusals of a contextual handle under an operator chain: the chain and the case, by name
constexpr const char *kChainedLongSlices = "an operator chain on a contextual handle (vk_corpus_set_contextual_sim_ops) over a corpus that holds a slice of more than 64 tokens: "
	"the doc / docw / docg / wide / longq scoring kernels know the clipped cosine only (vk_score_kernel and vk_score32_kernel run the chain)";
constexpr const char *kChainedLongQuery = "an operator chain on a contextual handle (vk_corpus_set_contextual_sim_ops) under a query of more than 64 tokens: "
	"the doc / docw / docg / wide / longq scoring kernels know the clipped cosine only (vk_score_kernel and vk_score32_kernel run the chain)";
constexpr const char *kChainedWideQuery = "an operator chain on a contextual handle (vk_corpus_set_contextual_sim_ops) under a query of 17 .. 64 tokens that the multi-block kernel "
	"does not take (rows too wide for its LDS, affine gaps with a_t < 0, VK_NO_SCORE32): the doc / docw / docg / wide / longq scoring kernels know the clipped cosine only";

inline query_route route_query(const route_facts &f, const route_switches &sw, const route_fits &fits) {
	query_route r;
	if (f.chained && f.len_t > VK_MAX_QUERY_LEN) {   // (vk_longq_kernel: asked by vk_validate_query, which routes no other query this long)
		r.status = VK_ERR_UNSUPPORTED;
		r.message = kChainedLongQuery;
		return r;
	}
	const bool align = f.algorithm == VK_ALG_ALIGN, rwmd = f.algorithm == VK_ALG_RWMD;
	const bool exact = exact_transport(f.algorithm, f.wmd_full);
	const bool relaxed_11 = rwmd && !f.wmd_full && f.rwmd_injective;   // a stream of row / column minima
	const bool fill = rwmd && !f.wmd_full && !f.rwmd_injective;        // the 1:n form: a slice's bag of words in LDS
	const bool is_static = f.layout == VK_LAYOUT_STATIC;
	const bool xlong = f.max_len > VK_MAX_SENT_LEN, has_mid = f.n_long_groups > 0;
	const bool wide_query = f.len_t > VK_FAST_QUERY_LEN;               // 17 .. 64 tokens: no fused kernel
	const int nq = (f.len_t + 15) / 16;
	const bool present[3] = {true, has_mid, xlong};   // (the slice table always has rows of at most 64 tokens: its padding)

	// ---- gap modes.  0 linear, 1 affine, 2 general (tables), 4 relaxed WMD, 5 exact transport's bound, 7 the 1:n relaxed WMD; 3 / 6:
	// the register-history forms of general gaps over slices of at most 32 / 64 tokens (vk_score_kernel, vk_score32_kernel)
	const int base = f.algorithm == VK_ALG_WRD ? 5 : rwmd ? (fill ? 7 : 4) : f.gaps.gap_mode;
	const bool linear_affine = base == 0 || base == 1;
	const bool tail_ok = f.ws_tail >= 1 && f.ws_tail <= 126;           // a table the doc / docg sweeps take: saturated within 126 tokens
	r.wide_gap_mode = base;
	r.gap_mode = (base == 2 && !wide_query) ? (f.max_short_len <= 32 ? 3 : 6) : base;

	// ---- at most 16 query tokens: which slices leave the fused kernels
	// general gaps over slices of 65 .. 512 tokens, and since round 4 linear / affine gaps too (VK_LONG_LINEAR=1 / VK_LONG_PASS=1: the
	// fused kernel's long pass): the one-wave-per-slice pass over the slices apart
	const bool mid_via_list = align && !wide_query && has_mid && (base == 2 || !sw.long_linear) && !sw.long_pass;
	const bool rwmd_mid_via_list = relaxed_11 && !wide_query && !xlong && has_mid && !sw.long_pass;
	const bool list_pass = !wide_query && (xlong || mid_via_list || rwmd_mid_via_list);
	const bool wide_family = wide_query || xlong || mid_via_list;      // the winners' tracebacks on the one-wave-per-slice family
	const bool doc_score = (xlong || rwmd_mid_via_list || (mid_via_list && !sw.no_doc_mid)) && !wide_query && (align || rwmd) && !sw.no_doc_kernel;
	// winners of 65 .. 512 tokens that the fused kernel's long pass scored under linear / affine gaps: retraced by vk_doc_kernel
	const bool doc_flow_only = align && !wide_family && f.max_len > VK_FAST_SENT_LEN && linear_affine && !sw.no_doc_flow;
	const bool doc = (doc_score || doc_flow_only) && (rwmd ? base == 4 && !sw.no_doc_rwmd : (linear_affine || (base == 2 && tail_ok && !sw.no_doc_general)));

	// ---- 17 .. 64 query tokens: the multi-block kernel over the slices of at most 64 tokens where it can, the others apart
	const bool docw = wide_query && !sw.no_docw && ((align && linear_affine) || (relaxed_11 && f.max_len > VK_FAST_SENT_LEN));
	const bool docg = align && wide_query && f.len_t <= 32 && f.max_len > VK_FAST_SENT_LEN && base == 2 && tail_ok && !sw.no_docg;
	const bool apart = wide_query && (align || relaxed_11) && f.has_apart && !sw.no_apart;   // a pass of their own over the slices apart
	const bool long_transport = wide_query && (exact || fill) && has_mid;                    // ... vk_long_bound / vk_long_rwmd_fill
	const bool skips_long = long_transport || apart;
	r.score32_gap_mode = exact ? 5 : base == 2 ? ((apart ? f.max_short_len : f.max_len) <= 32 ? 3 : 6) : base;
	r.wave_tiles = skips_long ? (f.len_t <= 32 ? f.max_short_pair_tiles : (f.max_short_len + 15) / 16 + 1)
		: (f.len_t <= 32 ? f.max_pair_tiles : (f.max_len + 15) / 16 + 1);
	const bool fits32 = r.fits32 = !wide_query || fits.score32_waves(is_static ? 0 : f.nk32, f.tail, r.wave_tiles, f.len_t, r.score32_gap_mode) >= 1;
	// (affine gaps: the prefix-scan form of F needs open_t >= extend_t)
	const bool multi_block = wide_query && fits32 && (skips_long || (!has_mid && f.max_len <= VK_FAST_SENT_LEN)) && (apart || !xlong) &&
		(!align || base != 1 || f.gaps.a_t >= 0.0f) && (exact || fill || !sw.no_score32);
	// a contextual handle under an operator chain: every scoring pass is vk_score_kernel or vk_score32_kernel, or the query is refused
	if (f.chained && (has_mid || xlong || (wide_query && !multi_block))) {
		r.status = VK_ERR_UNSUPPORTED;
		r.message = (has_mid || xlong) ? kChainedLongSlices : kChainedWideQuery;
		return r;
	}
	// exact transport and the 1:n RWMD have no other kernel for such queries: refused before anything is enqueued.  (Over a finalized
	// corpus whose long slices vk_validate_query has admitted, the kernel is ruled out by its LDS demand alone: fits32 is false.)
	if (wide_query && (exact || fill) && !multi_block) {
		r.status = VK_ERR_UNSUPPORTED;
		r.message = !fits32 ? "exact transport / 1:n RWMD with a query of more than 16 tokens: the query tiles of rows this wide and one wave's similarity strip exceed the LDS of a workgroup (160 KiB)"
			: "exact transport / 1:n RWMD with a query of more than 16 tokens: the multi-block kernel does not take this corpus";
		return r;
	}

	// ---- the scoring plan and the pass of each class of slices
	// (under a chain the score of a one-token slice is no clipped cosine: the fused kernel; nor does the shadow bound a chain's output)
	const bool span = !f.chained && !wide_query && align && !is_static && f.len_t == 1 && f.uniform_len == 1 && f.locality == VK_LOCAL && !f.tagged;
	const route_pass wide_pass = docw ? PASS_DOCW : docg ? PASS_DOCG : PASS_WIDE, doc_pass = doc ? PASS_DOC : PASS_WIDE;
	if (f.only) r.plan = PLAN_LISTED;
	else if (wide_query) {
		r.plan = multi_block ? PLAN_MULTI_BLOCK : docw ? PLAN_DOCW_ALL : docg ? PLAN_DOCG_ALL : PLAN_WIDE_ALL;
		if (multi_block) {
			r.pass[CLASS_SHORT] = PASS_SCORE32;
			r.pass[CLASS_MID] = fill ? PASS_LONG_RWMD_FILL : exact ? PASS_LONG_BOUND : wide_pass;
			r.pass[CLASS_XLONG] = wide_pass;
			if (apart) { r.list = LIST_APART; r.wide_pass = wide_pass; }
		} else {
			r.pass[CLASS_SHORT] = r.pass[CLASS_MID] = r.pass[CLASS_XLONG] = r.wide_pass = wide_pass;
			// (vk_wide_kernel walks the slice table itself unless whole documents make it sort its work)
			r.list = (wide_pass != PASS_WIDE || xlong) ? LIST_ALL : LIST_NONE;
		}
	} else if (span) {
		r.plan = PLAN_SPAN;
		r.pass[CLASS_SHORT] = PASS_SPAN;
	} else {
		r.plan = (!f.chained && f.bound_pass && bound_pass_takes(f) && f.kk <= VK_MAX_MATCHES) ? PLAN_BOUNDED : PLAN_FUSED;
		r.pass[CLASS_SHORT] = PASS_FUSED;
		r.pass[CLASS_MID] = (mid_via_list || rwmd_mid_via_list) ? doc_pass : PASS_FUSED_LONG;
		r.pass[CLASS_XLONG] = doc_pass;
		if (list_pass) { r.list = (mid_via_list || rwmd_mid_via_list) ? LIST_APART : LIST_XLONG; r.wide_pass = doc_pass; }
	}
	for (int k = 0; k < 3; k++)
		if (!present[k]) r.pass[k] = PASS_NONE;

	// ---- the winners' tracebacks
	r.flow = !(wide_family || doc_flow_only) ? FLOW_NARROW : (align && docw) ? FLOW_DOCW : docg ? FLOW_DOCG : doc ? FLOW_DOC : FLOW_WIDE;
	r.ostride = r.flow == FLOW_NARROW ? 16 : 64;

	// ---- vk_wide_kernel's state: the ring form over a list where the table saturates, else LDS where a slice's state fits
	if (base <= 4) {   // (the modes vk_wide_kernel has)
		r.ring_rows = fits.wide_ring_rows(nq, base, f.ws_tail);
		const bool ring_pass = (r.list == LIST_APART || r.list == LIST_XLONG) && r.ring_rows > 0;
		r.wide_lds_score = !xlong && !ring_pass && fits.wide_lds_demand(f.max_len, nq, base, f.tagged, 0) <= 160 * 1024;
		r.wide_lds_flow = !xlong && r.flow == FLOW_WIDE && fits.wide_lds_demand(f.max_len, nq, base, f.tagged, 1) <= 160 * 1024;
	}

	// ---- the aligner scores of all slices: written only if something reads them -- the submatch bound and, without traceback, the
	// winners; with traceback the flow kernel restates those of the winners, exact transport's solver states them
	r.raw = !(((align && f.want_flow) || exact) && !f.submatch && !sw.keep_raw);
	// (the span kernel: without a booster the score IS the aligner score)
	r.span_skip_raw = span && !f.submatch && ((f.want_flow && align) || !f.boost || !f.raw_score);
	return r;
}

} // namespace vk_host

#endif
