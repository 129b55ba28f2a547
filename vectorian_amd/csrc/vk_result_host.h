// vk_result_host.h -- from "the selected keys and their tracebacks" to a result set: the host-side rules every query path shares
// (vk_query.cpp, vk_batch.cpp, vk_longq_host.cpp).  One definition each of the selection keys' encoding, the order of a result set,
// the score of a winner restated from its traceback, the writer of a result set (the one place where the fields of a vk_topk_out are
// assigned), and the forms of the gap costs the kernels are launched with.
// Host only, no HIP types: tests/test_result_host.py compiles it with g++ and holds each rule against its statement in numpy (CPU tier).
#ifndef VK_RESULT_HOST_H
#define VK_RESULT_HOST_H

#include "../../include/vectorian_hip.h"
#include "vk_bound_host.h"   // the bound pass's host rules, for the programs that include this header to reach them

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

namespace vk_host {

// ---- selection keys: (orderable(score) << 32) | row of the slice table; 0 = empty slot.  Keys compare as unsigned 64-bit numbers in
// the order of a result set (score, then row).  The encoder is float_orderable, vk_select.hip:17 (and vk_doc.hip:36): a set sign bit
// flips every bit, a clear one sets the sign bit.  key_score inverts it bit for bit.
inline float key_score(uint64_t key) {
	const uint32_t ob = (uint32_t)(key >> 32);
	const uint32_t bits = (ob & 0x80000000u) ? (ob & 0x7fffffffu) : ~ob;
	float s;
	memcpy(&s, &bits, 4);
	return s;
}
inline uint32_t key_row(uint64_t key) { return (uint32_t)(key & 0xffffffffu); }
// the key that names a listed row to the traceback / rows / solver kernels (they read the row only; any non-zero score field)
inline uint64_t key_of_row(int64_t row) { return (1ull << 32) | (uint64_t)(uint32_t)row; }
// the selected keys of `cap` slots: up to the first empty one
inline int count_keys(const uint64_t *keys, int cap) {
	int n = 0;
	while (n < cap && keys[n] != 0) n++;
	return n;
}

// ---- the total order of a result set: score descending, ties by slice index descending (match/match_impl.h:8-42); admission is
// score > min_score (metric/alignment.h:284), so a score equal to min_score is out.  Scores must not be NaN (a strict weak order):
// the merges of records from other ranks map NaN to -inf before they come here.
inline bool ranks_before(float score_a, int64_t slice_a, float score_b, int64_t slice_b) {
	if (score_a != score_b) return score_a > score_b;
	return slice_a > slice_b;
}
// `order` holds positions i with score(i) and slice(i): drops those not above min_score, sorts the rest into the order above
template <typename Score, typename Slice> void rank_above(std::vector<int> &order, float min_score, Score score, Slice slice) {
	order.erase(std::remove_if(order.begin(), order.end(), [&](int i) { return !(score(i) > min_score); }), order.end());
	std::sort(order.begin(), order.end(), [&](int a, int b) { return ranks_before(score(a), (int64_t)slice(a), score(b), (int64_t)slice(b)); });
}

// ---- the score of a winner from its canonical aligner score `raw` and its traceback (match/match.h:295-307; reference_score,
// metric/alignment.h:84-106), operation by operation in float as the oracle's vko_score: the matched weight of THIS traceback (query
// token j counts tag_weights[j], or 1 without tag weights; total is their sum over the query), pow((total - matched) / total, w),
// ref = matched + that * (total - matched), (raw / ref) * boost.  map_row: the winner's mapping, -1 = unmatched.
// (A copy that added `matched += cond ? 1.0f : 0.0f` gave the same floats: x + 0.0f == x for the sums of non-negative terms here.)
inline float reference_score(float raw, const int16_t *map_row, int len_t, const float *tag_weights, float total, float submatch_weight, float boost) {
	float matched = 0.0f;
	for (int j = 0; j < len_t; j++)
		if (map_row[j] >= 0) matched += tag_weights ? tag_weights[j] : 1.0f;
	const float uw = powf((total - matched) / total, submatch_weight);
	const float ref = matched + uw * (total - matched);
	return (raw / ref) * boost;
}

// a winner without a stated flow (transports: SparseFlow / DenseFlow are stated from the similarity rows, not here)
inline void no_flow(int16_t *map_row, float *sim_row, int len_t) {
	for (int j = 0; j < len_t; j++) {
		map_row[j] = -1;
		sim_row[j] = 0.0f;
	}
}

// ---- where the host restates the winners' scores: this many runners-up are selected with them, above a floor lowered by the
// rounding slack of the scoring pass; the k best restated scores above min_score itself are kept
constexpr int kCanonMargin = 8;
inline float restated_floor(float min_score) { return min_score - 1e-5f * std::max(1.0f, std::fabs(min_score)); }

// ---- the writer of a result set.  Every query path ends here: score_selected, then write_result_set; the candidate rounds (exact
// transports, submatch weight) keep_best, then write_best.  Callers: the four exits of a query (query_run::listed_transports, transport_rounds, submatch_rounds, selected_result), vk_merge_topk and vk_merge_records
// (vk_query.cpp); vk_longq_query (vk_longq_host.cpp); batch_winner_rows, query_batch_shared_pass, query_batch_span and the GEMM
// path of query_batch_body (vk_batch.cpp).
// What came back from the device for one query: `cap` key slots, best first (up to the first empty one); the aligner scores where
// the path has them; where the winners were retraced, the rows of their mappings and edge similarities, `stride` elements apart.
// slice_of_row: the slice of a row of the slice table; null where rows are slices.
struct selected {
	const uint64_t *keys = nullptr;
	int cap = 0;
	const float *raw = nullptr;
	const int16_t *map = nullptr;
	const float *sim = nullptr;
	int stride = 0;
	const int32_t *slice_of_row = nullptr;
	int64_t row(int i) const { return (int64_t)key_row(keys[i]); }
	int64_t slice(int i) const { return slice_of_row ? (int64_t)slice_of_row[row(i)] : row(i); }
};
// a result set in the making: val / raw by position among the selected keys, order[i] the position of the i-th result (kept by the
// caller from query to query: no allocation per query on the batched paths)
struct result_set {
	std::vector<int> order;
	std::vector<float> val, raw;
	int n_out = 0;
};
// how score_selected restates position i: a callable returning (raw, score).  as_selected: not at all, the keys' scores in the keys'
// order (raw: the traceback's where there is one, else the score, for the caller to replace where the path states another).
// by_traceback: reference_score of the position's own traceback; boost by slice, null = none.
struct as_selected {};
struct by_traceback {
	const selected &v;
	int len_t;
	const float *tag_weights;
	float total, submatch_weight;
	const float *boost;
	std::pair<float, float> operator()(int i) const {
		return {v.raw[i], reference_score(v.raw[i], v.map + (size_t)i * v.stride, len_t, tag_weights, total, submatch_weight, boost ? boost[v.slice(i)] : 1.0f)};
	}
};
// The scores of the selected slices and how many of them are results: restated scores are ranked (rank_above: those not above
// min_score leave; ties by row, which orders as the slice does) unless the slices are `listed`, which keep the caller's order and
// ignore min_score; at most `limit` (k, or the number listed) are results.
template <typename Restate = as_selected>
int score_selected(const selected &v, result_set &rs, float min_score, int limit, bool listed, Restate restate = {}) {
	const int n_sel = count_keys(v.keys, v.cap);
	rs.order.resize((size_t)n_sel); rs.val.resize((size_t)n_sel); rs.raw.resize((size_t)n_sel);
	for (int i = 0; i < n_sel; i++) {
		rs.order[(size_t)i] = i;
		rs.val[(size_t)i] = key_score(v.keys[i]);
		rs.raw[(size_t)i] = v.raw ? v.raw[i] : rs.val[(size_t)i];
	}
	if constexpr (!std::is_same<Restate, as_selected>::value) {
		for (int i = 0; i < n_sel; i++) std::tie(rs.raw[(size_t)i], rs.val[(size_t)i]) = restate(i);
		if (!listed) rank_above(rs.order, min_score, [&](int i) { return rs.val[(size_t)i]; }, [&](int i) { return v.row(i); });
	}
	return rs.n_out = std::min((int)rs.order.size(), limit);
}
// Winner i of a result set: score, slice, the aligner score if the caller has an array for it.  Flows only where the caller asked
// for them (`flows`) and has both arrays: the len_t entries of the mapping and the edge similarities from the winner's rows, or,
// where the path states none (no rows), no_flow.  Nothing else is touched.
inline void write_winner(vk_topk_out *out, int i, int len_t, float score, int64_t slice, float raw, const int16_t *map_row, const float *sim_row, bool flows) {
	out->score[i] = score;
	out->sentence[i] = slice;
	if (out->raw_score) out->raw_score[i] = raw;
	if (!(flows && out->mapping && out->edge_sim)) return;
	if (!map_row) return no_flow(out->mapping + (size_t)i * len_t, out->edge_sim + (size_t)i * len_t, len_t);
	memcpy(out->mapping + (size_t)i * len_t, map_row, (size_t)len_t * sizeof(int16_t));
	memcpy(out->edge_sim + (size_t)i * len_t, sim_row, (size_t)len_t * sizeof(float));
}
// the merges of result sets (vk_merge_topk, vk_merge_records) carry along whichever rows source and destination both have
inline void merge_rows(vk_topk_out *out, int i, int len_t, const int16_t *map_row, const float *sim_row) {
	if (map_row && out->mapping) memcpy(out->mapping + (size_t)i * len_t, map_row, (size_t)len_t * sizeof(int16_t));
	if (sim_row && out->edge_sim) memcpy(out->edge_sim + (size_t)i * len_t, sim_row, (size_t)len_t * sizeof(float));
}
inline void write_result_set(vk_topk_out *out, const selected &v, const result_set &rs, int len_t, bool flows) {
	for (int i = 0; i < rs.n_out; i++) {
		const int src = rs.order[(size_t)i];
		write_winner(out, i, len_t, rs.val[(size_t)src], v.slice(src), rs.raw[(size_t)src], v.map ? v.map + (size_t)src * v.stride : nullptr,
			v.sim ? v.sim + (size_t)src * v.stride : nullptr, flows);
	}
	out->n_out = rs.n_out;
}
// The candidate rounds: a round's candidates above min_score join the best so far, which stay in the order of a result set, k at most
// (a candidate that leaves takes its traceback with it).  map / sim: the traceback of a candidate scored from it; empty for the
// transports.  When to stop is the caller's rule.
struct candidate { float val, raw; int64_t row; std::vector<int16_t> map; std::vector<float> sim; };
inline void keep_best(std::vector<candidate> &best, std::vector<candidate> &round, float min_score, int k) {
	for (candidate &cd : round)
		if (cd.val > min_score) best.push_back(std::move(cd));
	round.clear();
	const auto better = [](const candidate &a, const candidate &b) { return ranks_before(a.val, a.row, b.val, b.row); };
	if ((int)best.size() > k) {
		std::partial_sort(best.begin(), best.begin() + k, best.end(), better);
		best.resize((size_t)k);
	} else std::sort(best.begin(), best.end(), better);
}
inline void write_best(vk_topk_out *out, const std::vector<candidate> &best, const int32_t *slice_of_row, int len_t, bool flows) {
	for (size_t i = 0; i < best.size(); i++) {
		const candidate &b = best[i];
		write_winner(out, (int)i, len_t, b.val, slice_of_row ? (int64_t)slice_of_row[b.row] : b.row, b.raw, b.map.empty() ? nullptr : b.map.data(), b.sim.data(), flows);
	}
	out->n_out = (int)best.size();
}
// the aligner score behind a score of the batched relaxed-WMD pass: the boost taken out, the mean over the query's tokens undone
inline float unboosted_sum(float score, const float *boost, int64_t slice, int len_t) { return (boost ? score / boost[slice] : score) * (float)len_t; }

// ---- gap costs
inline float gap_cost(const vk_gap &g, int k) {
	if (k <= 0) return 0.0f;
	switch (g.kind) {
	case VK_GAP_LINEAR: return g.u * (float)k;
	case VK_GAP_AFFINE: return g.u + g.v * (float)k;
	default: return (g.table && k < g.n_table) ? g.table[k] : INFINITY;
	}
}

// The form of the recurrence a pair of gap costs is aligned with: 0 both linear (gs, gt per token); 1 linear / affine (a_* to open,
// g* per token, open_* their sum; a linear side opens at 0); 2 a table on either side (every field 0: the kernels read the tables).
// The callers copy the fields into their parameter struct.
struct gap_form { int gap_mode = 2; float gs = 0.0f, gt = 0.0f, a_s = 0.0f, a_t = 0.0f, open_s = 0.0f, open_t = 0.0f; };
inline gap_form classify_gaps(const vk_gap &s, const vk_gap &t) {
	gap_form f;
	if (s.kind == VK_GAP_LINEAR && t.kind == VK_GAP_LINEAR) {
		f.gap_mode = 0;
		f.gs = s.u; f.gt = t.u;
	} else if ((s.kind == VK_GAP_LINEAR || s.kind == VK_GAP_AFFINE) && (t.kind == VK_GAP_LINEAR || t.kind == VK_GAP_AFFINE)) {
		f.gap_mode = 1;
		f.a_s = s.kind == VK_GAP_AFFINE ? s.u : 0.0f;
		f.gs = s.kind == VK_GAP_AFFINE ? s.v : s.u;
		f.a_t = t.kind == VK_GAP_AFFINE ? t.u : 0.0f;
		f.gt = t.kind == VK_GAP_AFFINE ? t.v : t.u;
		f.open_s = f.a_s + f.gs;
		f.open_t = f.a_t + f.gt;
	}
	return f;
}

// wt[0..79]: w_t as given, up to the query's length (0 beyond it, and throughout when the query is no alignment); wt[80..159]: its
// subadditive closure w*[k] = min(w[k], min over a of w*[a] + w*[k - a]).  The register-history kernels take their in-row candidates
// from the row's values before in-row gaps, which is the sequential recurrence with w_t replaced by w* (dp_general_reg in
// vk_common.hip.h).  (Round 1 sent every table that was not strictly subadditive -- a linear cost handed over as a table, a convex
// one -- to the LDS-history kernel with its serial in-row chain: 12.7 ms per 1 M x 32 tokens against 2.9 ms.)
inline void wt_with_closure(float *wt, const vk_gap &gap_t, int len_t, bool is_align) {
	for (int i = 0; i < 80; i++) wt[i] = (is_align && i <= len_t) ? gap_cost(gap_t, i) : 0.0f;
	for (int k = 0; k < 80; k++) wt[80 + k] = wt[k];
	for (int k = 2; k <= len_t && k < 80; k++)
		for (int a = 1; a < k; a++) wt[80 + k] = std::min(wt[80 + k], wt[80 + a] + wt[80 + k - a]);
}

} // namespace vk_host

#endif
