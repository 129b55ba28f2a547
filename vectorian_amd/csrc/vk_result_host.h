// vk_result_host.h -- from "the selected keys and their tracebacks" to a result set: the host-side rules every query path shares
// (vk_query.cpp, vk_batch.cpp, vk_longq_host.cpp).  One definition each of the selection keys' encoding, the order of a result set,
// the score of a winner restated from its traceback, and the forms of the gap costs the kernels are launched with.
// Host only, no HIP types: tests/test_result_host.py compiles it with g++ and holds each rule against its statement in numpy (CPU tier).
#ifndef VK_RESULT_HOST_H
#define VK_RESULT_HOST_H

#include "../../include/vectorian_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// the integer helpers of the 6-bit shadow are compiled for the device too (vk_shadow6_kernel calls them)
#ifdef __HIPCC__
#define VK_HOST_DEVICE __host__ __device__
#else
#define VK_HOST_DEVICE
#endif

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

// ---- the 8-bit bound pass: the quantizer of one row x (the bf16 values as stored, handed over as floats).
// s = max|x| / 127, xq[k] = round(x[k] / s) (to nearest even, within -127 .. 127); e >= |x - s xq|, n >= |s xq|, a >= |x| (Euclidean
// norms, summed in double in k order, then rounded UP to float: quant_up).  A row of zeros gives zeros throughout.  The shadow's builder
// (vk_shadow_kernel, vk_pack.hip) is this function statement for statement.
struct quant_meta { float s = 0.0f, e = 0.0f, n = 0.0f, a = 0.0f; };
inline float quant_up(double x) {
	if (!(x > 0.0)) return 0.0f;
	return std::nextafterf((float)(x * (1.0 + 1e-6)), INFINITY);
}
inline quant_meta quantize_row_i8(const float *x, int d, int8_t *xq) {
	float m = 0.0f;
	for (int k = 0; k < d; k++) m = std::max(m, std::fabs(x[k]));
	quant_meta r;
	r.s = m / 127.0f;
	double e2 = 0.0, n2 = 0.0, a2 = 0.0;
	for (int k = 0; k < d; k++) {
		int v = 0;
		if (r.s > 0.0f) v = (int)std::min(127.0f, std::max(-127.0f, std::nearbyintf(x[k] / r.s)));
		xq[k] = (int8_t)v;
		const double xs = (double)r.s * (double)v, dd = (double)x[k] - xs;
		e2 += dd * dd; n2 += xs * xs; a2 += (double)x[k] * (double)x[k];
	}
	r.e = quant_up(std::sqrt(e2)); r.n = quant_up(std::sqrt(n2)); r.a = quant_up(std::sqrt(a2));
	return r;
}
// The constants of query column j in a cell of the bound pass, ub = clip01((s_x cs) I + e_x ca + cb) (I the exact integer product):
// cs = s_q, ca = a_q, cb = e_q N + gamma, with N >= every |s_x xq| of the corpus and X >= every |x| of it.  gamma:
// twice d_pad 2^-24 a_q X for the fp32 accumulation of the exact kernel's MFMA cosine and the five roundings of the bound's own
// evaluation, plus 2e-6 absolute for the same roundings near zero.  Rounded up.
inline void bound_cell_constants(const quant_meta &q, float N, float X, int d_pad, float *cs, float *ca, float *cb) {
	const double gamma = 2.0 * (double)d_pad * std::ldexp(1.0, -24) * (double)q.a * (double)X + 2e-6;
	*cs = q.s; *ca = q.a;
	*cb = quant_up((double)q.e * (double)N + gamma);
}

// ---- the 6-bit bound pass: E2M3 codes, bit 5 the sign, bits 4 .. 0 the magnitude: 0 .. 1.875 in steps of 0.125 (codes
// 0 .. 15), 2 .. 3.75 in steps of 0.25 (16 .. 23), 4 .. 7.5 in steps of 0.5 (24 .. 31) -- the operand format of
// v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 2.  No code is an infinity or a NaN.
VK_HOST_DEVICE inline int e2m3_eighths(int code) {   // 8 x the value: an integer, |.| <= 60
	const int mag = code & 31, e = mag >> 3, f = mag & 7;
	const int n = e == 0 ? f : (8 + f) << (e - 1);
	return (code & 32) ? -n : n;
}
// the magnitude bits of the grid value n8 / 8 (n8 = 0 .. 15, an even number up to 30, a multiple of 4 up to 60)
VK_HOST_DEVICE inline int e2m3_mag_of_eighths(int n8) {
	return n8 < 16 ? n8 : n8 < 32 ? 16 + ((n8 - 16) >> 1) : 24 + ((n8 - 32) >> 2);
}
// The quantizer of one row (the bf16 values as stored): s = max|x| / 7.5, xq[k] the code of the grid value nearest to x[k] / s -- a
// tie at the midpoint of a step goes to the even multiple of that step (nearbyintf), magnitudes clip to 7.5; e, n, a as quantize_row_i8
// gives them, with s x^ the value of the code.  A row of zeros gives zeros throughout.  The builder of the 6-bit shadow
// (vk_shadow6_kernel, vk_pack.hip) is this function statement for statement in its floating-point part and calls the same integer
// helpers (e2m3_mag_of_eighths, fp6_pack32).
inline quant_meta quantize_row_e2m3(const float *x, int d, uint8_t *xq) {
	float m = 0.0f;
	for (int k = 0; k < d; k++) m = std::max(m, std::fabs(x[k]));
	quant_meta r;
	r.s = m / 7.5f;
	double e2 = 0.0, n2 = 0.0, a2 = 0.0;
	for (int k = 0; k < d; k++) {
		int code = 0;
		float v = 0.0f;
		if (r.s > 0.0f) {
			const float t = std::min(7.5f, std::fabs(x[k] / r.s));
			const float step = t < 2.0f ? 0.125f : t < 4.0f ? 0.25f : 0.5f;
			const float a = std::min(7.5f, std::nearbyintf(t / step) * step);
			const int mag = e2m3_mag_of_eighths((int)(a * 8.0f));
			code = mag | ((x[k] < 0.0f && mag != 0) ? 32 : 0);
			v = x[k] < 0.0f ? -a : a;
		}
		xq[k] = (uint8_t)code;
		const double xs = (double)r.s * (double)v, dd = (double)x[k] - xs;
		e2 += dd * dd; n2 += xs * xs; a2 += (double)x[k] * (double)x[k];
	}
	r.e = quant_up(std::sqrt(e2)); r.n = quant_up(std::sqrt(n2)); r.a = quant_up(std::sqrt(a2));
	return r;
}
// A lane's operand of one K-step: 32 codes, code j at bits 6 j .. 6 j + 5 of 192 (six words).  Stored as the tile keeps a K-step of
// `quarters` 16-lane quarters: the first four words of lane l at 16 l, the last two behind all of those at 256 quarters + 8 l.
VK_HOST_DEVICE inline void fp6_pack32(const uint8_t *codes, uint32_t *w) {
	for (int i = 0; i < 6; i++) w[i] = 0u;
	for (int j = 0; j < 32; j++) {
		const int bit = 6 * j;
		w[bit >> 5] |= (uint32_t)(codes[j] & 63) << (bit & 31);
		if ((bit & 31) > 26) w[(bit >> 5) + 1] |= (uint32_t)(codes[j] & 63) >> (32 - (bit & 31));
	}
}
inline void fp6_store_lane(uint8_t *step, int quarters, int lane, const uint32_t *w) {
	memcpy(step + (size_t)lane * 16, w, 16);
	memcpy(step + (size_t)quarters * 256 + (size_t)lane * 8, w + 4, 8);
}
// one row's codes (d of them, zeros beyond) into row i of a tile whose last K-step keeps `live6` quarters (4: a query tile)
inline void fp6_put_row(uint8_t *tile, int live6, int i, const uint8_t *codes, int d) {
	uint8_t c32[32];
	uint32_t w[6];
	for (int t = 0; t < 3; t++)
		for (int g = 0; g < (t == 2 ? live6 : 4); g++) {
			for (int j = 0; j < 32; j++) { const int k = 128 * t + 32 * g + j; c32[j] = k < d ? codes[k] : 0; }
			fp6_pack32(c32, w);
			fp6_store_lane(tile + (size_t)t * 1536, t == 2 ? live6 : 4, 16 * g + i, w);
		}
}

// When a handle stops trying the bound pass: after 5 fallbacks to the full pass among its last 8 bound passes the next 64
// queries go without one.  A stream of queries whose bounds never separate thus pays at most 8 wasted bound passes per 72 queries.
// take(): does this query try the bound pass; record(): how the bound pass of a query that took it ended.
struct bound_backoff {
	uint32_t recent = 0;   // fallbacks among the last 8 bound passes, one bit each
	int skip = 0;          // queries still to go without a bound pass
	bool take() {
		if (skip > 0) { skip--; return false; }
		return true;
	}
	void record(bool fell_back) {
		recent = ((recent << 1) | (fell_back ? 1u : 0u)) & 0xffu;
		if (fell_back && __builtin_popcount(recent) >= 5) { skip = 64; recent = 0; }
	}
};

} // namespace vk_host

#endif
