// vk_pool_host.h -- span vectors pooled from token rows (vk_corpus_append_pooled): the mean, minimum or maximum of a span's
// token vectors, AggregatedTokenImpl of the reference (vectorian/embedding/span.py:27-93), one definition for the host and the device.
// The reference calls agg(v, axis=0) on the float32 array [n x d] of the span's UNMODIFIED token vectors; pool_fold() / pool_finish()
// are that call, per feature:
//   * MEAN: acc = row[0], then acc = acc + row[i] in fp32 for i ascending, then acc / (float)n -- what np.mean(v, axis=0) computes on
//     float32 for d >= 2 (a row-by-row fp32 sum, divided once by float32(n); at d = 1 numpy sums pairwise).  One rounding
//     per operation, nothing contracted or reassociated, the division correctly rounded.  (float)n is exact up to kPoolMaxSpanLen.
//   * MIN / MAX: numpy's minimum / maximum folded in token order; a NaN component makes the result NaN.
//   * a span without tokens is a row of NaN (the reference's out.fill(np.nan) stays).
//   * bf16 rows are widened exactly.
//   * gathered rows: a span's rows are vocab[ids[t]] for t in [start, end); the zero row of an out-of-vocabulary word takes part in n
//     and in the extremum.
// The launch geometry of vk_pool_spans_kernel (vk_pool.hip) is here too: one wave per span, kPoolSpansPerBlock spans per workgroup; a
// lane owns `vec` consecutive features of each of kPoolChunksPerPass chunks of 64 * vec features, and a wave takes a row in passes of
// kPoolChunksPerPass chunks.  No HIP types: tests/test_pool_host.py compiles this header with g++, plain and under AddressSanitizer /
// UBSan, holds pool_spans() against numpy and enumerates the grid (CPU tier).
#ifndef VK_POOL_HOST_H
#define VK_POOL_HOST_H

#include <cstddef>
#include <cstdint>
#include <cstring>

#ifndef VK_HOST_DEVICE
#ifdef __HIPCC__
#define VK_HOST_DEVICE __host__ __device__
#define VK_UNROLL _Pragma("unroll")
#else
#define VK_HOST_DEVICE
#define VK_UNROLL
#endif
#endif

namespace vk_host {

// the aggregates (VK_POOL_* of the C-ABI)
enum { POOL_MEAN = 0, POOL_MIN = 1, POOL_MAX = 2 };

constexpr int64_t kPoolMaxSpanLen = (int64_t)1 << 24;   // tokens of a span: (float)n is exact
constexpr int kPoolMaxD = 8192;                         // features of a row (vk_corpus_create's bound)
constexpr int kPoolThreads = 256;                       // a workgroup: four waves ...
constexpr int kPoolSpansPerBlock = kPoolThreads / 64;   // ... one span each
constexpr int kPoolChunksPerPass = 4;                   // feature chunks a lane holds accumulators for at a time
constexpr int kPoolRowsInFlight = 4;                    // token rows a wave loads before it folds them, in order
constexpr int kPoolIdBatch = 64;                        // token ids a wave loads at a time, one per lane (gathered rows)

inline bool pool_agg_ok(int32_t agg) { return agg == POOL_MEAN || agg == POOL_MIN || agg == POOL_MAX; }

VK_HOST_DEVICE inline float pool_widen_bf16(uint16_t b) {
	const uint32_t u = (uint32_t)b << 16;
#ifdef __HIP_DEVICE_COMPILE__
	return __builtin_bit_cast(float, u);
#else
	float f;
	memcpy(&f, &u, 4);
	return f;
#endif
}

VK_HOST_DEVICE inline float pool_nan() { return __builtin_nanf(""); }

// one token's step: acc holds the aggregate of the rows before x
template <int AGG>
VK_HOST_DEVICE inline float pool_fold(float acc, float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (AGG == POOL_MEAN) return acc + x;
	// np.minimum / np.maximum: the first operand where it is NaN or wins the comparison, else the second (a NaN there comes through)
	if (AGG == POOL_MIN) return (acc != acc || acc <= x) ? acc : x;
	return (acc != acc || acc >= x) ? acc : x;
}

// after the last token of a span of n >= 1 tokens
template <int AGG>
VK_HOST_DEVICE inline float pool_finish(float acc, int64_t n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (AGG == POOL_MEAN) return acc / (float)n;
	return acc;
}

// ---- the launch geometry

// features a lane loads at once: 4 (16 bytes of fp32, 8 of bf16) where every row starts on such a boundary, else 1
inline int pool_vec(int d, int elem_bytes, uintptr_t base) { return (d % 4 == 0 && base % (uintptr_t)(4 * elem_bytes) == 0) ? 4 : 1; }
VK_HOST_DEVICE inline int pool_chunk_features(int vec) { return 64 * vec; }
VK_HOST_DEVICE inline int pool_pass_features(int vec) { return kPoolChunksPerPass * pool_chunk_features(vec); }
VK_HOST_DEVICE inline int pool_passes(int d, int vec) { return (d + pool_pass_features(vec) - 1) / pool_pass_features(vec); }
// feature chunks a lane walks per row
VK_HOST_DEVICE inline int pool_chunks(int d, int vec) { return (d + pool_chunk_features(vec) - 1) / pool_chunk_features(vec); }
inline int64_t pool_grid(int64_t n_spans) { return (n_spans + kPoolSpansPerBlock - 1) / kPoolSpansPerBlock; }
// the span of wave `wave` of workgroup `block`; >= n_spans: the wave has none
VK_HOST_DEVICE inline int64_t pool_span_of(int64_t block, int wave) { return block * kPoolSpansPerBlock + wave; }
// the first of the `vec` features lane `lane` owns in chunk `chunk` of pass `pass`; >= d: none
VK_HOST_DEVICE inline int pool_feature_of(int pass, int chunk, int lane, int vec) {
	return (pass * kPoolChunksPerPass + chunk) * 64 * vec + lane * vec;
}

// ---- the whole aggregate on the host: out [n_spans x d].  rows: [n_rows x d] float, or uint16 bf16 bits (bf16 = true); ids: null, or
// the row of every token.  What the kernel computes, cell by cell.
template <int AGG>
inline void pool_spans_agg(const void *rows, bool bf16, int d, const int32_t *ids, const int64_t *start, const int64_t *end, int64_t n_spans, float *out) {
	for (int64_t s = 0; s < n_spans; s++) {
		const int64_t a = start[s], b = end[s];
		for (int k = 0; k < d; k++) {
			float acc = pool_nan();
			for (int64_t t = a; t < b; t++) {
				const int64_t r = ids ? (int64_t)ids[t] : t;
				const float x = bf16 ? pool_widen_bf16(((const uint16_t *)rows)[r * d + k]) : ((const float *)rows)[r * d + k];
				acc = t == a ? x : pool_fold<AGG>(acc, x);
			}
			out[s * d + k] = b > a ? pool_finish<AGG>(acc, b - a) : acc;
		}
	}
}

inline void pool_spans(int32_t agg, const void *rows, bool bf16, int d, const int32_t *ids, const int64_t *start, const int64_t *end, int64_t n_spans, float *out) {
	switch (agg) {
	case POOL_MEAN: pool_spans_agg<POOL_MEAN>(rows, bf16, d, ids, start, end, n_spans, out); break;
	case POOL_MIN: pool_spans_agg<POOL_MIN>(rows, bf16, d, ids, start, end, n_spans, out); break;
	default: pool_spans_agg<POOL_MAX>(rows, bf16, d, ids, start, end, n_spans, out); break;
	}
}

// ---- the arguments of vk_corpus_append_pooled that need no device: 0, or the status with *why set
enum { POOL_OK = 0, POOL_INVALID = 1, POOL_UNSUPPORTED = 2 };   // (VK_OK, VK_ERR_INVALID, VK_ERR_UNSUPPORTED)
inline int pool_check_spans(int64_t n_rows, const int32_t *ids, int64_t n_ids, const int64_t *start, const int64_t *end, int64_t n_spans, const char **why) {
	const int64_t limit = ids ? n_ids : n_rows;
	bool too_long = false;
	for (int64_t s = 0; s < n_spans; s++) {
		if (start[s] > end[s]) { *why = "a span starts after its end"; return POOL_INVALID; }
		if (start[s] < 0 || end[s] > limit) { *why = ids ? "a span outside the token ids" : "a span outside the rows"; return POOL_INVALID; }
		too_long = too_long || end[s] - start[s] > kPoolMaxSpanLen;
	}
	for (int64_t t = 0; ids && t < n_ids; t++)
		if (ids[t] < 0 || (int64_t)ids[t] >= n_rows) { *why = "a token id outside the rows"; return POOL_INVALID; }
	if (too_long) { *why = "a span of more than 2^24 tokens: its length is not exact in fp32"; return POOL_UNSUPPORTED; }
	return POOL_OK;
}

} // namespace vk_host

#endif
