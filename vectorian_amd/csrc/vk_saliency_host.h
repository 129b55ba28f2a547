// vk_saliency_host.h -- the booster of a Saliency, compiled on the device (vk_signal_*, vk_corpus_set_saliency): keyword
// signals per slice, smoothed over a document's neighbouring slices, averaged into one multiplicative weight per slice.  One
// definition of every cell for the kernels (vk_saliency.hip), the host driver (vk_corpus.cpp) and the tests.  The reference computes
// these with numpy and scipy per document (vectorian/saliency.py; Document::count_keywords, core/cpp/document.h:276-315):
//   * keyword signal: the tokens of a slice whose vocabulary id is in the keyword set, clipped at max_count, as
//     float32(min(count, max_count)) / float32(max_count) -- one correctly rounded fp32 division.  A token without an id (< 0, or beyond
//     the vocabulary) never counts.  The set is a bitmap over the vocabulary, one bit per id.
//   * MaxFilter(width): scipy.ndimage.maximum_filter(x, size=width) in one dimension, mode "reflect", origin 0: the window of output i
//     is the inputs i - width / 2 .. i - width / 2 + width - 1 (for an even width one more on the left than on the right), an index
//     outside the document reflected about its edges ( .. 1 0 | 0 1 .. n-1 | n-1 n-2 .. ), again and again where the window is longer
//     than the document.  On float32, comparisons only.
//   * ConvFilter(pulse): np.convolve(x, pulse, mode="same") in float64 where the pulse has at most as many taps as the document has
//     slices: y[i] = sum over taps t, ascending, of pulse[t] * x[i + (m - 1) / 2 - t], inputs outside the document counting 0; rounded to
//     float32 when stored.  (numpy does not specify the order of its sum: this header does, and the two agree to the last bit of a
//     float64 or the one before.)  A document with fewer slices than the pulse has taps passes through unchanged.
//   * the average: np.average([ones, s_1 .. s_m], axis=0, weights=w) -- the float64 products w[0] * 1, w[1] * s_1, .. added in list
//     order, divided by the float64 sum of the weights (numpy's: sequential below 8 weights, its unrolled block of 8 from there),
//     rounded to float32 once (Booster holds floats).
// The launch geometry of the three kernels is here too.  No HIP types: tests/test_saliency_host.py compiles this header with g++, plain
// and under AddressSanitizer / UBSan (CPU tier).
#ifndef VK_SALIENCY_HOST_H
#define VK_SALIENCY_HOST_H

#include <cstddef>
#include <cstdint>

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

constexpr int kSalMaxSignals = 8;                      // signal slots of a handle (VK_MAX_SIGNALS of the C-ABI)
enum { SAL_FILTER_MAX = 0, SAL_FILTER_CONV = 1 };      // VK_SIGNAL_FILTER_* of the C-ABI
constexpr int kSalMaxWidth = 4096;                     // slices a filter's window (taps of a pulse) may cover
constexpr int kSalMaxSliceLen = 32767;                 // tokens of a slice (VK_MAX_DOC_LEN)
constexpr int64_t kSalLdsVocab = 524288;               // vocabularies up to this size: the keyword bitmap is staged in LDS (64 KiB)
constexpr int kSalThreads = 256;                       // a workgroup: four waves ...
constexpr int kSalWavesPerBlock = kSalThreads / 64;    // ... one slice each at a time (the keyword kernel); one thread per slice (the others)
constexpr int64_t kSalMaxKeywordBlocks = 1024;         // the keyword kernel's grid: its waves stride over the slices (a block stages the bitmap once)

// ---- the keyword signal

VK_HOST_DEVICE inline int64_t sal_bitmap_words(int64_t vocab_size) { return (vocab_size + 31) / 32; }
// whether token id `id` is a keyword: a token without an id, or with one outside the vocabulary, is none
VK_HOST_DEVICE inline bool sal_is_keyword(const uint32_t *bitmap, int64_t vocab_size, int32_t id) {
	return id >= 0 && (int64_t)id < vocab_size && ((bitmap[id >> 5] >> (id & 31)) & 1u) != 0;
}
inline void sal_bitmap_set(uint32_t *bitmap, int32_t id) { bitmap[id >> 5] |= 1u << (id & 31); }
// float32(min(count, max_count)) / max_count
VK_HOST_DEVICE inline float sal_signal_value(int32_t count, int32_t max_count) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	return (float)(count < max_count ? count : max_count) / (float)max_count;
}
// the whole signal of one slice on the host: what a wave computes with ballots
inline float sal_keyword_signal(const int32_t *ids, int64_t start, int64_t end, const uint32_t *bitmap, int64_t vocab_size, int32_t max_count) {
	int32_t count = 0;
	for (int64_t t = start; t < end; t++) count += sal_is_keyword(bitmap, vocab_size, ids[t]) ? 1 : 0;
	return sal_signal_value(count, max_count);
}

// ---- the filters, over one document: n slices at x[0 .. n)

// index i of a document of n >= 1 slices, reflected about its edges ("reflect": the edge value is repeated), any i
VK_HOST_DEVICE inline int64_t sal_reflect(int64_t i, int64_t n) {
	const int64_t period = 2 * n;
	int64_t m = i % period;
	if (m < 0) m += period;
	return m < n ? m : period - 1 - m;
}
// first input of output i's window of `width` slices; the window is [first, first + width)
VK_HOST_DEVICE inline int64_t sal_max_first(int64_t i, int32_t width) { return i - width / 2; }
VK_HOST_DEVICE inline float sal_max_filter(const float *x, int64_t n, int64_t i, int32_t width) {
	const int64_t first = sal_max_first(i, width);
	float best = x[sal_reflect(first, n)];
	for (int32_t k = 1; k < width; k++) {
		const float v = x[sal_reflect(first + k, n)];
		best = v > best ? v : best;
	}
	return best;
}

// whether the convolution runs on a document of n slices; else its signal passes through
VK_HOST_DEVICE inline bool sal_conv_applies(int32_t taps, int64_t n) { return (int64_t)taps <= n; }
// the taps that meet an input inside the document, for output i: tap t reads x[i + (taps - 1) / 2 - t]
VK_HOST_DEVICE inline int32_t sal_conv_first_tap(int64_t i, int32_t taps, int64_t n) {
	const int64_t t = i + (taps - 1) / 2 - (n - 1);   // the input index is <= n - 1
	return (int32_t)(t > 0 ? t : 0);
}
VK_HOST_DEVICE inline int32_t sal_conv_end_tap(int64_t i, int32_t taps, int64_t n) {
	const int64_t t = i + (taps - 1) / 2 + 1;         // the input index is >= 0
	return (int32_t)(t < (int64_t)taps ? t : (int64_t)taps);
}
VK_HOST_DEVICE inline float sal_conv_same(const float *x, int64_t n, int64_t i, const double *pulse, int32_t taps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const int64_t centre = i + (taps - 1) / 2;
	double acc = 0.0;
	for (int32_t t = sal_conv_first_tap(i, taps, n), e = sal_conv_end_tap(i, taps, n); t < e; t++) acc = acc + pulse[t] * (double)x[centre - t];
	return (float)acc;
}
// one cell of a filtered signal
VK_HOST_DEVICE inline float sal_filter_cell(int32_t kind, const float *x, int64_t n, int64_t i, int32_t width, const double *pulse) {
	if (kind == SAL_FILTER_MAX) return sal_max_filter(x, n, i, width);
	return sal_conv_applies(width, n) ? sal_conv_same(x, n, i, pulse, width) : x[i];
}
// the document of slice s: the d with doc_off[d] <= s < doc_off[d + 1] (doc_off [n_docs + 1], ascending; empty documents are skipped)
VK_HOST_DEVICE inline int64_t sal_doc_of(const int64_t *doc_off, int64_t n_docs, int64_t s) {
	int64_t lo = 0, hi = n_docs;   // doc_off[lo] <= s < doc_off[hi]
	while (hi - lo > 1) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (doc_off[mid] <= s) lo = mid; else hi = mid;
	}
	return lo;
}
// np.sum over n float64 (the scale of np.average: its weights' sum) -- sequential below 8 addends, numpy's block of 8 from there.
// (A pulse arrives divided by its sum already: ConvFilter.__init__ does that with numpy itself.)
inline double sal_numpy_sum(const double *w, int64_t n) {
	if (n < 8) {
		double s = 0.0;
		for (int64_t i = 0; i < n; i++) s = s + w[i];
		return s;
	}
	if (n <= 128) {   // numpy's pairwise block: eight running sums, combined as a tree, the rest added one by one
		double r[8];
		for (int k = 0; k < 8; k++) r[k] = w[k];
		int64_t i = 8;
		for (; i + 8 <= n; i += 8) for (int k = 0; k < 8; k++) r[k] = r[k] + w[i + k];
		double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
		for (; i < n; i++) s = s + w[i];
		return s;
	}
	const int64_t half = (n / 2) & ~(int64_t)7;
	return sal_numpy_sum(w, half) + sal_numpy_sum(w + half, n - half);
}

// ---- the average: weights[0] of the ones, weights[1 + k] of signal k; wsum their sum (sal_numpy_sum)

// (the loop runs over all the slots with constant indices once unrolled: a kernel's argument struct stays where it is)
// signals: kSalMaxSignals pointers (those from n_signals on are not read); weights: kSalMaxSignals + 1 doubles
template <typename Signals, typename Weights>
VK_HOST_DEVICE inline float sal_boost_cell(const Signals &signals, int32_t n_signals, const Weights &weights, double wsum, int64_t s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	double acc = weights[0] * 1.0;
	VK_UNROLL
	for (int32_t k = 0; k < kSalMaxSignals; k++)
		if (k < n_signals) acc = acc + weights[1 + k] * (double)signals[k][s];
	return (float)(acc / wsum);
}
// what the bound pass asks of a booster (a score is monotone in its cells only then): not negative, not NaN
VK_HOST_DEVICE inline bool sal_boost_bounds_ok(float b) { return b >= 0.0f; }

// ---- the launch geometry

// the keyword kernel: wave w of block b takes the slices sal_keyword_first(b, w), + sal_keyword_stride(grid), ..
inline int64_t sal_keyword_grid(int64_t n_slices) {
	const int64_t blocks = (n_slices + kSalWavesPerBlock - 1) / kSalWavesPerBlock;
	return blocks < kSalMaxKeywordBlocks ? blocks : kSalMaxKeywordBlocks;
}
VK_HOST_DEVICE inline int64_t sal_keyword_first(int64_t block, int wave) { return block * kSalWavesPerBlock + wave; }
VK_HOST_DEVICE inline int64_t sal_keyword_stride(int64_t grid) { return grid * kSalWavesPerBlock; }
// the filter and the average kernels: one thread per slice (per row of the slice table)
inline int64_t sal_cell_grid(int64_t n) { return (n + kSalThreads - 1) / kSalThreads; }
VK_HOST_DEVICE inline int64_t sal_cell_of(int64_t block, int thread) { return block * kSalThreads + thread; }

// ---- whole arrays on the host: what the kernels compute, cell by cell

inline void sal_filter(int32_t kind, const float *x, float *y, const int64_t *doc_off, int64_t n_docs, int32_t width, const double *pulse) {
	for (int64_t d = 0; d < n_docs; d++) {
		const int64_t a = doc_off[d], n = doc_off[d + 1] - a;
		for (int64_t i = 0; i < n; i++) y[a + i] = sal_filter_cell(kind, x + a, n, i, width, pulse);
	}
}

// ---- the arguments that need no device: 0, or the status with *why set
enum { SAL_OK = 0, SAL_INVALID = 1 };   // (VK_OK, VK_ERR_INVALID)
inline int sal_check_docs(const int64_t *doc_off, int64_t n_docs, int64_t n_slices, const char **why) {
	if (n_docs < 0 || (n_docs == 0 && n_slices > 0)) { *why = "the documents do not cover the slices"; return SAL_INVALID; }
	if (n_docs == 0) return SAL_OK;
	if (doc_off[0] != 0 || doc_off[n_docs] != n_slices) { *why = "the document offsets must start at 0 and end at n_sentences"; return SAL_INVALID; }
	for (int64_t d = 0; d < n_docs; d++)
		if (doc_off[d] > doc_off[d + 1]) { *why = "the document offsets must ascend"; return SAL_INVALID; }
	return SAL_OK;
}

} // namespace vk_host

#endif
