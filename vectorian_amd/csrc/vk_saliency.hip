// vk_saliency.hip -- the booster of a Saliency, compiled on the device (vk_signal_keywords, vk_signal_filter, vk_corpus_set_saliency;
// DESIGN 18): three small kernels bound by the bytes they read -- the token ids once per keyword signal, a signal once per filter, the
// signals once for the average.  The arithmetic of every cell and the launch geometry: vk_saliency_host.h.
#include "vk_common.hip.h"
#include "vk_saliency_host.h"

// One wave per slice at a time (vk_host::sal_keyword_first / sal_keyword_stride): lane l looks at token a + l of the slice, a ballot
// and a population count add up the hits; a slice of more than 64 tokens takes further trips, an empty one none (its signal is 0).
// Overlapping windows each read their own range.  STAGED: the keyword bitmap fits 64 KiB and every workgroup copies it into LDS once,
// before its waves stride over the slices -- a hit test is then one LDS read; otherwise the bitmap is read from global memory (the
// caches keep what the corpus's frequent words touch).  row_of_slice: the row of the slice table of a slice (null: rows are slices).
template <bool STAGED>
__global__ __launch_bounds__(vk_host::kSalThreads) void vk_keyword_signal_kernel(const int32_t *__restrict__ ids, const int32_t *__restrict__ sent_start,
	const int32_t *__restrict__ sent_end, const int32_t *__restrict__ row_of_slice, int64_t n_slices, const uint32_t *__restrict__ bitmap, int64_t vocab_size,
	int32_t max_count, float *__restrict__ signal) {
	extern __shared__ uint32_t staged_bitmap[];
	const uint32_t *bits = bitmap;
	if constexpr (STAGED) {
		const int words = (int)vk_host::sal_bitmap_words(vocab_size);
		for (int i = threadIdx.x; i < words; i += vk_host::kSalThreads) staged_bitmap[i] = bitmap[i];
		__syncthreads();
		bits = staged_bitmap;
	}
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int64_t stride = vk_host::sal_keyword_stride(gridDim.x);
#pragma unroll 1
	for (int64_t s = vk_host::sal_keyword_first(blockIdx.x, wave); s < n_slices; s += stride) {
		const int64_t row = row_of_slice ? (int64_t)row_of_slice[s] : s;
		const int64_t a = sent_start[row], b = sent_end[row];
		int32_t count = 0;
#pragma unroll 1
		for (int64_t t0 = a; t0 < b; t0 += 64) {
			const int64_t t = t0 + lane;
			const bool hit = t < b && vk_host::sal_is_keyword(bits, vocab_size, ids[t]);
			count += __popcll(__ballot(hit));
		}
		if (lane == 0) signal[s] = vk_host::sal_signal_value(count, max_count);
	}
}

// One thread per slice: its document by bisection of the offsets, then the cell of the header over the document's segment of x.
// y is another buffer than x: a cell reads its neighbours' inputs.
__global__ __launch_bounds__(vk_host::kSalThreads) void vk_signal_filter_kernel(const float *__restrict__ x, float *__restrict__ y,
	const int64_t *__restrict__ doc_off, int64_t n_docs, int64_t n_slices, int32_t kind, int32_t width, const double *__restrict__ pulse) {
	const int64_t s = vk_host::sal_cell_of(blockIdx.x, threadIdx.x);
	if (s >= n_slices) return;
	const int64_t doc = vk_host::sal_doc_of(doc_off, n_docs, s);
	const int64_t a = doc_off[doc], n = doc_off[doc + 1] - a;
	y[s] = vk_host::sal_filter_cell(kind, x + a, n, s - a, width, pulse);
}

// One thread per row of the slice table (and of the 8 rows of padding behind it): the float64 average of the header for the row's
// slice, 1 for a row of padding.  The same value goes to the slice's place in `slices` (the host's copy is read from there), and a
// boost that is negative or NaN raises *bad (every writer stores the same word).
__global__ __launch_bounds__(vk_host::kSalThreads) void vk_boost_average_kernel(VkBoostAverageArgs p) {
	const int64_t e = vk_host::sal_cell_of(blockIdx.x, threadIdx.x);
	if (e >= p.n_entries + 8) return;
	const int64_t s = e >= p.n_entries ? -1 : p.entry_sent ? (int64_t)p.entry_sent[e] : e;
	float b = 1.0f;
	if (s >= 0) {
		b = vk_host::sal_boost_cell(p.signals, p.n_signals, p.weights, p.wsum, s);
		p.slices[s] = b;
		if (!vk_host::sal_boost_bounds_ok(b)) *p.bad = 1;
	}
	p.rows[e] = b;
}

extern "C" hipError_t vk_launch_keyword_signal(const int32_t *ids, const int32_t *sent_start, const int32_t *sent_end, const int32_t *row_of_slice,
	int64_t n_slices, const uint32_t *bitmap, int64_t vocab_size, int32_t max_count, float *signal, hipStream_t stream) {
	if (n_slices <= 0) return hipSuccess;
	if (!sent_start || !sent_end || !bitmap || !signal || vocab_size < 1 || max_count < 1) return hipErrorInvalidValue;   // (ids may be null: a corpus without tokens reads none)
	const unsigned grid = (unsigned)vk_host::sal_keyword_grid(n_slices);
	if (vocab_size <= vk_host::kSalLdsVocab)
		vk_keyword_signal_kernel<true><<<grid, vk_host::kSalThreads, (size_t)vk_host::sal_bitmap_words(vocab_size) * 4, stream>>>(ids, sent_start, sent_end,
			row_of_slice, n_slices, bitmap, vocab_size, max_count, signal);
	else
		vk_keyword_signal_kernel<false><<<grid, vk_host::kSalThreads, 0, stream>>>(ids, sent_start, sent_end, row_of_slice, n_slices, bitmap, vocab_size,
			max_count, signal);
	return hipGetLastError();
}

extern "C" hipError_t vk_launch_signal_filter(const float *x, float *y, const int64_t *doc_off, int64_t n_docs, int64_t n_slices, int32_t kind,
	int32_t width, const double *pulse, hipStream_t stream) {
	if (n_slices <= 0) return hipSuccess;
	if (!x || !y || x == y || !doc_off || n_docs < 1 || width < 1 || width > vk_host::kSalMaxWidth ||
		(kind != vk_host::SAL_FILTER_MAX && kind != vk_host::SAL_FILTER_CONV) || (kind == vk_host::SAL_FILTER_CONV && !pulse)) return hipErrorInvalidValue;
	const int64_t grid = vk_host::sal_cell_grid(n_slices);
	if (grid > 0x7fffffffll) return hipErrorInvalidValue;
	vk_signal_filter_kernel<<<(unsigned)grid, vk_host::kSalThreads, 0, stream>>>(x, y, doc_off, n_docs, n_slices, kind, width, pulse);
	return hipGetLastError();
}

extern "C" hipError_t vk_launch_boost_average(const VkBoostAverageArgs *p, hipStream_t stream) {
	if (!p || !p->rows || !p->slices || !p->bad || p->n_signals < 0 || p->n_signals > vk_host::kSalMaxSignals || p->n_entries < 0) return hipErrorInvalidValue;
	for (int k = 0; k < p->n_signals; k++) if (!p->signals[k]) return hipErrorInvalidValue;
	const int64_t grid = vk_host::sal_cell_grid(p->n_entries + 8);
	if (grid > 0x7fffffffll) return hipErrorInvalidValue;
	vk_boost_average_kernel<<<(unsigned)grid, vk_host::kSalThreads, 0, stream>>>(*p);
	return hipGetLastError();
}
