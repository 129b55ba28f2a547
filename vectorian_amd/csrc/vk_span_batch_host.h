// vk_span_batch_host.h -- the batched span pass (vk_span_batch_kernel): which batches take it, how many queries one
// workgroup stages in LDS (a "fill"), how many queries one score matrix holds (a "chunk"), the grid.  vk_batch.cpp routes and sizes
// its workspace from it, vk_span_batch.hip its launches; nothing else computes these numbers.  Host only, no HIP types:
// tests/test_span_batch_host.py compiles it with g++ and enumerates the shapes (CPU tier).
#ifndef VK_SPAN_BATCH_HOST_H
#define VK_SPAN_BATCH_HOST_H

#include <cstddef>
#include <cstdint>

namespace vk_host {

constexpr size_t kSpanBatchLdsPerCu = 160 * 1024;      // the LDS of a CU
constexpr int kSpanBatchBlocksPerCu = 1;                 // one workgroup per CU ...
constexpr int kSpanBatchThreads = 512;                   // ... of 8 waves, two per SIMD: the CU's waves share one set of staged query tiles
constexpr size_t kSpanBatchLdsBudget = kSpanBatchLdsPerCu / kSpanBatchBlocksPerCu;   // query tiles of one workgroup
// query tiles a workgroup may stage: the kernel is instantiated for these counts (a wave keeps two accumulators per staged tile)
constexpr int kSpanBatchFillSet[] = {8, 6, 4, 2, 1};
constexpr int kSpanBatchMaxFillTiles = kSpanBatchFillSet[0];
constexpr int kSpanBatchTilesPerWave = 2;                // span tiles a wave holds per read of a query fragment
constexpr int kSpanBatchRun = 4;                         // consecutive pairs of span tiles a wave takes in turn (as VK_SPAN_RUN)
constexpr size_t kSpanBatchMatrixCap = (size_t)1 << 30;  // bytes of the score matrix
constexpr int kSpanBatchRoute = 4;                       // batch_state[VK_BS_ROUTE] of this route

// ---- what the decision reads, and nothing else
struct span_batch_corpus {
	bool finalized = false, contextual = false, contiguous = false, has_entry_sent = false, sourced = false, chained = false;
	int uniform_len = 0, n_long_groups = 0, tile_bytes = 0;
	int64_t n = 0;   // rows of the slice table
};
struct span_batch_query {
	int len_t = 0;
	bool align = false, local = false, tagged = false, submatch = false, boost = false, want_flow = false, only = false;
	int max_matches = 0;
	float min_score = 0.0f;
};

// query tiles (16 queries each) one workgroup stages: the largest count of the set that fits the budget; 0: not even one
inline int span_batch_fill_tiles(int tile_bytes) {
	if (tile_bytes < 1) return 0;
	for (const int t : kSpanBatchFillSet)
		if ((size_t)t * (size_t)tile_bytes <= kSpanBatchLdsBudget) return t;
	return 0;
}
// the instantiation that serves a launch of `tiles` query tiles per workgroup: the smallest count of the set that holds them
inline int span_batch_form_tiles(int tiles) {
	int form = kSpanBatchMaxFillTiles;
	for (const int t : kSpanBatchFillSet)
		if (t >= tiles) form = t;
	return form;
}
inline int span_batch_fill_queries(int tile_bytes) { return 16 * span_batch_fill_tiles(tile_bytes); }
inline size_t span_batch_lds_bytes(int tile_bytes, int fill_tiles) { return (size_t)tile_bytes * (size_t)fill_tiles; }

// a row of the score matrix: the spans rounded up to whole tiles
inline int64_t span_batch_n_pad(int64_t n) { return (n + 15) / 16 * 16; }
// queries per score matrix: the largest multiple of 16 whose rows stay within `cap` bytes; 0: 16 rows exceed it
inline int64_t span_batch_chunk(int64_t n, size_t cap = kSpanBatchMatrixCap) {
	const int64_t n_pad = span_batch_n_pad(n);
	if (n_pad < 1) return 0;
	const int64_t rows = (int64_t)(cap / 4 / (size_t)n_pad);
	return rows / 16 * 16;
}
inline size_t span_batch_matrix_floats(int64_t n, int64_t queries) { return (size_t)span_batch_n_pad(n) * (size_t)queries; }
// The kernel addresses a cell of the matrix by an unsigned 32-bit index: the cap holds 2^28 floats.  (A tile of the corpus is
// addressed in 64 bits: 2^27 spans of 1,024 fp32 features are 2^39 bytes.)
static_assert(kSpanBatchMatrixCap / 4 <= ((size_t)1 << 32), "a cell's index fits 32 bits");
inline bool span_batch_index_fits_u32(int64_t n, int64_t queries) { return span_batch_matrix_floats(n, queries) <= ((size_t)1 << 32); }

inline bool span_batch_corpus_ok(const span_batch_corpus &c, size_t cap = kSpanBatchMatrixCap) {
	return c.finalized && c.contextual && c.contiguous && c.uniform_len == 1 && c.n_long_groups == 0 && !c.has_entry_sent && !c.sourced &&
		!c.chained && c.n >= 1 && span_batch_fill_tiles(c.tile_bytes) >= 1 && span_batch_chunk(c.n, cap) >= 16;
}
// one query of the batch beside query 0.  (The span condition of vk_route_host.h reads neither the gap costs nor min_score -- the
// local alignment of a 1 x 1 matrix has no gap -- so neither does this; vk_validate_query has looked at the gaps.)
inline bool span_batch_query_ok(const span_batch_query &q, const span_batch_query &q0) {
	return q.len_t == 1 && q.align && q.local && !q.tagged && !q.submatch && !q.boost && !q.want_flow && !q.only &&
		q.max_matches == q0.max_matches && q.min_score == q0.min_score;
}

// workgroups over the span tiles (grid.x; grid.y counts the fills of a chunk): a wave takes runs of kSpanBatchRun pairs of tiles
inline int span_batch_grid(int64_t n, int cus) {
	const int64_t tiles = span_batch_n_pad(n) / 16, per_wave = (int64_t)kSpanBatchTilesPerWave * kSpanBatchRun;
	const int64_t waves = kSpanBatchThreads / 64, runs = (tiles + per_wave - 1) / per_wave, want = (runs + waves - 1) / waves;
	const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * kSpanBatchBlocksPerCu;
	const int64_t g = want < cap ? want : cap;
	return (int)(g < 1 ? 1 : g);
}

} // namespace vk_host

#endif
