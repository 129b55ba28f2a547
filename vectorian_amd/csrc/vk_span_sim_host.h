// vk_span_sim_host.h -- the span index under a VectorSim that is not the bare cosine (vk_corpus_set_span_sim): the grid
// of vk_span_sim_kernel / vk_span_ops_kernel (vk_span_sim.hip), which tiles a wave takes, the LDS of the staged query, the floor of
// the selection, which queries are span-shaped, and the cell of a source AS THE KERNEL STREAMS IT -- zero-padded blocks of 16
// features, one double partial sum per lane (the residue class k mod 4 of one row), two exchanges across the four lanes of a row.
// vk_query.cpp reads the predicates, vk_span_sim.hip the geometry; nothing else computes these numbers.  No HIP types:
// tests/test_span_sim_host.py compiles the header with g++, plain and under AddressSanitizer / UBSan, holds the streamed cell against
// vk_host::sim_src_cell bit for bit and enumerates the grid walk (CPU tier).
#ifndef VK_SPAN_SIM_HOST_H
#define VK_SPAN_SIM_HOST_H

#include "vk_sim_ops_host.h"
#include "vk_sim_src_host.h"

#include <cstdint>
#include <vector>

namespace vk_host {

constexpr int kSpanSimThreads = 256;        // four waves per workgroup
constexpr int kSpanSimWaves = kSpanSimThreads / 64;
constexpr int kSpanSimRun = 4;              // consecutive tiles a wave takes in turn (as VK_SPAN_RUN of vk_span_kernel)
constexpr int kSpanSimBlocksPerCu = 3;      // 12 waves per CU, three per SIMD: as vk_span_kernel is launched
constexpr int kSpanSimMaxVgprs = 168;       // ... which a kernel of at most this many VGPRs reaches (512 / 3, in steps of 8)
constexpr int kSpanSimDepth = 8;            // blocks of 1 KiB a wave has in flight before the first use: 8 KiB, the read probe's pattern

// the span similarity of a handle: the source (the cosine: the MFMA chain on the unit tiles) and the chain.  active(): the handle is
// a span corpus under it -- (cosine, no operators) is the handle as it always was
struct span_sim {
	sim_src src{VK_SIMSRC_COSINE, 0.0f};
	sim_ops ops{};
	bool active() const { return src.kind != VK_SIMSRC_COSINE || ops.n > 0; }
	bool sourced() const { return src.kind != VK_SIMSRC_COSINE; }
};

// tiles of 16 spans
VK_HOST_DEVICE inline int64_t span_sim_tiles(int64_t n) { return (n + 15) >> 4; }
// workgroups: one wave per run of kSpanSimRun tiles, at most blocks_per_cu resident workgroups per CU (the rest: grid-stride)
inline int span_sim_grid(int64_t n, int cus, int blocks_per_cu = kSpanSimBlocksPerCu) {
	const int64_t runs = (span_sim_tiles(n) + kSpanSimRun - 1) / kSpanSimRun;
	const int64_t want = (runs + kSpanSimWaves - 1) / kSpanSimWaves > 0 ? (runs + kSpanSimWaves - 1) / kSpanSimWaves : 1;
	const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * (blocks_per_cu > 0 ? blocks_per_cu : 1);
	return (int)(want < cap ? want : cap);
}
// the walk of wave `wave` of workgroup `block`: runs first, first + stride, .. while run * kSpanSimRun < tiles; run r holds the tiles
// [r * kSpanSimRun, min((r + 1) * kSpanSimRun, tiles))
VK_HOST_DEVICE inline int64_t span_sim_first_run(int64_t block, int wave) { return block * kSpanSimWaves + wave; }
VK_HOST_DEVICE inline int64_t span_sim_run_stride(int64_t grid) { return grid * kSpanSimWaves; }
VK_HOST_DEVICE inline int64_t span_sim_run_begin(int64_t run) { return run * kSpanSimRun; }
VK_HOST_DEVICE inline int64_t span_sim_run_end(int64_t run, int64_t tiles) { return (run + 1) * kSpanSimRun < tiles ? (run + 1) * kSpanSimRun : tiles; }

// the unmodified rows: blocks of 16 features x 16 rows in 1 KiB; the staged query: 64 bytes per block (lane group g reads 16 bytes)
VK_HOST_DEVICE inline int span_sim_blocks(int d) { return (d + 15) >> 4; }
inline int span_sim_raw_tile_bytes(int d) { return span_sim_blocks(d) * 1024; }
inline size_t span_sim_lds_bytes(int d) { return (size_t)span_sim_blocks(d) * 64; }   // at most 4 KiB (kSimSrcMaxD)
// where feature 16 b + 4 s + g of the query sits in the staged copy (floats): slot (4 b + g) of four floats, element s
VK_HOST_DEVICE inline int span_sim_q_slot(int b, int g) { return 4 * b + g; }

// the floor of the selection: admission is score > max(min_score, 0) -- NaN and negative values are never matches
inline float span_sim_floor(float min_score) { return min_score > 0.0f ? min_score : 0.0f; }

// what a query on a span-sim handle must be; null, or what was asked that the route does not serve
struct span_sim_query {
	int32_t algorithm = VK_ALG_ALIGN, locality = VK_LOCAL, len_t = 1;
	int32_t uniform_len = 1;   // of the corpus
	bool tagged = false, submatch = false, boost = false, want_flow = false, only = false, sim_rows = false;
};
inline const char *span_sim_refusal(const span_sim_query &q) {
	if (q.uniform_len != 1) return "slices of more or less than one row";
	if (q.len_t != 1) return "a query of more than one token";
	if (q.algorithm == VK_ALG_RWMD) return "VK_ALG_RWMD";
	if (q.algorithm != VK_ALG_ALIGN) return "an algorithm other than VK_ALG_ALIGN";
	if (q.locality == VK_GLOBAL) return "global alignment";
	if (q.locality != VK_LOCAL) return "an alignment that is not local";
	if (q.tagged) return "tag weights";
	if (q.submatch) return "a submatch weight";
	if (q.boost) return "a booster";
	if (q.only) return "only_slices";   // (before want_flow, which a query that lists slices has to set)
	if (q.want_flow) return "want_flow";
	if (q.sim_rows) return "the winners' similarity rows";
	return nullptr;
}
inline bool span_sim_shaped(const span_sim_query &q) { return span_sim_refusal(q) == nullptr; }

// ---- the cell of a source as vk_span_sim_kernel streams it: span row a, query q, d features
// Both sides zero-padded to whole blocks.  Lane (g, i) of the wave owns row i's features 16 b + 4 s + g: one double accumulator
// (two under the sqrt-cosine), adds in ascending k -- s ascending inside a block, blocks ascending.  The four lanes of a row combine
// with the partner 16 lanes away (g ^ 1), then the partner 32 lanes away (g ^ 2): every lane ends with (s0 + s1) + (s2 + s3), in one
// operand order or the other.  sum_q: sim_src_abs_sum of the query, from the host.
template <int FORM>
inline float span_sim_cell_streamed(const float *a, const float *q, int d, float p, float sum_q) {
	const int nb = span_sim_blocks(d);
	std::vector<float> ap((size_t)nb * 16, 0.0f), qp((size_t)nb * 16, 0.0f);
	for (int k = 0; k < d; k++) { ap[(size_t)k] = a[k]; qp[(size_t)k] = q[k]; }
	double acc[4] = {0.0, 0.0, 0.0, 0.0}, abs_a[4] = {0.0, 0.0, 0.0, 0.0};
	for (int g = 0; g < 4; g++)
		for (int b = 0; b < nb; b++)
			for (int s = 0; s < 4; s++) {
				const int k = 16 * b + 4 * s + g;
				acc[g] += (double)sim_src_term<FORM>(ap[(size_t)k], qp[(size_t)k], p);
				if (FORM == SIM_SRC_SQRT_COS) abs_a[g] += (double)fabsf(ap[(size_t)k]);
			}
	double x16[4], x32[4], y16[4], y32[4];
	for (int g = 0; g < 4; g++) { x16[g] = acc[g] + acc[g ^ 1]; y16[g] = abs_a[g] + abs_a[g ^ 1]; }
	for (int g = 0; g < 4; g++) { x32[g] = x16[g] + x16[g ^ 2]; y32[g] = y16[g] + y16[g ^ 2]; }
	// (the lanes with g = 0 store)
	return sim_src_finish<FORM>((float)x32[0], p, (float)y32[0], sum_q);
}
inline float span_sim_cell_streamed(const float *a, const float *q, int d, const sim_src &src) {
	const float sum_q = sim_src_abs_sum(q, d);
	switch (sim_src_form(src)) {
	case SIM_SRC_P1: return span_sim_cell_streamed<SIM_SRC_P1>(a, q, d, src.arg, sum_q);
	case SIM_SRC_P2: return span_sim_cell_streamed<SIM_SRC_P2>(a, q, d, src.arg, sum_q);
	case SIM_SRC_PGEN: return span_sim_cell_streamed<SIM_SRC_PGEN>(a, q, d, src.arg, sum_q);
	default: return span_sim_cell_streamed<SIM_SRC_SQRT_COS>(a, q, d, src.arg, sum_q);
	}
}

} // namespace vk_host

#endif
