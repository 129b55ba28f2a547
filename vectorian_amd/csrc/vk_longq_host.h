// vk_longq_host.h -- the geometry of vk_longq_kernel (queries of 65 .. VK_MAX_LONG_QUERY_LEN tokens): strides, the carve-up
// of a workgroup's LDS and of its scratch region, the grid -- for both forms of the kernel, the one over slices of at most 64 tokens
// and the block form over slices of up to VK_MAX_SENT_LEN (512) tokens.  vk_longq.hip sizes its launches from it, vk_longq_host.cpp its
// buffers; nothing else computes these numbers.  Host only, no HIP types: tests/test_longq_geometry_host.py compiles it with g++ and
// enumerates every shape (CPU tier).
#ifndef VK_LONGQ_HOST_H
#define VK_LONGQ_HOST_H

#include <cstddef>
#include <cstdint>

namespace vk_host {

constexpr size_t kLongqLdsLimit = 160 * 1024;   // the LDS of a CU: no launch may ask for more
constexpr size_t kLongqCanonLds = 8 * 1024;     // VK_CANON_LDS (vk_common.hip.h; vk_longq.hip asserts that they agree): staging of sim_canon16
constexpr int kLongqFlowGrid = 256;             // workgroups of a traceback launch of the block form (their scratch regions are MBs)

// the strip's row: the longest slice of the pass rounded up to 16 columns (a 32-token corpus takes half the LDS of a 64-token one:
// twice the waves per CU)
inline int longq_stride(int max_len) { const int w = (max_len + 15) / 16 * 16; return w < 16 ? 16 : w > 64 ? 64 : w; }

// One launch of vk_longq_kernel.  max_len: the longest slice the launch meets -- at most 64: the form with one sweep per slice, beyond:
// the block form (column blocks of 64 slice tokens behind a border column).
struct longq_geometry {
	bool blocks = false;
	int lt_pad = 0;         // the query's tokens rounded up to 16 (rows of the strip)
	int s_stride = 0;       // floats per row of the strip
	int ls_pad = 64;        // columns per row of the matrix / records / similarities in the scratch region (block form: the longest slice rounded up to 64)
	// LDS: [canon][strip][border columns][matrix (general gaps, scoring pass, where it fits)]
	size_t canon_off = 0, canon_bytes = 0, strip_off = 0, strip_bytes = 0, col_off = 0, col_bytes = 0, hm_lds_off = 0, hm_lds_bytes = 0;
	bool hm_in_lds = false; // general gaps, scoring pass: the matrix sits behind the strip and the border columns, the launch takes no scratch
	size_t lds_bytes = 0;   // canon + strip + border columns (+ 64)
	size_t launch_lds_bytes = 0;   // the launch's dynamic LDS: lds_bytes and the matrix where it is in LDS
	// the scratch region of a workgroup: [matrix H (general gaps)][records (tracebacks)][unmodified similarities (tracebacks)]
	size_t hm_off = 0, hm_bytes = 0, dm_off = 0, dm_bytes = 0, su_off = 0, su_bytes = 0;
	size_t scratch_bytes = 0;   // the three parts rounded up to 256 bytes, and 256 to spare
};

// general gaps, scoring pass over slices of at most 64 tokens: does the matrix fit the LDS behind the strip (leaving room for at least
// two workgroups per CU)?
inline bool longq_hm_in_lds(int len_t, int max_len) {
	const size_t strip = (size_t)((len_t + 15) / 16 * 16) * longq_stride(max_len) * 4 + 64;
	return strip + (size_t)(len_t + 1) * longq_stride(max_len) * 4 <= 78 * 1024;
}

inline longq_geometry longq_geometry_of(int len_t, int max_len, int gap_mode, bool flow, bool tagged) {
	longq_geometry g;
	const bool general = gap_mode == 2;
	g.blocks = max_len > 64;
	g.lt_pad = (len_t + 15) / 16 * 16;
	g.s_stride = longq_stride(max_len);
	g.ls_pad = g.blocks ? (max_len + 63) / 64 * 64 : 64;
	g.canon_bytes = flow ? kLongqCanonLds : 0;
	g.strip_off = g.canon_bytes;
	g.strip_bytes = (size_t)g.lt_pad * g.s_stride * 4;
	g.col_off = g.strip_off + g.strip_bytes;
	// two border columns in turn, H[64 b][0 .. len_t] each, E[64 b][.] behind it under affine gaps
	g.col_bytes = g.blocks ? 2 * (size_t)(gap_mode == 1 ? 2 : 1) * (size_t)(len_t + 1) * 4 : 0;
	g.hm_lds_off = g.col_off + g.col_bytes;
	g.hm_in_lds = general && !flow && !g.blocks && longq_hm_in_lds(len_t, max_len);
	g.hm_lds_bytes = g.hm_in_lds ? (size_t)(len_t + 1) * g.s_stride * 4 : 0;
	g.lds_bytes = g.hm_lds_off + 64;
	g.launch_lds_bytes = g.lds_bytes + g.hm_lds_bytes;
	g.hm_bytes = general ? (size_t)(len_t + 1) * g.ls_pad * 4 : 0;                         // H[v][slice token] (where it is not in LDS)
	g.dm_bytes = flow ? (size_t)(len_t + 1) * g.ls_pad * 2 : 0;                            // direction | flags | gap length per cell
	// unmodified similarities (reported per edge): under tag weights; the block form always (the strips of earlier blocks are gone
	// when the walk back crosses into them)
	g.su_bytes = (flow && (tagged || g.blocks)) ? (size_t)g.lt_pad * g.ls_pad * 4 : 0;
	g.dm_off = g.hm_off + g.hm_bytes;
	g.su_off = g.dm_off + g.dm_bytes;
	g.scratch_bytes = (g.hm_bytes + g.dm_bytes + g.su_bytes + 255) / 256 * 256 + 256;
	return g;
}

// workgroups (one wave each) of a scoring pass: as many as `cus` CUs hold with this much LDS each, at most one per item
inline int longq_grid(int cus, size_t lds_bytes, int64_t n_items) {
	int per_cu = (int)(kLongqLdsLimit / ((lds_bytes + 511) / 512 * 512 + 512));
	if (per_cu < 1) per_cu = 1;
	if (per_cu > 16) per_cu = 16;
	const int64_t want = (int64_t)cus * per_cu;
	return (int)(n_items < want ? (n_items < 1 ? 1 : n_items) : want);
}
// ... of a traceback launch: one per winner; the block form caps them (the kernel loops over its items)
inline int longq_flow_grid(bool blocks, int n_winners) {
	const int n = n_winners < 1 ? 1 : n_winners;
	return blocks && n > kLongqFlowGrid ? kLongqFlowGrid : n;
}

} // namespace vk_host

#endif
