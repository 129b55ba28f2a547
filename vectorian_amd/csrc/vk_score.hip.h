// vk_score.hip.h -- the fused scoring kernel and its launcher templates.  The instantiations are spread over
// vk_score_m0..m3.hip (one per similarity MODE) so that they compile in parallel.
#ifndef VK_SCORE_HIP_H
#define VK_SCORE_HIP_H

#include <type_traits>
#include "vk_common.hip.h"

// ---------------------------------------------------------------------------
// the fused scoring kernel: one wave = 4 sentences at a time, grid-stride over groups.
//   MODE 0: contextual layout, NK32 K-steps (last one half filled when TAIL), query fragments in registers
//   MODE 1: contextual layout, bf16 rows of any d (runtime K loop)
//   MODE 2: static layout: gather rows of the per-query table by token id
//   MODE 3: contextual layout, NK32 K-steps, query tile staged in LDS (large d)
//   MODE 4: contextual layout, fp32 tiles of NK32 blocks of 16 features (compile time), query tile staged in LDS
//   MODE 5: MODE 1 for bf16 rows of 256 features and more: eight K-steps in flight instead of four
//   MODE 6: MODE 1 for fp32 rows (any d but the 300 of MODE 4)
//   MODE 7: the 8-bit shadow of a contextual bf16 corpus, NK32 K-steps of 64 int8 (here NK32 counts those): every cell an upper bound of
//           the cosine MODE 0 / 3 compute, so the score is an upper bound of theirs (the bound pass)
//   MODE 8: the 6-bit (E2M3) shadow, three K-steps of 128 features (NK32 = 3): as MODE 7, the product on the scaled fp6 MFMA
//   MODE 9: MODE 8 over the compact 6-bit shadow (3,712-byte tiles): the tile's loads differ, nothing else does
//   MODE 10 / 11 / 12: MODE 1 / 5 / 6 of a contextual handle under an operator chain (vk_corpus_set_contextual_sim_ops): a
//           cell is vk_host::contextual_cell -- the chain on the unclipped cosine, zeros on the columns past the query, the clip.  Every
//           width takes these (the 300-d and 768-d forms of MODE 0 / 3 / 4 know the clipped cosine only)
// GAP: 0 linear, 1 affine, 2 general (LDS history, serial in-row chain),
//      3 general, sentences <= 32 tokens, strictly subadditive w_t (register history),
//      4 relaxed word mover's distance (no DP: row / column minima of 1 - S),
//      5 word rotator's distance, upper bound of the score (stage 1),
//      6 as 3 for sentences <= 64 tokens,
//      7 relaxed word mover's distance, 1:n form (greedy fill by ascending distance),
//      8 as 3 under a slice-gap table that is flat beyond VK_BOUND_TAIL_K entries (dp_general_tail_reg): an upper bound of 3,
//        the bound pass only (MODE 7 / 8),
//      9 as 6, likewise.
// LT: padded query length (4, 8, 12, 16).
// ---------------------------------------------------------------------------

// VK_SCORE_VGPRS (vk_score_m7.hip, vk_score_m8.hip): a register budget for every kernel of the unit
#ifdef VK_SCORE_VGPRS
#define VK_SCORE_KERNEL_ATTR __attribute__((amdgpu_num_vgpr(VK_SCORE_VGPRS)))
#else
#define VK_SCORE_KERNEL_ATTR
#endif

// the body is text shared with vk_score_local_kernel (vk_score_m9f.hip): see vk_score_body.hip.inc for why it is no device function
template <int MODE, int NK32, bool TAIL, int GAP, int LT>
__global__ __launch_bounds__(256) VK_SCORE_KERNEL_ATTR void vk_score_kernel(VkScoreParams p) {
	constexpr int FULL_LQ = 0;
#include "vk_score_body.hip.inc"
}

// grid = every CU filled to the kernel's real residency (VGPR / LDS bound), not more: the waves
// walk the groups with a grid stride, so a second, partially filled round of workgroups would only
// add a tail.  VK_BLOCKS_PER_CU overrides (experiments).  residency > 0: workgroups per CU measured for that kernel, in place of the
// rules below (vk_score_m9f.hip).
template <typename K>
static hipError_t launch_sized(K kernel, const VkScoreParams &p, int want_blocks, size_t smem, hipStream_t stream, int residency = 0) {
	int occ = 0;
	const int threads = p.group_list ? 64 : 256;
	hipError_t e;
	if (smem > 64 * 1024) {
		e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
		if (e != hipSuccess) return e;
	}
	e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, smem);
	if (e != hipSuccess) return e;
	if (occ < 1) occ = 1;
	const int real_occ = occ;
	// measured on MI355X (1M x 32 x 300-d): 3 workgroups (12 waves) per CU stream HBM fastest --
	// 2.90 ms vs 3.51 ms at 5 per CU for the linear-gap kernel, 2.95 ms at 4; more concurrent streams cost bandwidth
	// the transport bound (WRD / full WMD stage 1) has the longest epilogue per group and wants every wave it can get to
	// hide it: 1 M x 32 x 300-d 3.54 ms at 3 per CU, 3.08 at 4; 768-d 4.31 ms at 1, 3.37 at 2
	const bool bound_pass = p.gap_mode == 5 || (p.gap_mode == 4 && p.wmd_bound == 1);
	// narrow rows (d <= 96) are not a stream either: a slice is 6 KB or less and the DP dominates -- 64-d, 32 tokens: 3.4 TB/s at
	// 3 per CU, 4.8 TB/s at 5; 96-d: 3.7 against 5.4 TB/s.  129..224-d: 4 per CU stream 4-8 % faster than 3 (6.4 against
	// 6.0 TB/s); 128-d and 256..1536-d: 3 per CU within 2 % of the best setting (tools/sweep_dims.py, profiles/r02_sweep_dims*.jsonl)
	const bool dp_bound = p.layout == VK_DEV_LAYOUT_STATIC || (p.nk32 <= 3 && p.bound_bits == 0);
	// the 8-bit shadow (MODE 7, 328-byte rows; 1 M x 32 tokens, general gaps): 1.58 - 1.61 ms at 3 per CU, 1.60 - 1.65 at 4, 1.70 at 5, 1.80 at 2 --
	// and three waves per SIMD of its 120 VGPRs leave room for the rounds' exact kernel beside it (vk_score_m7.hip)
	// the 6-bit shadow (MODE 8, 3,968-byte tiles, the same shape; two tiles per trip, 104 VGPRs, four waves per SIMD at the most):
	// ms_per_step 1.59 at 2 per CU, 1.44 at 3, 1.40 at 4 on a machine where the kernel before it (118 VGPRs, one tile per trip)
	// took 1.47 at 3, 1.53 - 1.56 at 4 and 1.53 at 5 -- at 4 that kernel alone was faster (1.35 ms) and the step slower, the
	// rounds waiting for the peer's pass; this one keeps ms_per_step within 0.02 ms of kernel_ms at 4
	// its flat-tailed form (GAP 8, the same 104 VGPRs): ms_per_step 1.275 - 1.287 at 3 per CU, 1.270 - 1.271 at 4
	// the 12-step shadow (768-d rows, 1 M slices of 8 .. 64 tokens, 64-row history): LDS and registers admit two per CU -- 4.40 ms; one: 5.98 ms
	const int stream_cap = ((p.bound_bits == 0 && p.nk32 >= 5 && p.nk32 <= 7) || p.bound_bits == 6) ? 4 : 3;
	if (occ > stream_cap && !dp_bound && !bound_pass) occ = stream_cap;   // the static layout is DP-bound, not a stream: keep full residency
	// 768-d rows: a wave already keeps 24 KiB of loads in flight per tile; one workgroup per CU measured fastest
	// (ragged 8..64 tokens, 400 k sentences: 3.37 ms at 1, 3.45 ms at 2 per CU)
	// -- the 768-d specialisation only: the generic kernel at 1024-d loses 20 % (32 tokens) to 38 % (ragged) with one group
	// per CU (tools/sweep_dims.py)
	// (nor under an operator chain, which runs 768-d rows on the generic form: MODE 11)
	if (p.nk32 == 24 && p.tail == 0 && p.prec == 0 && p.layout != VK_DEV_LAYOUT_STATIC && !bound_pass && p.sim_ops.n == 0) occ = 1;
	if (residency > 0) occ = residency < real_occ ? residency : real_occ;
	const char *ov = getenv("VK_BLOCKS_PER_CU");   // read per launch: tools/sweep_dims.py varies it inside one process
	if (ov && atoi(ov) > 0) occ = atoi(ov) < real_occ ? atoi(ov) : real_occ;
	int dev = 0, cus = 256;
	if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
	const int grid = want_blocks < cus * occ ? want_blocks : cus * occ;
	kernel<<<grid, threads, smem, stream>>>(p);
	return hipGetLastError();
}

template <int MODE, int NK32, bool TAIL, int GAP>
static hipError_t launch_score_lt(const VkScoreParams &p, int grid, size_t smem, hipStream_t stream) {
	const int lt = p.len_t <= 4 ? 4 : p.len_t <= 8 ? 8 : p.len_t <= 12 ? 12 : 16;
	switch (lt) {
	case 4: return launch_sized(vk_score_kernel<MODE, NK32, TAIL, GAP, 4>, p, grid, smem, stream);
	case 8: return launch_sized(vk_score_kernel<MODE, NK32, TAIL, GAP, 8>, p, grid, smem, stream);
	case 12: return launch_sized(vk_score_kernel<MODE, NK32, TAIL, GAP, 12>, p, grid, smem, stream);
	default: return launch_sized(vk_score_kernel<MODE, NK32, TAIL, GAP, 16>, p, grid, smem, stream);
	}
}

template <int MODE, int NK32, bool TAIL>
static hipError_t launch_score_gap(const VkScoreParams &p, int grid, size_t smem, hipStream_t stream) {
	switch (p.gap_mode) {
	case 0: return launch_score_lt<MODE, NK32, TAIL, 0>(p, grid, smem, stream);
	case 1: return launch_score_lt<MODE, NK32, TAIL, 1>(p, grid, smem, stream);
	case 3: return launch_score_lt<MODE, NK32, TAIL, 3>(p, grid, smem, stream);
	case 4: return launch_score_lt<MODE, NK32, TAIL, 4>(p, grid, smem, stream);
	case 5: return launch_score_lt<MODE, NK32, TAIL, 5>(p, grid, smem, stream);
	case 6: return launch_score_lt<MODE, NK32, TAIL, 6>(p, grid, smem, stream);
	case 7: return launch_score_lt<MODE, NK32, TAIL, 7>(p, grid, smem, stream);
	default: return launch_score_lt<MODE, NK32, TAIL, 2>(p, grid, smem, stream);
	}
}

#endif
