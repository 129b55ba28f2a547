// vk_score_m9t.hip -- vk_score_kernel, MODE 9 (the bound pass over the compact 6-bit shadow, vk_score_m9.hip) with general gaps under a
// slice-gap table that is flat beyond VK_BOUND_TAIL_K entries: GAP 8 (the 32-row history) and GAP 9 (the 64-row history), as
// vk_score_m8t.hip -- the same K (the host asks vk_score_m8t_tail_k for either layout) and the same budget;
// tests/test_bound_compact_registers.py holds the 32-row forms to an allocation of 104 and the 64-row forms to 120, no scratch.
#define VK_SCORE_VGPRS 104
#include "vk_score.hip.h"

// GAP 8 under local alignment for a query of 1 .. 16 tokens has a kernel of its own (vk_score_m9f.hip) unless
// VK_BOUND_DP=generic; everything else -- global and semiglobal, GAP 9 -- keeps vk_score_kernel
extern "C" hipError_t vk_launch_score_m9t(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	if (vk_score_m9f_takes(p)) return vk_launch_score_m9f(p, grid, smem_bytes, stream);
	switch (p->gap_mode) {
	case 8: return launch_score_lt<9, VK_DEV_FP6_STEPS, false, 8>(*p, grid, smem_bytes, stream);
	case 9: return launch_score_lt<9, VK_DEV_FP6_STEPS, false, 9>(*p, grid, smem_bytes, stream);
	default: return hipErrorInvalidValue;
	}
}
