// vk_score_m8t.hip -- vk_score_kernel, MODE 8 (the bound pass over the 6-bit shadow, vk_score_m8.hip) with general gaps under a
// slice-gap table that is flat beyond VK_BOUND_TAIL_K entries: GAP 8 (the 32-row history) and GAP 9 (the 64-row history), DESIGN 11.10.
// The history is K + 1 live rows and a running maximum, the table K + 2 scalars.  The budget is vk_score_m8.hip's (a target, not a
// limit); tests/test_bound_tail_registers.py holds the 32-row forms to an allocation of 104 and the 64-row forms to 120, no scratch.
#define VK_SCORE_VGPRS 104
#include "vk_score.hip.h"

extern "C" int32_t vk_score_m8t_tail_k(void) { return VK_BOUND_TAIL_K; }

extern "C" hipError_t vk_launch_score_m8t(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	switch (p->gap_mode) {
	case 8: return launch_score_lt<8, VK_DEV_FP6_STEPS, false, 8>(*p, grid, smem_bytes, stream);
	case 9: return launch_score_lt<8, VK_DEV_FP6_STEPS, false, 9>(*p, grid, smem_bytes, stream);
	default: return hipErrorInvalidValue;
	}
}
