// vk_score_m7t.hip -- vk_score_kernel, MODE 7 (the bound pass over the 8-bit shadow, vk_score_m7.hip) with general gaps under a
// slice-gap table that is flat beyond VK_BOUND_TAIL_K entries: GAP 8 (the 32-row history) and GAP 9 (the 64-row history), at five
// and at twelve K-steps.  No budget: the 64-row forms are held by LDS, as in vk_score_m7w.hip.
#include "vk_score.hip.h"

extern "C" int32_t vk_score_m7t_tail_k(void) { return VK_BOUND_TAIL_K; }

template <int NK64>
static hipError_t launch_m7t(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	switch (p->gap_mode) {
	case 8: return launch_score_lt<7, NK64, false, 8>(*p, grid, smem_bytes, stream);
	case 9: return launch_score_lt<7, NK64, false, 9>(*p, grid, smem_bytes, stream);
	default: return hipErrorInvalidValue;
	}
}
extern "C" hipError_t vk_launch_score_m7t(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	if (p->nk32 == 5) return launch_m7t<5>(p, grid, smem_bytes, stream);
	if (p->nk32 == 12) return launch_m7t<12>(p, grid, smem_bytes, stream);
	return hipErrorInvalidValue;
}
