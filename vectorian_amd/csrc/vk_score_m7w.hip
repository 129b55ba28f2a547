// vk_score_m7w.hip -- vk_score_kernel, MODE 7 (see vk_score_m7.hip) with general gaps over slices of 33 .. 64 tokens: the 64-row
// register history takes 192 VGPRs, no budget
#include "vk_score.hip.h"

extern "C" hipError_t vk_launch_score_m7w(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	if (p->nk32 == 12) return launch_score_lt<7, 12, false, 6>(*p, grid, smem_bytes, stream);
	return launch_score_lt<7, 5, false, 6>(*p, grid, smem_bytes, stream);
}
