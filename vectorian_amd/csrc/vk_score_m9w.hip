// vk_score_m9w.hip -- vk_score_kernel, MODE 9 (see vk_score_m9.hip) with general gaps over slices of 33 .. 64 tokens: the 64-row
// register history, no budget (as vk_score_m8w.hip)
#include "vk_score.hip.h"

extern "C" hipError_t vk_launch_score_m9w(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	return launch_score_lt<9, VK_DEV_FP6_STEPS, false, 6>(*p, grid, smem_bytes, stream);
}
