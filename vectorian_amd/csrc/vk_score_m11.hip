// vk_score_m11.hip -- vk_score_kernel, MODE 11 (see vk_score.hip.h)
#include "vk_score.hip.h"

extern "C" hipError_t vk_launch_score_m11(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	return launch_score_gap<11, 0, false>(*p, grid, smem_bytes, stream);
}
