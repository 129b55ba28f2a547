// vk_score_m10.hip -- vk_score_kernel, MODE 10 (see vk_score.hip.h)
#include "vk_score.hip.h"

extern "C" hipError_t vk_launch_score_m10(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	return launch_score_gap<10, 0, false>(*p, grid, smem_bytes, stream);
}
