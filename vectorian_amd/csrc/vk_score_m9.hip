// vk_score_m9.hip -- vk_score_kernel, MODE 9: the bound pass over the compact 6-bit (E2M3) shadow (see vk_score.hip.h);
// the 64-row register history of general gaps is in vk_score_m9w.hip, the flat-tailed forms in vk_score_m9t.hip (and, under local alignment, vk_score_m9f.hip).
// MODE 8's kernels with another load side (load_tile_fp6<., true>, vk_common.hip.h): 3,712-byte tiles, seven loads per tile.  The budget
// is vk_score_m8.hip's: every form here allocates 104 VGPRs without scratch at two tiles per trip (tools/kernel_regs.py
// --bound); tests/test_bound_compact_registers.py holds them to it.
#define VK_SCORE_VGPRS 120
#include "vk_score.hip.h"

extern "C" hipError_t vk_launch_score_m9w(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream);
extern "C" hipError_t vk_launch_score_m9t(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream);
extern "C" hipError_t vk_launch_score_m9(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	if (p->bound_live != 2 || p->tile_bytes != VK_DEV_FP6C_TILE_BYTES) return hipErrorInvalidValue;
	if (p->pos_s) return hipErrorInvalidValue;   // no tag weights under a bound (vk_score.hip.h, TAGS)
	switch (p->gap_mode) {
	case 0: return launch_score_lt<9, VK_DEV_FP6_STEPS, false, 0>(*p, grid, smem_bytes, stream);
	case 1: return launch_score_lt<9, VK_DEV_FP6_STEPS, false, 1>(*p, grid, smem_bytes, stream);
	case 3: return launch_score_lt<9, VK_DEV_FP6_STEPS, false, 3>(*p, grid, smem_bytes, stream);
	case 6: return vk_launch_score_m9w(p, grid, smem_bytes, stream);
	case 8: case 9: return vk_launch_score_m9t(p, grid, smem_bytes, stream);
	default: return hipErrorInvalidValue;
	}
}
