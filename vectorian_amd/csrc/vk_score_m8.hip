// vk_score_m8.hip -- vk_score_kernel, MODE 8: the bound pass over the 6-bit (E2M3) shadow (see vk_score.hip.h); the 64-row
// register history of general gaps is in vk_score_m8w.hip.
// The budget of vk_score_m7.hip (a target, not a limit: the compiler exceeds it rather than spill).  With no loop invariant of the DP
// left in the kernel's lifetime every form here allocates 104 VGPRs without scratch at two tiles per trip (2 x 18 tile registers: three
// K-steps of 4 + 2 each), four waves per SIMD; a wave of the rounds' exact kernel allocates 104 (it was 144).  The figures by gap
// mode and query width are in DESIGN 11.9 (tools/kernel_regs.py); tests/test_bound_kernel_registers.py holds them to 120.
#define VK_SCORE_VGPRS 120
#include "vk_score.hip.h"

// 289 .. 304 features (three K-steps of 128 E2M3 codes, the last with bound_live of its four quarters); alignments over slices of at
// most 64 tokens only: the gap modes of the main launch
extern "C" hipError_t vk_launch_score_m8w(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream);
extern "C" hipError_t vk_launch_score_m8t(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream);   // the flat-tailed forms (vk_score_m8t.hip)
extern "C" hipError_t vk_launch_score_m8(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	if (p->bound_live < 1 || p->bound_live > 4 || p->tile_bytes != VK_DEV_FP6_TILE_BYTES(p->bound_live)) return hipErrorInvalidValue;
	if (p->pos_s) return hipErrorInvalidValue;   // no tag weights under a bound (vk_score.hip.h, TAGS)
	switch (p->gap_mode) {
	case 0: return launch_score_lt<8, VK_DEV_FP6_STEPS, false, 0>(*p, grid, smem_bytes, stream);
	case 1: return launch_score_lt<8, VK_DEV_FP6_STEPS, false, 1>(*p, grid, smem_bytes, stream);
	case 3: return launch_score_lt<8, VK_DEV_FP6_STEPS, false, 3>(*p, grid, smem_bytes, stream);
	case 6: return vk_launch_score_m8w(p, grid, smem_bytes, stream);
	case 8: case 9: return vk_launch_score_m8t(p, grid, smem_bytes, stream);
	default: return hipErrorInvalidValue;
	}
}
