// vk_score_m7.hip -- vk_score_kernel, MODE 7: the bound pass over the 8-bit shadow (see vk_score.hip.h); the 64-row register
// history of general gaps is in vk_score_m7w.hip.
// A budget of 120 VGPRs (a target the compiler may exceed rather than spill to scratch).  With general gaps (GAP 3) the kernel takes 110 /
// 114 / 118 / 122 VGPRs for queries padded to 4 / 8 / 12 / 16 columns, no AGPRs, and keeps 54 - 58 SGPRs of its gap tables in VGPR lanes
// (counted in those figures).  Up to 12 columns that allocates 112 - 120: three waves per SIMD leave 152 of the 512, room for a wave of
// the exact kernel (136: the rounds' rescoring of this handle and of the peer) beside the bound pass -- the headline's shape, and the only
// one this was measured on.  Without the budget the 12-column form allocated 128 (118 + 4 AGPRs for the MFMA result), three waves left
// 128, and the exact kernel waited for the peer's whole bound pass (1.47 ms in the trace).  13 - 16 query tokens: 122 allocates 128 with
// the budget too, so there the rescoring waits its turn behind the peer's bound pass; results are the same, the overlap is lost.
#define VK_SCORE_VGPRS 120
#include "vk_score.hip.h"

// 257 .. 320 features (five K-steps of 64 int8); alignments over slices of at most 64 tokens only: the gap modes of the main launch
extern "C" hipError_t vk_launch_score_m7w(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream);
extern "C" hipError_t vk_launch_score_m7(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	if (p->nk32 != 5) return hipErrorInvalidValue;
	switch (p->gap_mode) {
	case 0: return launch_score_lt<7, 5, false, 0>(*p, grid, smem_bytes, stream);
	case 1: return launch_score_lt<7, 5, false, 1>(*p, grid, smem_bytes, stream);
	case 3: return launch_score_lt<7, 5, false, 3>(*p, grid, smem_bytes, stream);
	case 6: return vk_launch_score_m7w(p, grid, smem_bytes, stream);
	default: return hipErrorInvalidValue;
	}
}
