// vk_score_m7.hip -- vk_score_kernel, MODE 7: the bound pass over the 8-bit shadow (see vk_score.hip.h); the 64-row register
// history of general gaps is in vk_score_m7w.hip.
// A budget of 120 VGPRs (a target the compiler may exceed rather than spill to scratch).  With general gaps (GAP 3) the kernel takes 110 /
// 114 / 118 / 122 VGPRs for queries padded to 4 / 8 / 12 / 16 columns, no AGPRs, and keeps 54 - 58 SGPRs of its gap tables in VGPR lanes
// (counted in those figures).  Up to 12 columns that allocates 112 - 120: three waves per SIMD leave 152 of the 512, room for a wave of
// the exact kernel (136: the rounds' rescoring of this handle and of the peer) beside the bound pass -- the headline's shape, and the only
// one this was measured on.  Without the budget the 12-column form allocated 128 (118 + 4 AGPRs for the MFMA result), three waves left
// 128, and the exact kernel waited for the peer's whole bound pass (1.47 ms in the trace).  13 - 16 query tokens: 122 allocates 128 with
// the budget too, so there the rescoring waits its turn behind the peer's bound pass; results are the same, the overlap is lost.
// The twelve-step form (768-d rows) takes 117 / 121 / 125 / 125 under the same budget: from 8 columns on it allocates 128 like the
// 16-column form above (DESIGN 11.3 has the whole table).
#define VK_SCORE_VGPRS 120
#include "vk_score.hip.h"

// 289 .. 304 features (five K-steps of 64 int8) and 753 .. 768 (twelve, two batches of six in flight: dot_tile_i8); alignments over
// slices of at most 64 tokens only: the gap modes of the main launch
extern "C" hipError_t vk_launch_score_m7w(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream);
template <int NK64>
static hipError_t launch_m7(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	switch (p->gap_mode) {
	case 0: return launch_score_lt<7, NK64, false, 0>(*p, grid, smem_bytes, stream);
	case 1: return launch_score_lt<7, NK64, false, 1>(*p, grid, smem_bytes, stream);
	case 3: return launch_score_lt<7, NK64, false, 3>(*p, grid, smem_bytes, stream);
	case 6: return vk_launch_score_m7w(p, grid, smem_bytes, stream);
	default: return hipErrorInvalidValue;
	}
}
extern "C" hipError_t vk_launch_score_m7(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	if (p->bound_live < 1 || p->bound_live > 4) return hipErrorInvalidValue;
	if (p->nk32 == 5) return launch_m7<5>(p, grid, smem_bytes, stream);
	if (p->nk32 == 12) return launch_m7<12>(p, grid, smem_bytes, stream);
	return hipErrorInvalidValue;
}
