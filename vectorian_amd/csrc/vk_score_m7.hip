// vk_score_m7.hip -- vk_score_kernel, MODE 7: the bound pass over the 8-bit shadow (see vk_score.hip.h); the 64-row register
// history of general gaps is in vk_score_m7w.hip.
// A budget of 120 VGPRs (a target the compiler may exceed rather than spill to scratch).  It was set when the general-gap forms took 110 /
// 114 / 118 / 122 VGPRs for queries padded to 4 / 8 / 12 / 16 columns: 44 of those were loop invariants of the DP that the compiler
// kept for the kernel's lifetime (dp_general_reg makes them per group now), and eight were the tag modifier's, which a
// bound pass never has.  Today the forms take 66 / 70 / 74 / 81 (five K-steps) and 69 / 70 / 74 / 79 (twelve), allocate 72 - 88 and keep
// five waves per SIMD or more; three workgroups per CU (launch_sized) leave more than half of the registers to the rounds' exact kernel,
// whose rescoring form allocates 96 at 300-d.  The gap tables still spill 50 - 60 SGPRs into VGPR lanes (counted in those figures).
// DESIGN 11.9 has the whole table; nothing but the headline's shape was timed.
#define VK_SCORE_VGPRS 120
#include "vk_score.hip.h"

// 289 .. 304 features (five K-steps of 64 int8) and 753 .. 768 (twelve, two batches of six in flight: dot_tile_i8); alignments over
// slices of at most 64 tokens only: the gap modes of the main launch
extern "C" hipError_t vk_launch_score_m7w(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream);
extern "C" hipError_t vk_launch_score_m7t(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream);   // the flat-tailed forms (vk_score_m7t.hip)
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
	if (p->pos_s) return hipErrorInvalidValue;   // no tag weights under a bound (vk_score.hip.h, TAGS)
	if (p->gap_mode == 8 || p->gap_mode == 9) return vk_launch_score_m7t(p, grid, smem_bytes, stream);
	if (p->nk32 == 5) return launch_m7<5>(p, grid, smem_bytes, stream);
	if (p->nk32 == 12) return launch_m7<12>(p, grid, smem_bytes, stream);
	return hipErrorInvalidValue;
}
