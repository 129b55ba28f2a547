// vk_score_m9f.hip -- vk_score_local_kernel: vk_score_kernel<9, ., false, 8, LT> (the flat-tailed bound pass over the compact 6-bit
// shadow, vk_score_m9t.hip) for local alignment and a query of exactly LQ tokens, LT = 4 * ceil(LQ / 4).  The body is
// vk_score_kernel's (vk_score_body.hip.inc); at the DP a group of four slices of exactly 32 tokens takes the straight-line form
// dp_tail_local_full, every other group dp_general_tail_reg with the locality and the column count at compile time.  Both are
// bit-identical to the form vk_score_kernel calls, so the bounds are the same floats whichever kernel ran.
// The budget is vk_score_m9t.hip's; tests/test_bound_fast_dp_registers.py holds every form to an allocation of 104 without scratch
// and the instantiations to the set the launcher below dispatches to.
#define VK_SCORE_VGPRS 104
#include <cstring>
#include "vk_score.hip.h"

template <int LT, int LQ>
__global__ __launch_bounds__(256) VK_SCORE_KERNEL_ATTR void vk_score_local_kernel(VkScoreParams p) {
	static_assert(LT == (LQ + 3) / 4 * 4, "the strip is as wide as vk_score_kernel's for a query of LQ tokens");
	constexpr int MODE = 9, NK32 = VK_DEV_FP6_STEPS, GAP = 8, FULL_LQ = LQ;
	constexpr bool TAIL = false;
#include "vk_score_body.hip.inc"
}

// 1: vk_launch_score_m9t hands this launch to vk_launch_score_m9f.  VK_BOUND_DP=generic keeps vk_score_kernel (read per launch, as
// VK_BLOCKS_PER_CU is); the host asks the same question to report which kernel ran (vk_bound_pass_dp)
extern "C" int32_t vk_score_m9f_takes(const VkScoreParams *p) {
	if (p->gap_mode != 8 || p->locality != VK_DEV_LOCAL || p->len_t < 1 || p->len_t > 16) return 0;
	const char *dp = getenv("VK_BOUND_DP");
	return dp && strcmp(dp, "generic") == 0 ? 0 : 1;
}

// the same grid and LDS as launch_score_lt<9, ., false, 8> gives vk_score_kernel, at three workgroups per CU where that kernel takes four:
// with a third fewer VALU instructions a fourth wave per SIMD buys the pass nothing and takes the room the rounds' exact kernel of the
// query in flight beside it runs in (1 M x 32 tokens, 10-token query: DESIGN 11.12, profiles/bound_fast_dp_ab.json)
#define VK_M9F_BLOCKS_PER_CU 3
extern "C" hipError_t vk_launch_score_m9f(const VkScoreParams *p, int32_t grid, size_t smem_bytes, hipStream_t stream) {
	if (!vk_score_m9f_takes(p)) return hipErrorInvalidValue;
	switch (p->len_t) {
#define VK_M9F_CASE(LQ) case LQ: return launch_sized(vk_score_local_kernel<(LQ + 3) / 4 * 4, LQ>, *p, grid, smem_bytes, stream, VK_M9F_BLOCKS_PER_CU);
	VK_M9F_CASE(1) VK_M9F_CASE(2) VK_M9F_CASE(3) VK_M9F_CASE(4) VK_M9F_CASE(5) VK_M9F_CASE(6) VK_M9F_CASE(7) VK_M9F_CASE(8)
	VK_M9F_CASE(9) VK_M9F_CASE(10) VK_M9F_CASE(11) VK_M9F_CASE(12) VK_M9F_CASE(13) VK_M9F_CASE(14) VK_M9F_CASE(15) VK_M9F_CASE(16)
#undef VK_M9F_CASE
	default: return hipErrorInvalidValue;
	}
}
