// vk_longq.hip.h -- what the two units of the long queries share (vk_longq.hip: slices of at most 64 tokens; vk_longq_blocks.hip: the
// block form, slices of up to 512 tokens): the lane shift of the sweep, the 300-d tile product of the fill, the codes of a cell's
// record, the device's CU count for the grids.  Strides, LDS and scratch carve-up, grids: vk_longq_host.h (host only).
#ifndef VK_LONGQ_HIP_H
#define VK_LONGQ_HIP_H

#include "vk_common.hip.h"
#include "vk_longq_host.h"

static_assert(vk_host::kLongqCanonLds == VK_CANON_LDS, "vk_longq_host.h restates VK_CANON_LDS");

// value of lane - 1 (lane 0: `border`): one DPP move across the wave (wave_shr:1; the first version shifted through ds_bpermute, an LDS
// round trip per step and register, and twice per step)
__device__ __forceinline__ float lane_up(float x, float border) {
	return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, border), __builtin_bit_cast(int, x), 0x138, 0xf, 0xf, false));
}

// 300-d bf16 rows: the slice's token tiles (up to three at a time) stay in registers as A fragments while the query's tiles stream
// past them -- each query tile is fetched from L2 once per slice (the second and third use hit the L1) instead of once per token
// tile, and the token tiles once instead of once per query tile: 407 -> 97 KB of L2 traffic per 32-token slice and 100-token query,
// which is what the first form of this pass was bound by (39 -> ms per million slices).  Plain loads for the query
// tile (it is re-read by every wave), same MFMA sequence as sim_tile.
template <int NK, bool HALF>
__device__ __forceinline__ f32x4 longq_sim_tile(const QFrag<NK, HALF> &f, const uint8_t *__restrict__ qtile, int lane) {
	bf16x8 x[NK];
#pragma unroll
	for (int t = 0; t < NK; t++) {
		if (HALF && t == NK - 1) x[t] = load_half_block(qtile + t * 1024, lane, false);
		else x[t] = *reinterpret_cast<const bf16x8 *>(qtile + t * 1024 + lane * 16);
	}
	f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
	for (int t = 0; t < NK; t++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.q[t], x[t], acc, 0, 0, 0);
	acc[0] = clip01(acc[0]); acc[1] = clip01(acc[1]); acc[2] = clip01(acc[2]); acc[3] = clip01(acc[3]);
	return acc;
}

enum { LQ_STOP = 0, LQ_DIAG = 1, LQ_UP = 2, LQ_LEFT = 3 };   // D_* of the oracle; bits 0-1 of a cell's record, bit 2: E extended, bit 3: F extended, bits 4..: gap length

static inline int longq_device_cus() {
	int dev = 0, cus = 256;
	if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
	return cus;
}

#endif
