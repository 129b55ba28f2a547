// vk_sim_ops_host.h -- the operator chain of a ModifiedVectorSim over the cosine (vectorian/sim/vector.py:179-200,
// vectorian/sim/kernel.py:14-76), one definition for the host and the device.  The reference runs the operators as numpy calls on the
// float32 similarity matrix, in place, one after the other; apply() is that chain for one cell: fp32 throughout, one rounding per numpy
// operation, nothing contracted into a fused multiply-add.  The device compiles it into the two table kernels of the static layout
// (vk_pack.hip, vk_rwmd_batch.hip) and into the canonical restatement of the winners' cells (static_cell, vk_common.hip.h); the host
// side validates a chain (vk_corpus_set_sim_ops).  No HIP types: tests/test_sim_ops_host.py compiles it with g++ under AddressSanitizer
// and UBSan and holds every operator against vectorian_amd/kernel.py in numpy float32, bit for bit (CPU tier).
#ifndef VK_SIM_OPS_HOST_H
#define VK_SIM_OPS_HOST_H

#include "../../include/vectorian_hip.h"

#include <cmath>
#include <cstdint>

#ifndef VK_HOST_DEVICE
#ifdef __HIPCC__
#define VK_HOST_DEVICE __host__ __device__
#define VK_UNROLL _Pragma("unroll")
#else
#define VK_HOST_DEVICE
#define VK_UNROLL
#endif
#endif

namespace vk_host {

// the chain of a handle: n operators, applied in order (n = 0: the plain cosine).  A kernel argument by value: the loop is wave-uniform
struct sim_ops {
	int32_t n;
	int32_t kind[VK_MAX_SIM_OPS];
	float arg[VK_MAX_SIM_OPS];
};

// VK_OK, or why vk_corpus_set_sim_ops refuses the chain (*bad: the offending operator, -1: the count)
inline int sim_ops_check(const int32_t *kinds, const float *args, int32_t n_ops, int *bad) {
	*bad = -1;
	if (n_ops < 0 || n_ops > VK_MAX_SIM_OPS) return VK_ERR_INVALID;
	for (int i = 0; i < n_ops; i++) {
		*bad = i;
		if (kinds[i] < VK_SIMOP_BIAS || kinds[i] > VK_SIMOP_RADIAL_BASIS) return VK_ERR_INVALID;
		if (!std::isfinite(args[i])) return VK_ERR_INVALID;
	}
	*bad = -1;
	return VK_OK;
}

VK_HOST_DEVICE inline float sim_ops_apply(float x, const sim_ops &ops) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	for (int i = 0; i < ops.n; i++) {
		const float a = ops.arg[i];
		switch (ops.kind[i]) {
		case VK_SIMOP_BIAS: x = x + a; break;                                  // data += bias (kernel.py:37-38)
		case VK_SIMOP_SCALE: x = x * a; break;                                 // data *= scale (:48-49)
		case VK_SIMOP_THRESHOLD: {                                             // x = maximum(0, data - t); x[x > 0] += t (:70-73)
			const float y = fmaxf(0.0f, x - a);
			x = y > 0.0f ? y + a : 0.0f;
		} break;
		case VK_SIMOP_ONE_MINUS: x = fmaxf(0.0f, 1.0f - x); break;             // maximum(0, 1 - data) (:26-27)
		case VK_SIMOP_POWER: x = powf(fmaxf(x, 0.0f), a); break;               // power(maximum(data, 0), exp) (:59-60)
		case VK_SIMOP_RADIAL_BASIS: {                                          // exp(-gamma * power(data, 2)) (:18-19): numpy squares by x * x
			const float sq = x * x;
			x = expf((-a) * sq);
		} break;
		default: break;
		}
	}
	return x;
}

// One similarity cell of a VK_LAYOUT_CONTEXTUAL handle (vk_corpus_set_contextual_sim_ops; metric/contextual.cpp:40-56: the VectorSim
// on the token vectors, then the clip): clip01(chain(cosine)) on the columns the query holds, 0 on the padding behind them -- the
// chain of a zero cosine is no zero ((x + 1) / 2: 0.5), and the DPs' and the relaxed transports' maxima count on zeros there.  No
// sim[id(t_j)][j] = 1 rewrite: that is metric/static.cpp's alone.  n = 0: the clipped cosine, bit for bit, whatever in_query says.
// The scoring epilogues (vk_score_body.hip.inc, vk_score32.hip), the restatement of the winners' cells and
// tests/test_contextual_cell_host.py all state the cell through this function.
VK_HOST_DEVICE inline float contextual_cell(float cosine, bool in_query, const sim_ops &ops) {
	if (ops.n > 0) cosine = in_query ? sim_ops_apply(cosine, ops) : 0.0f;
	return fminf(fmaxf(cosine, 0.0f), 1.0f);   // clip01 (vk_common.hip.h): xt::clip(sim, 0, 1), NaN -> 0
}

} // namespace vk_host

#endif
