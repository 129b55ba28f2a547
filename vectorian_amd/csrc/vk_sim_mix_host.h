// vk_sim_mix_host.h -- the token similarity combinators of a static corpus (vk_corpus_set_sim_mix): MixedTokenSimilarity and
// MaximumTokenSimilarity of vectorian/sim/modifier.py, one definition for the host and the device.  The reference builds every
// operand's matrix completely -- VectorSim, chain, sim[id(t_j)][j] = 1, clip (metric/static.cpp:9-78) -- and hands the clipped float32
// matrices to the Python operator (metric/modifier.cpp:18-74); nothing is clipped afterwards.  sim_mix_cell() is that operator for one
// cell:
//   AVERAGE  out[:] = np.average([S_0 .. S_{M-1}], axis=0, weights=w).  With float32 matrices and Python weights numpy runs this in
//            float64: acc = sum_m double(S_m) * double(w_m), added in operand order; the weights added in the same order; acc / that
//            sum, rounded to float32 once on assignment.  (M < 8: numpy's sum is a plain loop there.)  Nothing contracted.
//   MAXIMUM  np.choose(np.argmax(..)): the cell-wise maximum of the float32 cells, the first of equal values (the same float).
//            MinimumTokenSimilarity computes this too: upstream's ExtremumTokenSimilarity.__call__ never reads its operator.
// Zeros map to zero under both, so the padding of the operands' tables needs no mask.  No HIP types: tests/test_sim_mix_host.py
// compiles the header with g++ under AddressSanitizer and UBSan and holds it against numpy bit for bit (CPU tier).
#ifndef VK_SIM_MIX_HOST_H
#define VK_SIM_MIX_HOST_H

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

// the combinator of a handle: kind VK_SIMMIX_*, n operands (operand 0 is the handle itself), the weights of AVERAGE.  A kernel
// argument by value
struct sim_mix {
	int32_t kind;
	int32_t n;
	double w[VK_MAX_SIM_OPERANDS];
};

// VK_OK, or VK_ERR_INVALID with the reason vk_corpus_set_sim_mix refuses in *why
inline int sim_mix_check(int32_t kind, int32_t n_operands, const double *weights, const char **why) {
	*why = "";
	if (kind != VK_SIMMIX_AVERAGE && kind != VK_SIMMIX_MAXIMUM) { *why = "unknown kind"; return VK_ERR_INVALID; }
	if (n_operands < 2 || n_operands > VK_MAX_SIM_OPERANDS) { *why = "n_operands must be 2 .. VK_MAX_SIM_OPERANDS (4)"; return VK_ERR_INVALID; }
	if (kind != VK_SIMMIX_AVERAGE) return VK_OK;
	if (!weights) { *why = "VK_SIMMIX_AVERAGE needs weights"; return VK_ERR_INVALID; }
	double sum = 0.0;
	for (int m = 0; m < n_operands; m++) {
		if (!std::isfinite(weights[m]) || weights[m] < 0.0) { *why = "a weight is negative or not finite"; return VK_ERR_INVALID; }
		sum += weights[m];
	}
	if (!(sum > 0.0) || !std::isfinite(sum)) { *why = "the weights must sum to more than 0"; return VK_ERR_INVALID; }
	return VK_OK;
}

// cells[m]: operand m's clipped cell, m < mix.n (the loops run to the constant bound so that a kernel keeps `cells` in registers)
VK_HOST_DEVICE inline float sim_mix_cell(const float *cells, const sim_mix &mix) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (mix.kind == VK_SIMMIX_AVERAGE) {
		double acc = (double)cells[0] * mix.w[0], scl = mix.w[0];
		VK_UNROLL
		for (int m = 1; m < VK_MAX_SIM_OPERANDS; m++)
			if (m < mix.n) {
				const double prod = (double)cells[m] * mix.w[m];
				acc = acc + prod;
				scl = scl + mix.w[m];
			}
		return (float)(acc / scl);
	}
	float best = cells[0];
	VK_UNROLL
	for (int m = 1; m < VK_MAX_SIM_OPERANDS; m++)
		if (m < mix.n && cells[m] > best) best = cells[m];
	return best;
}

} // namespace vk_host

#endif
