// vk_sim_src_host.h -- the vector similarities beside the cosine that a static corpus computes (vk_corpus_set_sim_source):
// PNormDistance (vectorian/sim/vector.py:135-160) and ImprovedSqrtCosineSim (:98-132), one definition for the host and the device.
// Both run on the UNMODIFIED fp32 vectors.  The reference states a cell as numpy calls over the feature axis; sim_src_cell() is that
// cell:
//   * every TERM in fp32, one rounding per numpy operation of the reference, nothing contracted --
//       p-norm, p = 1:   |a_k - b_k|                         (difference, absolute value; np.power(x, 1) is x)
//       p-norm, p = 2:   t = |a_k - b_k|, t * t              (np.power(x, 2) is the product)
//       p-norm, other p: powf(|a_k - b_k|, p)
//       sqrt-cosine:     sqrtf(max(0, fl32(a_k b_k)))        (the reference doubles every vector into max(0, x), max(0, -x): of the
//                                                             two products of a feature at most one is non-zero, and it is a_k b_k)
//   * every SUM over the features in double, in a FIXED order, rounded to fp32 once: four partial sums, s[g] over the features
//     k = g, g + 4, g + 8, .. (k mod 4 = g) in ascending k, combined as (s[0] + s[1]) + (s[2] + s[3]).  That is the order in which a
//     wave streams the fp32 tile layout (vk_pack_rows_kernel: lane 16 g + i holds features 16 b + 4 s + g of row i) with coalesced
//     1 KiB loads: one partial sum per lane, two exchanges across the four lanes of a row (vk_source_table_kernel, vk_pack.hip).
//     (The reference sums in fp32, pairwise: a few ulp away)
//   * the FINISH in fp32 --
//       p = 1: the sum;  p = 2: sqrtf(sum);  other p: powf(sum, fl32(1 / p))  (np.power(d, 1 / p): 1 / p in double, then float32)
//       sqrt-cosine: sum / (sqrtf(sum_k |a_k|) * sqrtf(sum_k |b_k|)), the two sums in the order above; a quotient that is not
//       finite (a zero vector: 0 / 0) is 0 (nan_to_num).
// The operator chain (vk_sim_ops_host.h), sim[id(t_j)][j] = 1 and the clip follow in the table kernel.  Under such a source the
// table's cell IS the canonical cell: the winners' restatements read it (static_table_cell, vk_common.hip.h).
// No HIP types: tests/test_vector_sim_host.py compiles this header with g++, plain and under AddressSanitizer / UBSan, and holds the
// exactly rounded forms against a numpy restatement of the order above bit for bit (CPU tier).
#ifndef VK_SIM_SRC_HOST_H
#define VK_SIM_SRC_HOST_H

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

// the source of a handle (kind: VK_SIMSRC_*; arg: p of the p-norm).  A kernel argument by value: every branch on it is wave-uniform
struct sim_src {
	int32_t kind;
	float arg;
};

// the four forms of the table kernel
enum { SIM_SRC_P1 = 0, SIM_SRC_P2 = 1, SIM_SRC_PGEN = 2, SIM_SRC_SQRT_COS = 3 };

// rows wider than this do not run under a source: the table kernel keeps a query tile's 16 fp32 rows in LDS (64 KiB)
constexpr int kSimSrcMaxD = 1024;

// VK_OK, or VK_ERR_INVALID: an unknown kind, p not finite or <= 0
inline int sim_src_check(int32_t kind, float arg) {
	if (kind == VK_SIMSRC_COSINE || kind == VK_SIMSRC_SQRT_COSINE) return VK_OK;
	if (kind != VK_SIMSRC_PNORM) return VK_ERR_INVALID;
	return (std::isfinite(arg) && arg > 0.0f) ? VK_OK : VK_ERR_INVALID;
}

VK_HOST_DEVICE inline int sim_src_form(const sim_src &src) {
	if (src.kind == VK_SIMSRC_SQRT_COSINE) return SIM_SRC_SQRT_COS;
	return src.arg == 1.0f ? SIM_SRC_P1 : src.arg == 2.0f ? SIM_SRC_P2 : SIM_SRC_PGEN;
}

template <int FORM>
VK_HOST_DEVICE inline float sim_src_term(float a, float b, float p) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (FORM == SIM_SRC_SQRT_COS) {
		const float ab = a * b;
		return sqrtf(fmaxf(0.0f, ab));
	}
	const float diff = a - b;
	const float t = fabsf(diff);
	if (FORM == SIM_SRC_P1) return t;
	if (FORM == SIM_SRC_P2) return t * t;
	return powf(t, p);
}

// the four partial sums into one float
VK_HOST_DEVICE inline float sim_src_combine(double s0, double s1, double s2, double s3) { return (float)((s0 + s1) + (s2 + s3)); }

// sum_a, sum_b: sum_k |a_k|, sum_k |b_k| (sqrt-cosine only)
template <int FORM>
VK_HOST_DEVICE inline float sim_src_finish(float sum, float p, float sum_a, float sum_b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (FORM == SIM_SRC_P1) return sum;
	if (FORM == SIM_SRC_P2) return sqrtf(sum);
	if (FORM == SIM_SRC_PGEN) return powf(sum, (float)(1.0 / (double)p));
	const float x = sqrtf(sum_a), y = sqrtf(sum_b);
	const float denom = x * y;
	const float q = sum / denom;
	return (q - q) == 0.0f ? q : 0.0f;   // (q - q is 0 exactly for the finite floats)
}

// sum_k |a_k| in the order above
inline float sim_src_abs_sum(const float *a, int d) {
	double s[4] = {0.0, 0.0, 0.0, 0.0};
	for (int k = 0; k < d; k++) s[k & 3] += (double)fabsf(a[k]);
	return sim_src_combine(s[0], s[1], s[2], s[3]);
}

template <int FORM>
inline float sim_src_cell_form(const float *a, const float *b, int d, float p) {
	double s[4] = {0.0, 0.0, 0.0, 0.0};
	for (int k = 0; k < d; k++) s[k & 3] += (double)sim_src_term<FORM>(a[k], b[k], p);
	const float sum = sim_src_combine(s[0], s[1], s[2], s[3]);
	if (FORM != SIM_SRC_SQRT_COS) return sim_src_finish<FORM>(sum, p, 0.0f, 0.0f);
	return sim_src_finish<FORM>(sum, p, sim_src_abs_sum(a, d), sim_src_abs_sum(b, d));
}

// one cell: vectors a and b of d features under `src` (not the cosine)
inline float sim_src_cell(const float *a, const float *b, int d, const sim_src &src) {
	switch (sim_src_form(src)) {
	case SIM_SRC_P1: return sim_src_cell_form<SIM_SRC_P1>(a, b, d, src.arg);
	case SIM_SRC_P2: return sim_src_cell_form<SIM_SRC_P2>(a, b, d, src.arg);
	case SIM_SRC_PGEN: return sim_src_cell_form<SIM_SRC_PGEN>(a, b, d, src.arg);
	default: return sim_src_cell_form<SIM_SRC_SQRT_COS>(a, b, d, src.arg);
	}
}

} // namespace vk_host

#endif
