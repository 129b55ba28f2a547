// vk_span_sim.hip -- the span index under a VectorSim that is not the bare cosine (vk_corpus_set_span_sim).
// vk_span_kernel (vk_score.hip) answers a one-row query over one-row slices with the clipped cosine.  Here the score of span i is
// ops(src(span_i, q)) as one float32, UNCLIPPED (the reference's SpanEncoderIndex has no clip):
//   vk_span_sim_kernel<FORM>: src is a p-norm distance or the sqrt-cosine, on the unmodified fp32 rows -- the cell of
//     vk_sim_src_host.h, streamed as vk_span_sim_host.h restates it;
//   vk_span_ops_kernel: src is the cosine -- vk_span_kernel's MFMA chain on the unit tiles with the sums left as the matrix pipe
//     leaves them, the chain as epilogue.
// Both walk the tiles as vk_span_kernel does (runs of consecutive tiles per wave, grid-stride) and store 64 bytes of scores per tile.
#include "vk_common.hip.h"
#include "vk_span_sim_host.h"

// One pass over the unmodified rows per query: ceil(d / 16) KiB per 16 spans.  A block is 16 features of 16 rows in 1 KiB; lane
// 16 g + i holds features 16 b + 4 s + g (s = 0 .. 3) of row i as one 16-byte load.  The workgroup stages the query once in LDS in
// the same order, zero-padded to a whole block: slot 4 b + g holds the query's features 16 b + 4 s + g, one 16-byte read per block,
// the same address across the 16 lanes of a quarter.  Padding features are zero on both sides and their term is +0.0 under every
// form, which leaves the bits of a sum of non-negative terms: no tail branch.  Each lane owns the residue class k mod 4 = g of its
// row -- one double accumulator, adds in ascending k -- and the four lanes of a row combine as (s0 + s1) + (s2 + s3) in two
// exchanges.  kSpanSimDepth blocks (8 KiB per wave) are loaded before the first is used; the rows are read once per query:
// nontemporal.  Nothing is indexed by a run-time value: no scratch.
template <int FORM>
__device__ __forceinline__ void span_sim_block(const f32x4 x, const float4 q, const float p_arg, double &acc, double &abs_a) {
	const float qe[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
	for (int e = 0; e < 4; e++) {
		acc += (double)vk_host::sim_src_term<FORM>(x[e], qe[e], p_arg);
		if constexpr (FORM == vk_host::SIM_SRC_SQRT_COS) abs_a += (double)fabsf(x[e]);
	}
}

template <int FORM>
__global__ __launch_bounds__(256) void vk_span_sim_kernel(VkSpanSimParams p) {
	extern __shared__ float4 vk_span_sim_qlds[];
	const int nb = p.raw_tile_bytes >> 10;
	for (int idx = threadIdx.x; idx < nb * 4; idx += vk_host::kSpanSimThreads) {
		const int b = idx >> 2, g = idx & 3;   // idx == span_sim_q_slot(b, g)
		float v[4];
#pragma unroll
		for (int e = 0; e < 4; e++) {
			const int k = 16 * b + 4 * e + g;
			v[e] = k < p.d ? p.q_row[k] : 0.0f;
		}
		vk_span_sim_qlds[idx] = make_float4(v[0], v[1], v[2], v[3]);
	}
	__syncthreads();
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4;
	const float p_arg = p.src.arg;
	const int64_t n_tiles = vk_host::span_sim_tiles(p.n);
	constexpr int D = vk_host::kSpanSimDepth;
	for (int64_t run = vk_host::span_sim_first_run(blockIdx.x, wv); vk_host::span_sim_run_begin(run) < n_tiles; run += vk_host::span_sim_run_stride(gridDim.x))
	for (int64_t tile = vk_host::span_sim_run_begin(run); tile < vk_host::span_sim_run_end(run, n_tiles); tile++) {
		const uint8_t *__restrict__ tp = p.raw_tiles + tile * (int64_t)p.raw_tile_bytes + lane * 16;
		double acc = 0.0, abs_a = 0.0;
		int b = 0;
#pragma unroll 1
		for (; b + D <= nb; b += D) {
			f32x4 x[D];
#pragma unroll
			for (int i = 0; i < D; i++) x[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(tp + (int64_t)(b + i) * 1024));
			__builtin_amdgcn_sched_barrier(0);   // keep the batch of loads in front of its terms (the scheduler sinks them otherwise)
#pragma unroll
			for (int i = 0; i < D; i++) span_sim_block<FORM>(x[i], vk_span_sim_qlds[4 * (b + i) + g], p_arg, acc, abs_a);
		}
		if (b + 4 <= nb) {
			f32x4 x[4];
#pragma unroll
			for (int i = 0; i < 4; i++) x[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(tp + (int64_t)(b + i) * 1024));
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int i = 0; i < 4; i++) span_sim_block<FORM>(x[i], vk_span_sim_qlds[4 * (b + i) + g], p_arg, acc, abs_a);
			b += 4;
		}
#pragma unroll 1
		for (; b < nb; b++) {
			const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(tp + (int64_t)b * 1024));
			span_sim_block<FORM>(x, vk_span_sim_qlds[4 * b + g], p_arg, acc, abs_a);
		}
		// (s0 + s1) + (s2 + s3) across the lanes i, 16 + i, 32 + i, 48 + i: an IEEE sum does not depend on the order of its two operands
		acc += __shfl_xor(acc, 16, 64);
		acc += __shfl_xor(acc, 32, 64);
		float sum_a = 0.0f;
		if constexpr (FORM == vk_host::SIM_SRC_SQRT_COS) {
			abs_a += __shfl_xor(abs_a, 16, 64);
			abs_a += __shfl_xor(abs_a, 32, 64);
			sum_a = (float)abs_a;
		}
		const int64_t s_idx = tile * 16 + lane;
		if (lane < 16 && s_idx < p.n) {
			float v = vk_host::sim_src_finish<FORM>((float)acc, p_arg, sum_a, p.q_abs_sum);
			if (p.ops.n > 0) v = vk_host::sim_ops_apply(v, p.ops);
			p.scores[s_idx] = v;
		}
	}
}

// The cosine under a chain: vk_span_kernel's instruction sequence -- K ascending, one accumulator chain from zero; the generic
// tile product is the specialised widths' MFMA sequence (vk_common.hip.h) -- without the clip, column 0 kept, the chain on it.
__global__ __launch_bounds__(256) void vk_span_ops_kernel(VkSpanSimParams p) {
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int64_t n_tiles = vk_host::span_sim_tiles(p.n);
	for (int64_t run = vk_host::span_sim_first_run(blockIdx.x, wv); vk_host::span_sim_run_begin(run) < n_tiles; run += vk_host::span_sim_run_stride(gridDim.x))
	for (int64_t tile = vk_host::span_sim_run_begin(run); tile < vk_host::span_sim_run_end(run, n_tiles); tile++) {
		const f32x4 acc = sim_tile_generic<false, -1, false>(p.qtile, p.tiles + tile * (int64_t)p.tile_bytes, p.nk32, p.tail, lane, p.prec);
		const int64_t s_idx = tile * 16 + lane;
		if (lane < 16 && s_idx < p.n) p.scores[s_idx] = vk_host::sim_ops_apply(acc[0], p.ops);   // query column 0, span `lane`
	}
}

static int span_sim_grid_now(int64_t n) {
	int dev = 0, cus = 256, per_cu = vk_host::kSpanSimBlocksPerCu;
	const char *ov = getenv("VK_BLOCKS_PER_CU");   // read per launch, as vk_launch_span does
	if (ov && atoi(ov) > 0) per_cu = atoi(ov);
	if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
	return vk_host::span_sim_grid(n, cus, per_cu);
}

// Internal (tests; not part of the ABI): workgroups of a launch over n spans on the current device (vk_host::span_sim_grid)
extern "C" int32_t vk_span_sim_launch_grid(int64_t n) { return span_sim_grid_now(n); }

extern "C" hipError_t vk_launch_span_sim(const VkSpanSimParams *pp, hipStream_t stream) {
	const VkSpanSimParams &p = *pp;
	if (p.n <= 0) return hipSuccess;
	if (!p.scores) return hipErrorInvalidValue;
	const int grid = span_sim_grid_now(p.n);
	if (p.src.kind == VK_SIMSRC_COSINE) {
		if (!p.tiles || !p.qtile) return hipErrorInvalidValue;
		vk_span_ops_kernel<<<grid, vk_host::kSpanSimThreads, 0, stream>>>(p);
		return hipGetLastError();
	}
	if (!p.raw_tiles || !p.q_row || p.d < 1 || p.d > vk_host::kSimSrcMaxD || p.raw_tile_bytes != vk_host::span_sim_raw_tile_bytes(p.d)) return hipErrorInvalidValue;
	const size_t lds = vk_host::span_sim_lds_bytes(p.d);
	switch (vk_host::sim_src_form(p.src)) {
	case vk_host::SIM_SRC_P1: vk_span_sim_kernel<vk_host::SIM_SRC_P1><<<grid, vk_host::kSpanSimThreads, lds, stream>>>(p); break;
	case vk_host::SIM_SRC_P2: vk_span_sim_kernel<vk_host::SIM_SRC_P2><<<grid, vk_host::kSpanSimThreads, lds, stream>>>(p); break;
	case vk_host::SIM_SRC_PGEN: vk_span_sim_kernel<vk_host::SIM_SRC_PGEN><<<grid, vk_host::kSpanSimThreads, lds, stream>>>(p); break;
	default: vk_span_sim_kernel<vk_host::SIM_SRC_SQRT_COS><<<grid, vk_host::kSpanSimThreads, lds, stream>>>(p); break;
	}
	return hipGetLastError();
}
