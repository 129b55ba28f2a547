// vk_pool.hip -- span vectors pooled from token rows on the device (vk_corpus_append_pooled): a segmented reduction over
// token rows, bound by the bytes of the rows.  The arithmetic of a cell and the launch geometry: vk_pool_host.h.
#include "vk_common.hip.h"
#include "vk_pool_host.h"

namespace {

constexpr int kChunks = vk_host::kPoolChunksPerPass, kRows = vk_host::kPoolRowsInFlight, kIdBatch = vk_host::kPoolIdBatch;
static_assert(kIdBatch == 64, "a wave's lanes hold one token id each");
static_assert(kIdBatch % kRows == 0, "a batch of ids is whole groups of rows in flight");

// VEC features of a row, from its element `at`, widened to fp32
template <typename T, int VEC> struct pool_piece;
template <> struct pool_piece<float, 4> {
	static __device__ __forceinline__ void load(const float *__restrict__ p, float (&x)[4]) {
		const float4 v = *reinterpret_cast<const float4 *>(p);
		x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
	}
};
template <> struct pool_piece<float, 1> {
	static __device__ __forceinline__ void load(const float *__restrict__ p, float (&x)[1]) { x[0] = *p; }
};
template <> struct pool_piece<uint16_t, 4> {
	static __device__ __forceinline__ void load(const uint16_t *__restrict__ p, float (&x)[4]) {
		const uint2 v = *reinterpret_cast<const uint2 *>(p);
		x[0] = __builtin_bit_cast(float, v.x << 16); x[1] = __builtin_bit_cast(float, v.x & 0xffff0000u);
		x[2] = __builtin_bit_cast(float, v.y << 16); x[3] = __builtin_bit_cast(float, v.y & 0xffff0000u);
	}
};
template <> struct pool_piece<uint16_t, 1> {
	static __device__ __forceinline__ void load(const uint16_t *__restrict__ p, float (&x)[1]) { x[0] = vk_host::pool_widen_bf16(*p); }
};

}   // namespace

// One wave per span (vk_host::pool_span_of).  Lanes own features: lane l holds VEC consecutive features of each of kChunks chunks of
// 64 * VEC features (vk_host::pool_feature_of) and walks a row wider than that in passes.  Per pass the wave walks the span's tokens
// in ascending order, kRows rows at a time: the loads of the group are issued together (a row past the span's end is its last row
// again, so that the loads stay unconditional), then folded row by row -- the order of the sum is the header's, and what is in flight
// comes from the loads of a group and from the other waves of the SIMD.  GATHER: the row of token t is ids[t]; a wave loads 64 ids at
// a time, one per lane, and reads each back as a scalar (v_readlane).  Every index of acc[][] and x[][][] is a constant once the loops
// are unrolled: nothing goes to scratch (tests/test_pool_registers.py).
// The host has checked every span against the rows / ids and every id against the rows (vk_host::pool_check_spans).
template <int AGG, bool GATHER, typename T, int VEC>
__global__ __launch_bounds__(vk_host::kPoolThreads) void vk_pool_spans_kernel(const T *__restrict__ rows, const int32_t *__restrict__ ids,
	const int64_t *__restrict__ start, const int64_t *__restrict__ end, int64_t n_spans, int32_t d, float *__restrict__ out) {
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int64_t span = vk_host::pool_span_of(blockIdx.x, wave);
	if (span >= n_spans) return;
	const int64_t a = start[span], b = end[span];
	float *__restrict__ orow = out + span * (int64_t)d;
	const int n_pass = vk_host::pool_passes(d, VEC);
#pragma unroll 1
	for (int pass = 0; pass < n_pass; pass++) {
		// chunk c of this pass is live (some lane owns features of it) while c < live: uniform
		const int f_lane = vk_host::pool_feature_of(pass, 0, lane, VEC);
		const int left = d - vk_host::pool_feature_of(pass, 0, 0, VEC);
		const int live = min(kChunks, (left + 64 * VEC - 1) / (64 * VEC));
		float acc[kChunks][VEC];
#pragma unroll
		for (int c = 0; c < kChunks; c++)
#pragma unroll
			for (int e = 0; e < VEC; e++) acc[c][e] = vk_host::pool_nan();
#pragma unroll 1
		for (int64_t t0 = a; t0 < b; t0 += kIdBatch) {
			const int m = (int)min((int64_t)kIdBatch, b - t0);   // tokens of this batch
			int my_id = 0;
			if constexpr (GATHER) my_id = ids[t0 + min(lane, m - 1)];
#pragma unroll 1
			for (int j = 0; j < m; j += kRows) {
				float x[kRows][kChunks][VEC];
#pragma unroll
				for (int r = 0; r < kRows; r++) {
					const int jr = min(j + r, m - 1);
					const int64_t row = GATHER ? (int64_t)__builtin_amdgcn_readlane(my_id, jr) : t0 + jr;
					const T *__restrict__ rp = rows + row * (int64_t)d + f_lane;
#pragma unroll
					for (int c = 0; c < kChunks; c++) {
						if (c < live) {
							if (f_lane + c * 64 * VEC < d) pool_piece<T, VEC>::load(rp + c * 64 * VEC, x[r][c]);
							else {
#pragma unroll
								for (int e = 0; e < VEC; e++) x[r][c][e] = 0.0f;
							}
						}
					}
				}
#pragma unroll
				for (int r = 0; r < kRows; r++) {
					if (j + r < m) {
						const bool first = t0 == a && j + r == 0;
#pragma unroll
						for (int c = 0; c < kChunks; c++) {
							if (c < live) {
#pragma unroll
								for (int e = 0; e < VEC; e++) acc[c][e] = first ? x[r][c][e] : vk_host::pool_fold<AGG>(acc[c][e], x[r][c][e]);
							}
						}
					}
				}
			}
		}
#pragma unroll
		for (int c = 0; c < kChunks; c++) {
			if (c < live && f_lane + c * 64 * VEC < d) {
				float v[VEC];
#pragma unroll
				for (int e = 0; e < VEC; e++) v[e] = b > a ? vk_host::pool_finish<AGG>(acc[c][e], b - a) : acc[c][e];
				float *__restrict__ op = orow + f_lane + c * 64 * VEC;
				if constexpr (VEC == 4) *reinterpret_cast<float4 *>(op) = make_float4(v[0], v[1], v[2], v[3]);
				else *op = v[0];
			}
		}
	}
}

// rows: [n_rows x d] fp32 or bf16 bits on the device; ids: null, or the row of every token; start / end: the spans, int64 on the
// device; out: [n_spans x d] fp32.  The form (16-byte pieces or single elements) follows the width and the base of the rows.
extern "C" hipError_t vk_launch_pool_spans(const void *rows, int32_t dtype_bf16, const int32_t *ids, const int64_t *start, const int64_t *end,
	int64_t n_spans, int32_t d, int32_t agg, float *out, hipStream_t stream) {
	if (n_spans <= 0) return hipSuccess;
	if (d < 1 || d > vk_host::kPoolMaxD || !vk_host::pool_agg_ok(agg) || !start || !end || !out) return hipErrorInvalidValue;   // (rows may be null: spans without tokens read none)
	const int64_t grid64 = vk_host::pool_grid(n_spans);
	if (grid64 > 0x7fffffffll) return hipErrorInvalidValue;
	const unsigned grid = (unsigned)grid64;
	const int vec = ((uintptr_t)out % 16 == 0) ? vk_host::pool_vec(d, dtype_bf16 ? 2 : 4, (uintptr_t)rows) : 1;
#define VK_POOL_FORM(AGG, GATHER, T, VEC) \
	vk_pool_spans_kernel<AGG, GATHER, T, VEC><<<grid, vk_host::kPoolThreads, 0, stream>>>((const T *)rows, ids, start, end, n_spans, d, out)
#define VK_POOL_VEC(AGG, GATHER, T) do { if (vec == 4) VK_POOL_FORM(AGG, GATHER, T, 4); else VK_POOL_FORM(AGG, GATHER, T, 1); } while (0)
#define VK_POOL_T(AGG, GATHER) do { if (dtype_bf16) VK_POOL_VEC(AGG, GATHER, uint16_t); else VK_POOL_VEC(AGG, GATHER, float); } while (0)
#define VK_POOL_GATHER(AGG) do { if (ids) VK_POOL_T(AGG, true); else VK_POOL_T(AGG, false); } while (0)
	switch (agg) {
	case vk_host::POOL_MEAN: VK_POOL_GATHER(vk_host::POOL_MEAN); break;
	case vk_host::POOL_MIN: VK_POOL_GATHER(vk_host::POOL_MIN); break;
	default: VK_POOL_GATHER(vk_host::POOL_MAX); break;
	}
#undef VK_POOL_GATHER
#undef VK_POOL_T
#undef VK_POOL_VEC
#undef VK_POOL_FORM
	return hipGetLastError();
}
