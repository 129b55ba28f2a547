// vk_pack.hip -- corpus upload (normalise, round, tile order) and the per-query table of the static layout.
#include "vk_common.hip.h"
#include "vk_bound_host.h"   // the format of a shadow and the quantizer of a row (host and device)
#include "vk_sim_src_host.h" // the cell of a source that is not the cosine (host and device)

// ---------------------------------------------------------------------------
// corpus upload: L2-normalise rows (Vectors.normalized, vectorian/embedding/vectors.py:71-86),
// round to bf16 (RNE) and store in tile order.  One wave per row.
// ---------------------------------------------------------------------------

template <typename T> __device__ __forceinline__ float load_elem(const T *p);
template <> __device__ __forceinline__ float load_elem<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float load_elem<uint16_t>(const uint16_t *p) {
	return __builtin_bit_cast(float, ((uint32_t)*p) << 16);
}

template <typename T>
__global__ __launch_bounds__(256) void vk_pack_rows_kernel(
	const T *__restrict__ in, int64_t n_rows, int32_t d, int32_t d_pad, int64_t row0,
	uint8_t *__restrict__ tiles, float *__restrict__ mag_out, int32_t normalize, int32_t prec) {

	const int lane = threadIdx.x & 63;
	const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (r >= n_rows) return;
	const T *row = in + r * (int64_t)d;

	float m = 1.0f;
	if (normalize || mag_out) {
		double acc = 0.0;
		for (int k = lane; k < d; k += 64) {
			const double x = (double)load_elem<T>(row + k);
			acc += x * x;
		}
		for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
		m = (float)sqrt(acc);
		if (m != m) m = 0.0f;
		if (mag_out && lane == 0) mag_out[row0 + r] = m;
	}

	const int64_t grow = row0 + r;
	const int64_t tile = grow >> 4;
	const int i = (int)(grow & 15);
	const int nk32 = d_pad >> 5;
	const int tile_bytes = prec ? d_pad * 64 : d_pad * 32;
	uint8_t *tp = tiles + tile * (int64_t)tile_bytes;
	if (prec) {
		// fp32 tiles (operand order of v_mfma_f32_16x16x4_f32): a block of 16 features is 1 KiB; lane 16 g + i owns
		// row i, features 16 b + 4 s + g for s = 0..3 (element s feeds MFMA step s)
		for (int k = lane; k < d_pad; k += 64) {
			float x = 0.0f;
			if (k < d) {
				x = load_elem<T>(row + k);
				if (normalize) {
					x = x / m;
					if (x != x) x = 0.0f;
				}
			}
			const int b = k >> 4, sidx = (k & 15) >> 2, g = k & 3;
			*reinterpret_cast<float *>(tp + b * 1024 + (g * 16 + i) * 16 + sidx * 4) = x;
		}
		return;
	}

	const int n8 = d_pad >> 3;                  // 8-element chunks; chunk c: K-step c>>2, lane group c&3
	(void)nk32;
	for (int c = lane; c < n8; c += 64) {
		const int k0 = c * 8;
		const int off = (c >> 2) * 1024 + ((c & 3) * 16 + i) * 16;
		uint16_t v[8];
		for (int j = 0; j < 8; j++) {
			float x = 0.0f;
			if (k0 + j < d) {
				x = load_elem<T>(row + k0 + j);
				if (normalize) {
					x = x / m;
					if (x != x) x = 0.0f;
				}
			}
			v[j] = f32_to_bf16_rne(x);
		}
		uint4 w;
		w.x = v[0] | ((uint32_t)v[1] << 16); w.y = v[2] | ((uint32_t)v[3] << 16);
		w.z = v[4] | ((uint32_t)v[5] << 16); w.w = v[6] | ((uint32_t)v[7] << 16);
		*reinterpret_cast<uint4 *>(tp + off) = w;
	}
}

// ---------------------------------------------------------------------------
// The shadow of a bf16 contextual corpus, built once at vk_corpus_finalize in the format vk_bound_host.h
// describes.  One thread per row: vk_host::quantize_row on the format's grid -- the function the query's side runs on the host --
// reading the row out of its token tile and collecting each lane's operand, which one vector store (the E2M3 grid: two) puts where
// i8_offset / fp6_store_lane put it; features >= d are zero codes, rows past the corpus zeros throughout.  stats[0] / [1]: the
// largest |s_x xq| / |x| of the corpus as float bits (non-negative floats order as their bits), stats[2]: some element is not
// finite (no shadow then).
// ---------------------------------------------------------------------------

// the operand a lane collects, code by code (its place in the operand is a constant once quantize_row's loop is unrolled), and stores
// when it is whole.  int8: sixteen codes, one uint4
template <typename Grid> struct lane_operand;
template <> struct lane_operand<vk_host::grid_i8> {
	uint32_t w[4];
	__device__ __forceinline__ void put(const vk_host::shadow_format &, uint8_t *dst, int i, int k, int code) {
		const int j = k & 15;
		if ((j & 3) == 0) w[j >> 2] = 0u;
		w[j >> 2] |= ((uint32_t)code & 255u) << ((j & 3) * 8);
		if (j == 15) *reinterpret_cast<uint4 *>(dst + vk_host::i8_offset(i, k - 15)) = uint4{w[0], w[1], w[2], w[3]};
	}
};
// E2M3: thirty-two codes through the host's packer, a uint4 and a uint2
template <> struct lane_operand<vk_host::grid_e2m3> {
	uint8_t codes[32];
	__device__ __forceinline__ void put(const vk_host::shadow_format &f, uint8_t *dst, int i, int k, int code) {
		const int j = k & 31;
		codes[j] = (uint8_t)code;
		if (j != 31) return;
		uint32_t w[6];
		vk_host::fp6_pack32(codes, w);
		const int t = k >> 7, quarters = t == f.steps - 1 ? f.kept : 4, lane = 16 * ((k & 127) >> 5) + i;
		uint8_t *step = dst + t * f.step_bytes();
		if (f.compact && t == f.steps - 1) {   // parts P and Q (quarters 0 and 1: the walk ends at 320 features)
			vk_host::fp6c_store_lane(step, lane, w);
			return;
		}
		*reinterpret_cast<uint4 *>(step + lane * 16) = uint4{w[0], w[1], w[2], w[3]};
		*reinterpret_cast<uint2 *>(step + quarters * 256 + lane * 8) = uint2{w[4], w[5]};
	}
};

template <typename Grid>
__global__ __launch_bounds__(256) void vk_shadow_kernel(const uint8_t *__restrict__ tiles, int64_t n_tiles, int64_t rows_total, int32_t tile_bytes,
	const vk_host::shadow_format f, uint8_t *__restrict__ shadow, uint32_t *__restrict__ stats) {
	const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= n_tiles * 16) return;
	const int i = (int)(row & 15);
	const uint8_t *src = tiles + (row >> 4) * (int64_t)tile_bytes;
	uint8_t *dst = shadow + (row >> 4) * (int64_t)f.tile_bytes();
	const int dk = row < rows_total ? f.d : 0;   // rows past the corpus (the tile's padding, the zero tile): zeros
	bool bad = false;
	lane_operand<Grid> op;
	const vk_host::quant_meta m = vk_host::quantize_row<Grid>(dk, f.walk(),
		[&](int k) {
			const float x = tile_elem(src, i, k, 0);
			bad = bad || !(fabsf(x) <= 3.4028234e38f);
			return x;
		},
		[&](int k, int code) { op.put(f, dst, i, k, code); }, f.compact != 0);
	if (f.compact) *reinterpret_cast<uint32_t *>(dst + f.meta_offset() + i * 4) = vk_host::fp6c_meta(m.s, m.e);
	else *reinterpret_cast<float2 *>(dst + f.meta_offset() + i * 8) = float2{m.s, m.e};
	if (bad) atomicOr(stats + 2, 1u);
	else {
		atomicMax(stats + 0, __builtin_bit_cast(uint32_t, m.n));
		atomicMax(stats + 1, __builtin_bit_cast(uint32_t, m.a));
	}
}

// the host's description of the 6-bit form is the one the bound kernel is compiled with (vk_device.h), at every number of live quarters
constexpr vk_host::shadow_format fmt6_of(int d) { return vk_host::shadow_format_of(d, 10, 1, 0, VK_LAYOUT_CONTEXTUAL, 6); }
constexpr bool fmt6_is_the_devices(int d, int live) {
	return fmt6_of(d).live == live && fmt6_of(d).steps == VK_DEV_FP6_STEPS && fmt6_of(d).step_bytes() == VK_DEV_FP6_STEP_BYTES
		&& fmt6_of(d).tile_bytes() == VK_DEV_FP6_TILE_BYTES(live) && fmt6_of(d).qtile_bytes() == VK_DEV_FP6_QTILE_BYTES;
}
static_assert(fmt6_is_the_devices(257, 1) && fmt6_is_the_devices(289, 2) && fmt6_is_the_devices(304, 2) && fmt6_is_the_devices(321, 3) && fmt6_is_the_devices(384, 4),
	"vk_host::shadow_format and VK_DEV_FP6_*");
// ... and so is its description of the compact form
constexpr vk_host::shadow_format fmt6c_of(int d) { return vk_host::shadow_format_of(d, 10, 1, 0, VK_LAYOUT_CONTEXTUAL, vk_host::bits6_compact); }
constexpr bool fmt6c_is_the_devices(int d) {
	return fmt6c_of(d).compact == 1 && fmt6c_of(d).bits == 6 && fmt6c_of(d).live == 2 && fmt6c_of(d).steps == VK_DEV_FP6_STEPS && fmt6c_of(d).step_bytes() == VK_DEV_FP6_STEP_BYTES
		&& fmt6c_of(d).meta_offset() == VK_DEV_FP6C_META_OFFSET && fmt6c_of(d).tile_bytes() == VK_DEV_FP6C_TILE_BYTES && fmt6c_of(d).qtile_bytes() == VK_DEV_FP6_QTILE_BYTES
		&& fmt6c_of(d).width() == 304 && fmt6c_of(d).walk() == 320;
}
static_assert(fmt6c_is_the_devices(289) && fmt6c_is_the_devices(300) && fmt6c_is_the_devices(304), "vk_host::shadow_format and VK_DEV_FP6C_*");

extern "C" hipError_t vk_launch_shadow(const uint8_t *tiles, int64_t n_tiles, int64_t rows_total, int32_t tile_bytes, const vk_host::shadow_format *f,
	uint8_t *shadow, uint32_t *stats, hipStream_t stream) {
	if (f->bits == 0 || f->live < 1 || f->live > 4 || f->kept < f->live || f->kept > 4 || f->d > f->width()) return hipErrorInvalidValue;
	hipError_t e = hipMemsetAsync(stats, 0, 16, stream);
	if (e != hipSuccess) return e;
	const unsigned grid = (unsigned)((n_tiles * 16 + 255) / 256);
	if (f->bits == 8) vk_shadow_kernel<vk_host::grid_i8><<<grid, 256, 0, stream>>>(tiles, n_tiles, rows_total, tile_bytes, *f, shadow, stats);
	else vk_shadow_kernel<vk_host::grid_e2m3><<<grid, 256, 0, stream>>>(tiles, n_tiles, rows_total, tile_bytes, *f, shadow, stats);
	return hipGetLastError();
}

// One v_mfma_i32_16x16x64_i8 on a query tile and a token tile of 16 rows x 64 int8 each, row-major in, packed as the shadow packs
// them: out[16 j + i] = sum_k q[j][k] x[i][k].  The lane map of the operands, checked with exact integers (tests/test_gpu_bound_pass.py).
__global__ void vk_i8_probe_kernel(const int8_t *__restrict__ q, const int8_t *__restrict__ x, int32_t *__restrict__ out) {
	const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
	const i32x4 a = *reinterpret_cast<const i32x4 *>(q + i * 64 + g * 16);
	const i32x4 b = *reinterpret_cast<const i32x4 *>(x + i * 64 + g * 16);
	i32x4 acc = {0, 0, 0, 0};
	acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
	for (int r = 0; r < 4; r++) out[(4 * g + r) * 16 + i] = acc[r];
}
extern "C" hipError_t vk_launch_i8_probe(const int8_t *q, const int8_t *x, int32_t *out, hipStream_t stream) {
	vk_i8_probe_kernel<<<1, 64, 0, stream>>>(q, x, out);
	return hipGetLastError();
}

// One shadow tile against one 8-bit query tile, both in the shadow's block order already, through the bound kernel's own product:
// the query tile staged in LDS as MODE 7 stages it, dot_tile_i8<NK> with `live` quarters of the last block fetched
// (tests/test_gpu_bound_live_bytes.py: the bytes of the dead quarters must not reach the product).
template <int NK>
__global__ __launch_bounds__(64) void vk_i8_bound_probe_kernel(const uint8_t *__restrict__ qtile8, const uint8_t *__restrict__ tile8, int32_t live,
	int32_t *__restrict__ out) {
	__shared__ float4 qlds4[NK * 64];
	const int lane = threadIdx.x;
	for (int i = lane; i < NK * 64; i += 64) qlds4[i] = *reinterpret_cast<const float4 *>(qtile8 + i * 16);
	__syncthreads();
	const i32x4 acc = dot_tile_i8<NK>(reinterpret_cast<const uint8_t *>(qlds4), tile8, lane, live);
	for (int r = 0; r < 4; r++) out[(4 * (lane >> 4) + r) * 16 + (lane & 15)] = acc[r];
}
extern "C" hipError_t vk_launch_i8_bound_probe(const uint8_t *qtile8, const uint8_t *tile8, int32_t nk64, int32_t live, int32_t *out, hipStream_t stream) {
	if (live < 1 || live > 4) return hipErrorInvalidValue;
	if (nk64 == 5) vk_i8_bound_probe_kernel<5><<<1, 64, 0, stream>>>(qtile8, tile8, live, out);
	else if (nk64 == 12) vk_i8_bound_probe_kernel<12><<<1, 64, 0, stream>>>(qtile8, tile8, live, out);
	else return hipErrorInvalidValue;
	return hipGetLastError();
}

// One 6-bit shadow tile against one 6-bit query tile, both packed already, through the bound kernel's own product: the query tile
// staged in LDS as MODE 8 stages it, dot_tile_fp6 with `live6` quarters in the tile's last K-step (tests/test_gpu_bound6_product.py)
// COMPACT: the tile is a compact one (MODE 9's loads, tests/test_gpu_bound_compact_product.py); live6 is not read
template <bool COMPACT>
__global__ __launch_bounds__(64) void vk_fp6_bound_probe_kernel(const uint8_t *__restrict__ qtile6, const uint8_t *__restrict__ tile6, int32_t live6,
	float *__restrict__ out) {
	__shared__ float4 qlds4[VK_DEV_FP6_QTILE_BYTES / 16];
	const int lane = threadIdx.x;
	for (int i = lane; i < VK_DEV_FP6_QTILE_BYTES / 16; i += 64) qlds4[i] = *reinterpret_cast<const float4 *>(qtile6 + i * 16);
	__syncthreads();
	const f32x4 acc = dot_tile_fp6<COMPACT>(reinterpret_cast<const uint8_t *>(qlds4), tile6, lane, live6);
	for (int r = 0; r < 4; r++) out[(4 * (lane >> 4) + r) * 16 + (lane & 15)] = acc[r];
}
extern "C" hipError_t vk_launch_fp6c_bound_probe(const uint8_t *qtile6, const uint8_t *tile6c, float *out, hipStream_t stream) {
	vk_fp6_bound_probe_kernel<true><<<1, 64, 0, stream>>>(qtile6, tile6c, 2, out);
	return hipGetLastError();
}
extern "C" hipError_t vk_launch_fp6_bound_probe(const uint8_t *qtile6, const uint8_t *tile6, int32_t live6, float *out, hipStream_t stream) {
	if (live6 < 1 || live6 > 4) return hipErrorInvalidValue;
	vk_fp6_bound_probe_kernel<false><<<1, 64, 0, stream>>>(qtile6, tile6, live6, out);
	return hipGetLastError();
}

// ---------------------------------------------------------------------------
// static layout: per-query similarity table [V_pad x 16] (metric/static.cpp:9-78)
// ---------------------------------------------------------------------------

// OPS: under an operator chain (vk_corpus_set_sim_ops) -- the tile product without its clip, the chain on the cells of the V vocabulary
// rows x the len_t query columns, then the clip; the padding of either side stays zero.  Without a chain: the kernel as it always was.
template <bool OPS>
__global__ __launch_bounds__(256) void vk_table_kernel(const uint8_t *__restrict__ etiles, const uint8_t *__restrict__ qtile,
	int32_t n_tiles, int32_t nk32, int32_t tail, int32_t tile_bytes, float *__restrict__ table, int32_t prec, int32_t len_t, int32_t V,
	const vk_host::sim_ops ops) {
	const int lane = threadIdx.x & 63;
	const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (tile >= n_tiles) return;
	f32x4 acc = sim_tile_generic<false, -1, !OPS>(qtile, etiles + (int64_t)tile * tile_bytes, nk32, tail, lane, prec);
	if constexpr (OPS) {
		const bool word = tile * 16 + (lane & 15) < V;
#pragma unroll
		for (int r = 0; r < 4; r++) acc[r] = static_cell(acc[r], false, word && (lane >> 4) * 4 + r < len_t, ops);
	}
	*reinterpret_cast<f32x4 *>(table + ((int64_t)tile * 16 + (lane & 15)) * 16 + (lane >> 4) * 4) = acc;
}

// The same table under a source that is not the cosine (vk_corpus_set_sim_source; the cell: vk_sim_src_host.h), from the fp32 copy of
// the UNMODIFIED vocabulary rows (fp32 tile layout: a block of 16 features is 1 KiB, lane 16 g + i owns row i, features
// 16 b + 4 s + g for s = 0..3) and the query tile's unmodified rows.  A workgroup stages the query rows in LDS in the same order --
// qlds[(4 b + g) * 16 + j]: features 16 b + 4 s + g of query row j, one 16-byte read per column, the same address for the 16 lanes
// of a quarter -- and each of its four waves takes one vocabulary tile: one coalesced 1 KiB load per block, the terms of the lane's
// row against the len_t live columns into double partial sums (the lane's are those of the features k mod 4 = g, ascending: the
// header's order), two exchanges across the four lanes of a row, the finish, the handle's chain, the clip.  Lane 16 g + i then
// holds row i x columns 4 g .. 4 g + 3, as vk_table_kernel's lanes do.  Vocabulary rows past V and columns past len_t stay ZERO: a
// distance to a row of padding is not zero, 1 - x of it can be positive, and the epilogues' maxima count on zeros there.
// FORM: vk_host::SIM_SRC_*.  No array is indexed by a run-time value: nothing goes to scratch.
template <int FORM>
__global__ __launch_bounds__(256) void vk_source_table_kernel(const uint8_t *__restrict__ raw_tiles, int32_t n_tiles, int32_t raw_tile_bytes, int32_t d,
	const float *__restrict__ q_rows, const float *__restrict__ q_abs_sums, float *__restrict__ table, int32_t len_t, int32_t V,
	const float p_arg, const vk_host::sim_ops ops) {
	extern __shared__ float4 vk_src_qlds[];
	const int nb = raw_tile_bytes >> 10;
	for (int idx = threadIdx.x; idx < nb * 64; idx += 256) {
		const int b = idx >> 6, g = (idx >> 4) & 3, j = idx & 15;
		float v[4];
#pragma unroll
		for (int e = 0; e < 4; e++) {
			const int k = 16 * b + 4 * e + g;
			v[e] = (j < len_t && k < d) ? q_rows[(int64_t)j * d + k] : 0.0f;
		}
		vk_src_qlds[idx] = make_float4(v[0], v[1], v[2], v[3]);
	}
	__syncthreads();
	const int lane = threadIdx.x & 63;
	const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (tile >= n_tiles) return;
	const int i = lane & 15, g = lane >> 4;
	const uint8_t *__restrict__ tp = raw_tiles + (int64_t)tile * raw_tile_bytes;
	double acc[16];
#pragma unroll
	for (int j = 0; j < 16; j++) acc[j] = 0.0;
	double abs_a = 0.0;
#pragma unroll 1
	for (int b = 0; b < nb; b++) {
		const float4 x4 = *reinterpret_cast<const float4 *>(tp + (int64_t)b * 1024 + lane * 16);
		const float x[4] = {x4.x, x4.y, x4.z, x4.w};
		if constexpr (FORM == vk_host::SIM_SRC_SQRT_COS) {
#pragma unroll
			for (int e = 0; e < 4; e++) abs_a += (double)fabsf(x[e]);
		}
#pragma unroll
		for (int j = 0; j < 16; j++) {
			if (j < len_t) {   // (uniform)
				const float4 q4 = vk_src_qlds[(4 * b + g) * 16 + j];
				const float q[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
				for (int e = 0; e < 4; e++) acc[j] += (double)vk_host::sim_src_term<FORM>(x[e], q[e], p_arg);
			}
		}
	}
	// (s0 + s1) + (s2 + s3) across the lanes i, 16 + i, 32 + i, 48 + i: an IEEE sum does not depend on the order of its two operands
	float sum_a = 0.0f;
	if constexpr (FORM == vk_host::SIM_SRC_SQRT_COS) {
		abs_a += __shfl_xor(abs_a, 16, 64);
		abs_a += __shfl_xor(abs_a, 32, 64);
		sum_a = (float)abs_a;
	}
	const bool word = tile * 16 + i < V;
	float cell[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
	for (int j = 0; j < 16; j++) {
		if (j < len_t) {
			double s = acc[j];
			s += __shfl_xor(s, 16, 64);
			s += __shfl_xor(s, 32, 64);
			if ((j >> 2) == g) {   // this lane's four columns: the finish, the chain, the clip
				float v = vk_host::sim_src_finish<FORM>((float)s, p_arg, sum_a, FORM == vk_host::SIM_SRC_SQRT_COS ? q_abs_sums[j] : 0.0f);
				if (ops.n > 0) v = vk_host::sim_ops_apply(v, ops);
				cell[j & 3] = word ? clip01(v) : 0.0f;
			}
		}
	}
	*reinterpret_cast<float4 *>(table + ((int64_t)tile * 16 + i) * 16 + g * 4) = make_float4(cell[0], cell[1], cell[2], cell[3]);
}

// sim[id(t_j)][j] = 1 (metric/static.cpp:58-67); runs after vk_table_kernel
__global__ void vk_table_fix_kernel(float *__restrict__ table, const int32_t *__restrict__ q_ids, int32_t len_t, int32_t V) {
	const int j = threadIdx.x;
	if (j < len_t) {
		const int id = q_ids[j];
		if (id >= 0 && id < V) table[(int64_t)id * 16 + j] = 1.0f;
	}
}

extern "C" hipError_t vk_launch_pack(const void *in, int32_t dtype_bf16, int64_t n_rows, int32_t d, int32_t d_pad, int64_t row0,
	uint8_t *tiles, float *mag_out, int32_t normalize, int32_t prec, hipStream_t stream) {
	if (n_rows <= 0) return hipSuccess;
	const unsigned grid = (unsigned)((n_rows + 3) / 4);
	if (dtype_bf16)
		vk_pack_rows_kernel<uint16_t><<<grid, 256, 0, stream>>>((const uint16_t *)in, n_rows, d, d_pad, row0, tiles, mag_out, normalize, prec);
	else
		vk_pack_rows_kernel<float><<<grid, 256, 0, stream>>>((const float *)in, n_rows, d, d_pad, row0, tiles, mag_out, normalize, prec);
	return hipGetLastError();
}

extern "C" hipError_t vk_launch_table_fix(float *table, const int32_t *q_ids, int32_t len_t, int32_t V, hipStream_t stream) {
	vk_table_fix_kernel<<<1, 64, 0, stream>>>(table, q_ids, len_t, V);
	return hipGetLastError();
}

extern "C" hipError_t vk_launch_table(const uint8_t *etiles, const uint8_t *qtile, int32_t n_tiles, int32_t nk32, int32_t tail,
	int32_t tile_bytes, float *table, const int32_t *q_ids, int32_t len_t, int32_t V, int32_t prec, const vk_host::sim_ops *ops,
	const VkSimSrcArgs *src, hipStream_t stream) {
	const vk_host::sim_ops chain = ops ? *ops : vk_host::sim_ops{};
	if (src && src->src.kind != VK_SIMSRC_COSINE) {
		// the query tile's rows in LDS: 64 bytes per feature (d rounded up to 16), at most 64 KiB (vk_host::kSimSrcMaxD)
		if (!src->raw_tiles || !src->q_rows || !src->q_abs_sums || src->d < 1 || src->d > vk_host::kSimSrcMaxD || src->raw_tile_bytes != (src->d + 15) / 16 * 1024 ||
			len_t < 1 || len_t > 16) return hipErrorInvalidValue;
		const unsigned grid = (unsigned)((n_tiles + 3) / 4);
		const size_t lds = (size_t)src->raw_tile_bytes;
#define VK_SRC_TABLE(FORM) vk_source_table_kernel<FORM><<<grid, 256, lds, stream>>>(src->raw_tiles, n_tiles, src->raw_tile_bytes, src->d, src->q_rows, \
	src->q_abs_sums, table, len_t, V, src->src.arg, chain)
		switch (vk_host::sim_src_form(src->src)) {
		case vk_host::SIM_SRC_P1: VK_SRC_TABLE(vk_host::SIM_SRC_P1); break;
		case vk_host::SIM_SRC_P2: VK_SRC_TABLE(vk_host::SIM_SRC_P2); break;
		case vk_host::SIM_SRC_PGEN: VK_SRC_TABLE(vk_host::SIM_SRC_PGEN); break;
		default: VK_SRC_TABLE(vk_host::SIM_SRC_SQRT_COS); break;
		}
#undef VK_SRC_TABLE
	}
	else if (chain.n > 0) vk_table_kernel<true><<<(n_tiles + 3) / 4, 256, 0, stream>>>(etiles, qtile, n_tiles, nk32, tail, tile_bytes, table, prec, len_t, V, chain);
	else vk_table_kernel<false><<<(n_tiles + 3) / 4, 256, 0, stream>>>(etiles, qtile, n_tiles, nk32, tail, tile_bytes, table, prec, len_t, V, vk_host::sim_ops{});
	if (q_ids) vk_table_fix_kernel<<<1, 64, 0, stream>>>(table, q_ids, len_t, V);
	return hipGetLastError();
}
