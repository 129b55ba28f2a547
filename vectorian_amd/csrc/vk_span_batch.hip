// vk_span_batch.hip -- a batch of one-token queries against the one-token slices of a span corpus.
// vk_span_kernel (vk_score.hip) runs one MFMA chain per 16 spans and keeps column 0 of the result; here the query tile holds 16
// different queries and all 16 columns are kept: one pass over the span tiles serves every query a workgroup has staged in LDS.
// Geometry (queries per LDS fill, the grid): vk_span_batch_host.h.
#include "vk_common.hip.h"
#include "vk_span_batch_host.h"

namespace {

constexpr int kTiles = vk_host::kSpanBatchTilesPerWave, kRun = vk_host::kSpanBatchRun, kThreads = vk_host::kSpanBatchThreads;
constexpr int kChunk = 4;   // K-blocks of both span tiles loaded ahead of their MFMAs: 8 KiB per wave in flight
static_assert(kTiles == 2, "the kernel body names its two span tiles");

// one K-block (1 KiB: 16 bytes per lane) of a query tile against the same block of a span tile, added to the chain -- the
// instruction(s) sim_tile / sim_tile_generic issue for that block
template <int PREC>
__device__ __forceinline__ f32x4 mma_block(const f32x4 q, const f32x4 x, f32x4 acc) {
	if constexpr (PREC) {
#pragma unroll
		for (int e = 0; e < 4; e++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q[e], x[e], acc, 0, 0, 0);
		return acc;
	} else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, q), __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
}

__device__ __forceinline__ f32x4 load_block(const uint8_t *__restrict__ tile, int t, int lane) {
	return __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(tile + t * 1024 + lane * 16));
}

}   // namespace

// NK > 0: the K-blocks of a tile known at compile time (bf16: steps of 32 features, the last one half filled when TAIL; fp32: blocks
// of 16 features); NK = 0: p.nk32 / p.tail.  QT: query tiles of 16 queries a workgroup stages (tiles past the launch's last: zeros).
// A wave takes runs of kRun pairs of span tiles; per K-block it reads each staged query fragment once (ds_read_b128) and issues the
// block's MFMAs for both span tiles: one accumulator chain from zero per (query tile, span tile), K ascending.
template <int NK, bool TAIL, int PREC, int QT>
__global__ __launch_bounds__(kThreads) void vk_span_batch_kernel(VkSpanBatchParams p) {
	extern __shared__ __attribute__((aligned(16))) uint8_t qlds[];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int tile_bytes = p.tile_bytes;
	const int qt0 = blockIdx.y * p.fill_tiles, n_here = min(p.fill_tiles, p.n_qtiles - qt0);   // (fill_tiles <= QT: the launcher)
	const int row_end = min(p.n_queries, (qt0 + n_here) * 16);   // rows of the matrix this workgroup writes end here
	{   // this workgroup's query tiles into LDS, 16 bytes per thread and step (tile_bytes is a multiple of 512)
		const int have = n_here * tile_bytes, all = QT * tile_bytes;
		const uint8_t *src = p.qtiles + (size_t)qt0 * tile_bytes;
		const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
		for (int o = threadIdx.x * 16; o < all; o += kThreads * 16)
			*reinterpret_cast<f32x4 *>(qlds + o) = o < have ? *reinterpret_cast<const f32x4 *>(src + o) : zero;
	}
	__syncthreads();
	const int nk = NK > 0 ? NK : p.nk32;
	const bool tail = PREC == 0 && (NK > 0 ? TAIL : p.tail != 0);
	const int nfull = tail ? nk - 1 : nk;
	const int64_t n_pairs = (p.n_tiles + kTiles - 1) / kTiles;
	const uint32_t n_pad = (uint32_t)p.n_pad;
	const int row0 = qt0 * 16 + 4 * (lane >> 4);   // the first of this lane's four queries of query tile 0
	for (int64_t run = (int64_t)blockIdx.x * (kThreads / 64) + wv; run * kRun < n_pairs; run += (int64_t)gridDim.x * (kThreads / 64))
	for (int64_t pair = run * kRun; pair < (run + 1) * kRun && pair < n_pairs; pair++) {
		const int64_t tile_a = pair * kTiles;
		const bool two = tile_a + 1 < p.n_tiles;   // (the corpus's last tile alone: its block is read twice, one result dropped)
		const uint8_t *ta = p.tiles + tile_a * tile_bytes, *tb = two ? ta + tile_bytes : ta;
		f32x4 acc[QT][kTiles];
#pragma unroll
		for (int qt = 0; qt < QT; qt++) {
			acc[qt][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
			acc[qt][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
		}
		const auto blocks = [&](const int t) {   // kChunk whole K-blocks from t on
			f32x4 xa[kChunk], xb[kChunk];
#pragma unroll
			for (int i = 0; i < kChunk; i++) { xa[i] = load_block(ta, t + i, lane); xb[i] = load_block(tb, t + i, lane); }
			__builtin_amdgcn_sched_barrier(0);   // the loads stay in front of their MFMAs
#pragma unroll
			for (int i = 0; i < kChunk; i++) {
#pragma unroll
				for (int qt = 0; qt < QT; qt++) {
					const f32x4 q = *reinterpret_cast<const f32x4 *>(qlds + qt * tile_bytes + (t + i) * 1024 + lane * 16);
					acc[qt][0] = mma_block<PREC>(q, xa[i], acc[qt][0]);
					acc[qt][1] = mma_block<PREC>(q, xb[i], acc[qt][1]);
				}
			}
		};
		const auto block = [&](const int t) {
			const f32x4 xa = load_block(ta, t, lane), xb = load_block(tb, t, lane);
#pragma unroll
			for (int qt = 0; qt < QT; qt++) {
				const f32x4 q = *reinterpret_cast<const f32x4 *>(qlds + qt * tile_bytes + t * 1024 + lane * 16);
				acc[qt][0] = mma_block<PREC>(q, xa, acc[qt][0]);
				acc[qt][1] = mma_block<PREC>(q, xb, acc[qt][1]);
			}
		};
		if constexpr (NK > 0) {
			constexpr int NFULL = TAIL ? NK - 1 : NK;
#pragma unroll
			for (int c = 0; c < NFULL / kChunk; c++) blocks(c * kChunk);
#pragma unroll
			for (int t = NFULL / kChunk * kChunk; t < NFULL; t++) block(t);
		} else {
			int t = 0;
			for (; t + kChunk <= nfull; t += kChunk) blocks(t);
			for (; t < nfull; t++) block(t);
		}
		if (tail) {   // the half block: 32 x 16 bytes, the upper lanes contribute zeros on both sides (load_half_block)
			const bf16x8 xa = load_half_block(ta + nfull * 1024, lane, true), xb = load_half_block(tb + nfull * 1024, lane, true);
			const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
			for (int qt = 0; qt < QT; qt++) {
				bf16x8 q = *reinterpret_cast<const bf16x8 *>(qlds + qt * tile_bytes + nfull * 1024 + (lane & 31) * 16);
				q = lane < 32 ? q : z;
				acc[qt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q, xa, acc[qt][0], 0, 0, 0);
				acc[qt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q, xb, acc[qt][1], 0, 0, 0);
			}
		}
		// lane l holds S[span l & 15][query 4 (l >> 4) + r] of each (query tile, span tile): stored as matrix[query][span], 64 bytes
		// per query and span tile.  The cell's index fits 32 bits (vk_span_batch_host.h).
		const uint32_t col = (uint32_t)(tile_a * 16) + (uint32_t)(lane & 15);
#pragma unroll
		for (int qt = 0; qt < QT; qt++) {
#pragma unroll
			for (int r = 0; r < 4; r++) {
				const int row = row0 + qt * 16 + r;
				if (row >= row_end) continue;
				const uint32_t at = (uint32_t)row * n_pad + col;
				p.matrix[at] = clip01(acc[qt][0][r]);
				if (two) p.matrix[at + 16] = clip01(acc[qt][1][r]);
			}
		}
	}
}

template <int NK, bool TAIL, int PREC, int QT>
static hipError_t launch_qt(const VkSpanBatchParams &p, hipStream_t stream) {
	int dev = 0, cus = 256;
	if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
	const size_t smem = vk_host::span_batch_lds_bytes(p.tile_bytes, QT);
	if (smem > vk_host::kSpanBatchLdsBudget) return hipErrorInvalidValue;
	const auto kernel = vk_span_batch_kernel<NK, TAIL, PREC, QT>;
	if (smem > 64 * 1024) {
		const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
		if (e != hipSuccess) return e;
	}
	const dim3 grid((unsigned)vk_host::span_batch_grid(p.n_tiles * 16, cus), (unsigned)((p.n_qtiles + p.fill_tiles - 1) / p.fill_tiles));
	kernel<<<grid, kThreads, smem, stream>>>(p);
	return hipGetLastError();
}

template <int NK, bool TAIL, int PREC>
static hipError_t launch_form(const VkSpanBatchParams &p, hipStream_t stream) {
	switch (vk_host::span_batch_form_tiles(p.fill_tiles)) {
	case 1: return launch_qt<NK, TAIL, PREC, 1>(p, stream);
	case 2: return launch_qt<NK, TAIL, PREC, 2>(p, stream);
	case 4: return launch_qt<NK, TAIL, PREC, 4>(p, stream);
	case 6: return launch_qt<NK, TAIL, PREC, 6>(p, stream);
	default: return launch_qt<NK, TAIL, PREC, 8>(p, stream);
	}
}

// p->fill_tiles: the query tiles per workgroup of this launch, at most vk_host::span_batch_fill_tiles(tile_bytes) and p->n_qtiles
extern "C" hipError_t vk_launch_span_batch(const VkSpanBatchParams *pp, hipStream_t stream) {
	const VkSpanBatchParams &p = *pp;
	if (p.n_tiles < 1 || p.n_qtiles < 1 || p.fill_tiles < 1 || p.fill_tiles > vk_host::span_batch_fill_tiles(p.tile_bytes) ||
		p.n_pad != p.n_tiles * 16 || !vk_host::span_batch_index_fits_u32(p.n_pad, p.n_queries)) return hipErrorInvalidValue;
	// the widths vk_launch_span specialises, and the 300-d fp32 rows of vk_score_m4
	if (p.prec) return p.nk32 == 19 ? launch_form<19, false, 1>(p, stream) : launch_form<0, false, 1>(p, stream);
	if (p.nk32 == 10 && p.tail == 1) return launch_form<10, true, 0>(p, stream);
	if (p.nk32 == 12 && p.tail == 0) return launch_form<12, false, 0>(p, stream);
	if (p.nk32 == 24 && p.tail == 0) return launch_form<24, false, 0>(p, stream);
	if (p.nk32 == 32 && p.tail == 0) return launch_form<32, false, 0>(p, stream);
	return launch_form<0, false, 0>(p, stream);
}
