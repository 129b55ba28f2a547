// vk_mix.hip -- token similarity combinators over the static layout (vk_corpus_set_sim_mix): the per-query table of a
// cosine operand in the canonical arithmetic, and the combination of the operands' tables into the handle's table.
#include "vk_common.hip.h"
#include "vk_sim_mix_host.h" // the combination of one cell (host and device)

// The per-query table [V_pad x 16] of a cosine operand of a mixed handle.  The handle's table is what every restatement site reads
// (static_table_cell), and the tests hold the winners against the oracle's arithmetic with ==: the cosine of a cell is therefore the
// canonical one -- sim_canon16's four double sums -- not the matrix pipe's sum of vk_table_kernel.  One wave takes the 16
// vocabulary rows of a tile x the 16 columns of the query tile, staged through its own VK_CANON_LDS bytes; lane 16 g + i holds row i x
// columns 4 g .. 4 g + 3, as vk_table_kernel's lanes do.  Then the operand's chain on the cells of the V rows x the len_t columns and
// the clip (static_cell); the padding of either side holds zero rows, whose cosine is 0.  vk_table_fix_kernel runs after it.
__global__ __launch_bounds__(256) void vk_canon_table_kernel(const uint8_t *__restrict__ etiles, const uint8_t *__restrict__ qtile,
	int32_t n_tiles, int32_t nk32, int32_t tail, int32_t tile_bytes, int32_t d, float *__restrict__ table, int32_t prec, int32_t len_t, int32_t V,
	const vk_host::sim_ops ops) {
	__shared__ float4 canon4[4 * VK_CANON_LDS / 16];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int tile = blockIdx.x * 4 + wave;
	if (tile >= n_tiles) return;   // (no workgroup barrier below: a wave's staging is its own)
	uint8_t *canon = reinterpret_cast<uint8_t *>(canon4) + wave * VK_CANON_LDS;
	float val[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	sim_canon16(canon_row_ptr(etiles + (int64_t)tile * tile_bytes, lane), qtile, nk32, tail, d, prec, canon, lane, val);
	const bool word = tile * 16 + (lane & 15) < V;
	const int cb = (lane >> 4) * 4;
#pragma unroll
	for (int r = 0; r < 4; r++) val[r] = static_cell(val[r], false, word && cb + r < len_t, ops);
	*reinterpret_cast<float4 *>(table + ((int64_t)tile * 16 + (lane & 15)) * 16 + cb) = make_float4(val[0], val[1], val[2], val[3]);
}

// The handle's table from its operands' tables, cell by cell (vk_host::sim_mix_cell): one 16-byte load per operand and one 16-byte
// store per thread.  No mask for the padding: every operand's is 0 there, and both combinators map zeros to zero.  in[0] may be
// `out` (no __restrict__): a thread reads its four cells of every operand before it writes them.
__global__ __launch_bounds__(256) void vk_table_mix_kernel(const VkMixArgs a) {
	const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
	if (i >= a.n_cells) return;
	float4 x[VK_MAX_SIM_OPERANDS];
#pragma unroll
	for (int m = 0; m < VK_MAX_SIM_OPERANDS; m++)
		x[m] = m < a.mix.n ? *reinterpret_cast<const float4 *>(a.in[m] + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	float cx[VK_MAX_SIM_OPERANDS], cy[VK_MAX_SIM_OPERANDS], cz[VK_MAX_SIM_OPERANDS], cw[VK_MAX_SIM_OPERANDS];
#pragma unroll
	for (int m = 0; m < VK_MAX_SIM_OPERANDS; m++) { cx[m] = x[m].x; cy[m] = x[m].y; cz[m] = x[m].z; cw[m] = x[m].w; }
	*reinterpret_cast<float4 *>(a.out + i) = make_float4(vk_host::sim_mix_cell(cx, a.mix), vk_host::sim_mix_cell(cy, a.mix),
		vk_host::sim_mix_cell(cz, a.mix), vk_host::sim_mix_cell(cw, a.mix));
}

extern "C" hipError_t vk_launch_canon_table(const uint8_t *etiles, const uint8_t *qtile, int32_t n_tiles, int32_t nk32, int32_t tail,
	int32_t tile_bytes, int32_t d, float *table, const int32_t *q_ids, int32_t len_t, int32_t V, int32_t prec, const vk_host::sim_ops *ops,
	hipStream_t stream) {
	if (n_tiles < 1 || len_t < 1 || len_t > 16) return hipErrorInvalidValue;
	vk_canon_table_kernel<<<(n_tiles + 3) / 4, 256, 0, stream>>>(etiles, qtile, n_tiles, nk32, tail, tile_bytes, d, table, prec, len_t, V,
		ops ? *ops : vk_host::sim_ops{});
	if (q_ids) return vk_launch_table_fix(table, q_ids, len_t, V, stream);
	return hipGetLastError();
}

extern "C" hipError_t vk_launch_table_mix(const VkMixArgs *a, hipStream_t stream) {
	if (a->mix.n < 2 || a->mix.n > VK_MAX_SIM_OPERANDS || a->n_cells < 4 || a->n_cells % 4 != 0) return hipErrorInvalidValue;
	for (int m = 0; m < a->mix.n; m++) if (!a->in[m]) return hipErrorInvalidValue;
	vk_table_mix_kernel<<<(unsigned)((a->n_cells / 4 + 255) / 256), 256, 0, stream>>>(*a);
	return hipGetLastError();
}
