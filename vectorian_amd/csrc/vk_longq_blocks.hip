// vk_longq_blocks.hip -- alignments of queries of 65 .. 512 tokens over slices of 65 .. 512 tokens: the block form of vk_longq_kernel
// (vk_longq.hip: the sweep, the strip, the order of candidates, the traceback -- read that file first).
#include "vk_longq.hip.h"

// The block form: slices of up to VK_DEV_MAX_LONG_LEN (512) tokens.  Still one wave per slice; the slice's columns go by in
// blocks of 64 tokens, block b = slice tokens 64 b + 1 .. 64 b + 64, each block the sweep of vk_longq_kernel over all the query's
// tokens with a strip of its own.  What links block b to block b - 1 is one column: the lane of u = 64 b stores H[64 b][v] (affine
// gaps: E[64 b][v] too) for every v while its block runs, and in block b that column is lane 0's `border` in lane_up where block 0
// has the DP's border row.  Two such columns in LDS behind the strip, read and written in turn.  The matrix of general gaps, the
// cells' records and the unmodified similarities have rows of the slice's length rounded up to 64 and live in the scratch region;
// the gap-over-s scan walks k = 1 .. u across the blocks.  The scoring pass walks p.order (the rows of more than 64 tokens, longest
// first) and overwrites the -inf vk_longq_kernel left there; the tracebacks take winners of any length (a short one is a single
// block); the start cell stays the first maximum in row-major order: an earlier block holds the smaller u, a later one replaces on
// strictly greater only.
// A kernel and a unit of its own, the fills and the sweep restated: as a template flag of vk_longq_kernel, with the fills as device
// functions of both, or merely as a second kernel in that unit, it changed vk_longq_kernel's code (inlining, register allocation,
// schedule); timed as a template flag, 200,000 slices of at most 64 tokens took 2 - 5 % longer than on the commit before
// (profiles/long_query_mixed.jsonl, "run": "flag_*").  The pass over such slices stays as it was, to the instruction.
template <bool FLOW, int GAP>
__global__ __launch_bounds__(64) void vk_longq_blocks_kernel(VkLongqParams p) {
	extern __shared__ float4 vk_smem4[];
	uint8_t *canon = reinterpret_cast<uint8_t *>(vk_smem4);
	float *Sl = reinterpret_cast<float *>(canon + (FLOW ? VK_CANON_LDS : 0));   // [lt_pad][64]: S[v - 1][u - u0 - 1] of the block the DP runs on
	const int lane = threadIdx.x;
	const int LT = p.len_t, SW = p.s_stride;
	uint8_t *region = p.scratch ? p.scratch + (int64_t)blockIdx.x * p.scratch_stride : nullptr;
	// the scratch region: the host's carve-up (vk_host::longq_geometry_of), sized for the corpus's longest slice
	float *Hm = reinterpret_cast<float *>(region);                     // GAP 2: H[v][u - 1], v = 0 .. LT, rows of LS floats
	int16_t *Dm = reinterpret_cast<int16_t *>(region + p.dm_off);      // FLOW: the cells' records, rows of LS
	float *Su = reinterpret_cast<float *>(region + p.su_off);          // FLOW: the unmodified similarities of ALL blocks, rows of LS (the walk back crosses blocks whose strips are gone)
	float *colbuf = Sl + (size_t)((LT + 15) / 16 * 16) * SW;          // two border columns of CB floats behind the strip
	const int CB = (GAP == 1 ? 2 : 1) * (LT + 1);
	const bool is_static = p.layout == VK_DEV_LAYOUT_STATIC;
	const bool local = p.locality == VK_DEV_LOCAL, global = p.locality == VK_DEV_GLOBAL;
	const float gs = p.gs, gt = p.gt, a_s = p.a_s, a_t = p.a_t, open_s = p.open_s, open_t = p.open_t;

	const int64_t n_items = FLOW ? (int64_t)p.n_keys : (int64_t)p.n_order;
	for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
		int64_t g = item;
		if (FLOW) {
			const uint64_t key = p.keys[item];
			if (key == 0) continue;   // fewer than k admitted
			g = (int64_t)(uint32_t)(key & 0xffffffffu);
		} else g = (int64_t)p.order[item];
		const int t_a = p.sent_start[g], t_b = p.sent_end[g];
		const int len_s = t_b - t_a;
		if (len_s < 1 || len_s > VK_DEV_MAX_LONG_LEN) {   // (longer slices: refused by the host before the launch; empty ones carry no score)
			if (!FLOW && lane == 0) { p.scores[g] = VK_NEG_INF; if (p.raw) p.raw[g] = VK_NEG_INF; }
			continue;
		}
		const int LS = (len_s + 63) / 64 * 64;   // columns per row of the matrix, the records and the unmodified similarities
		const int n_blocks = LS / 64;

		auto border_s = [&](int k) -> float {   // H[k][0]
			if (!global || k == 0) return 0.0f;
			return GAP == 0 ? -(gs * (float)k) : GAP == 1 ? -(a_s + gs * (float)k) : -p.ws[k];
		};
		auto border_t = [&](int k) -> float {   // H[0][k]
			if (!global || k <= 0) return 0.0f;
			return GAP == 0 ? -(gt * (float)k) : GAP == 1 ? -(a_t + gt * (float)k) : -p.wt[k];
		};
		float raw = 0.0f;     // the aligner score, and where the traceback starts: first maximum in row-major order = smallest u, then smallest v
		int su = 0, sv = 0;
#pragma unroll 1
		for (int blk = 0; blk < n_blocks; blk++) {
			const int u0 = 64 * blk;                                    // slice tokens before this block
			const int cnt = len_s - u0 < 64 ? len_s - u0 : 64;          // ... in it
			const int u = u0 + lane + 1;
			const bool ucol = u <= len_s;
			const float *col_in = colbuf + (blk & 1) * CB;              // H[u0][v] (and E[u0][v] at LT + 1 + v), v = 0 .. LT
			float *col_out = colbuf + ((blk + 1) & 1) * CB;             // ... H[u0 + 64][v], written by lane 63 for the next block
			const bool hand_on = lane == 63 && blk + 1 < n_blocks;

			// ---- similarities of the block's tokens (a whole slice of at most 64 tokens, or one column block): Sl[(v - 1) * SW + (u - u0 - 1)]
			const int t0 = t_a + u0, t1 = t0 + cnt;
			if constexpr (FLOW) {
				for (int rb = 0; rb * 16 < cnt; rb++) {
					const int rel = rb * 16 + (lane & 15);
					const int tok = t0 + (rel < cnt ? rel : 0);   // (past the slice's end its first token again, never read)
					const int id = is_static ? p.tok_id[tok] : 0;
					const uint8_t *xrow = is_static ? canon_row_ptr_static(p.tiles, p.tile_bytes, id) : p.tiles + (int64_t)(tok >> 4) * p.tile_bytes + (tok & 15) * 16;
					const int ps = p.pos_s ? p.pos_s[tok] : 0;
#pragma unroll 1
					for (int b = 0; b < p.nq; b++) {
						float val[4] = {0.0f, 0.0f, 0.0f, 0.0f};
						if (!(is_static && p.sim_src))   // (not the cosine: static_cell takes the table's cell)
							sim_canon16(xrow, p.qtile + (int64_t)b * p.tile_bytes, p.nk32, p.tail, p.d, p.prec, canon, lane, val);
						const int c0 = 16 * b + (lane >> 4) * 4;
#pragma unroll
						for (int r = 0; r < 4; r++) {
							float x = is_static ? static_cell(val[r], p.q_ids && p.q_ids[c0 + r] == id, c0 + r < p.len_t, p.sim_ops, p.sim_src, p.table, p.table_stride, id, c0 + r) : vk_host::contextual_cell(val[r], c0 + r < p.len_t, p.sim_ops);   // chain, sim[id(t_j)][j] = 1 (metric/static.cpp:46-67), clip
							if (rel < cnt && c0 + r < LT) Su[(c0 + r) * LS + u0 + rel] = x;
							if (p.pos_s) x = tag_weighted(x, p.tw[c0 + r], ps, p.tpos[c0 + r], p.tw_keep, p.tw_threshold);
							if (rel < cnt) Sl[(c0 + r) * SW + rel] = x;
						}
					}
				}
			} else if (is_static) {
				const int id = ucol ? p.tok_id[t0 + lane] : 0;
				const int ps = (p.pos_s && ucol) ? p.pos_s[t0 + lane] : 0;
				for (int b = 0; b < p.nq; b++) {
					const float *row = p.table + (int64_t)b * p.table_stride + (int64_t)id * 16;
					float4 x[4];
#pragma unroll
					for (int j = 0; j < 4; j++) x[j] = *reinterpret_cast<const float4 *>(row + 4 * j);
#pragma unroll
					for (int j = 0; j < 4; j++) {
						const float e[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
#pragma unroll
						for (int r = 0; r < 4; r++) {
							const int c = 16 * b + 4 * j + r;
							float y = e[r];
							if (p.pos_s) y = tag_weighted(y, p.tw[c], ps, p.tpos[c], p.tw_keep, p.tw_threshold);
							if (ucol) Sl[c * SW + lane] = y;
						}
					}
				}
			} else {
				const int tile0 = t0 >> 4, off = t0 - tile0 * 16, ntiles = ((t1 + 15) >> 4) - tile0;
				if (p.prec == 0 && p.nk32 == 10 && p.tail == 1) {
					for (int j0 = 0; j0 < ntiles; j0 += 3) {
						QFrag<10, true> tf[3];
#pragma unroll
						for (int jj = 0; jj < 3; jj++)   // (past the slice's last tile: that tile again, its columns fall outside the slice and are dropped)
							load_qfrag(tf[jj], p.tiles + (int64_t)(tile0 + (j0 + jj < ntiles ? j0 + jj : ntiles - 1)) * p.tile_bytes, lane);
						for (int b = 0; b < p.nq; b++) {
							const int vq = 16 * b + (lane & 15);
#pragma unroll
							for (int jj = 0; jj < 3; jj++) {
								if (j0 + jj >= ntiles) break;
								const f32x4 acc = longq_sim_tile(tf[jj], p.qtile + (int64_t)b * p.tile_bytes, lane);
#pragma unroll
								for (int r = 0; r < 4; r++) {
									const int c = 16 * (j0 + jj) + 4 * (lane >> 4) + r - off;
									if (c >= 0 && c < cnt) {
										float y = acc[r];
										if (p.pos_s) y = tag_weighted(y, p.tw[vq], p.pos_s[t0 + c], p.tpos[vq], p.tw_keep, p.tw_threshold);
										Sl[vq * SW + c] = y;
									}
								}
							}
						}
					}
				} else
				for (int b = 0; b < p.nq; b++) {
					const int vq = 16 * b + (lane & 15);   // this lane's query token (0-based)
					for (int j = 0; j < ntiles; j++) {
						// A = the token tile, B = the query tile: lane l holds S[query row l & 15][token 4 (l >> 4) + r of the tile]
						const f32x4 acc = sim_tile_generic(p.tiles + (int64_t)(tile0 + j) * p.tile_bytes, p.qtile + (int64_t)b * p.tile_bytes, p.nk32, p.tail, lane, p.prec);
#pragma unroll
						for (int r = 0; r < 4; r++) {
							const int c = 16 * j + 4 * (lane >> 4) + r - off;   // column of the slice
							if (c >= 0 && c < cnt) {
								float y = acc[r];
								if (p.pos_s) y = tag_weighted(y, p.tw[vq], p.pos_s[t0 + c], p.tpos[vq], p.tw_keep, p.tw_threshold);
								Sl[vq * SW + c] = y;
							}
						}
					}
				}
			}
			wave_lds_fence();

			// ---- the sweep.  a1 = H[u][v - 1] of this lane's row (borders included), prev_up = H[u - 1][v - 1]; e1 / f1: the affine solver's states
			float a1 = border_s(u);
			float prev_up = border_s(u0);   // H[u - 1][v - 1]: what `up` was one step ago (step 2: H[u0][0]; H[0][0] = 0)
			float e1 = VK_NEG_INF, f1 = VK_NEG_INF;
			float tail_max = VK_NEG_INF;   // general gaps, scoring pass: max of H[u][v'] over v' <= v - tail (see the scan below)
			float best_v = 0.0f;          // LOCAL / SEMIGLOBAL: this row's best cell, first v among equals (borders are 0: "borders first")
			int best_at = 0;
			// (general gaps: row 0 and column 0 of the matrix are not stored -- the scans below take the borders from border_t / border_s)
			const int steps_end = cnt + LT;
			for (int dg = 2; dg <= steps_end; dg++) {
				const int v = dg - (lane + 1);
				const bool act = ucol && v >= 1 && v <= LT;
				float edge_h = border_t(dg - 1), edge_e = VK_NEG_INF;    // lane 0's H[u - 1][v], E[u - 1][v]: the border row, or the column block b - 1 left
				if (blk > 0) {
					const int vb = dg - 1 < LT ? dg - 1 : LT;
					edge_h = col_in[vb];
					if (GAP == 1) edge_e = col_in[LT + 1 + vb];
				}
				const float up_h = lane_up(a1, edge_h);                  // H[u - 1][v] (lane 0: the border)
				const float dg_h = prev_up;                              // H[u - 1][v - 1] = H[u - 1][v] of the step before
				prev_up = up_h;
				float up_e = VK_NEG_INF;
				if (GAP == 1) up_e = lane_up(e1, edge_e);                // E[u - 1][v]
				const float s = act ? Sl[(v - 1) * SW + lane] : 0.0f;
				float best, e = VK_NEG_INF, f = VK_NEG_INF;
				int dir = LQ_DIAG, kk = 0, ee = 0, fe = 0;
				{
					const float c = dg_h + s;
					if (local) { best = 0.0f; dir = LQ_STOP; if (c > best) { best = c; dir = LQ_DIAG; } }
					else best = c;
				}
				if (GAP == 0) {
					float c = up_h - gs;
					if (c > best) { best = c; dir = LQ_UP; }
					c = a1 - gt;
					if (c > best) { best = c; dir = LQ_LEFT; }
				} else if (GAP == 1) {
					// gap of length 1 (open) first, longer (extend) only if strictly greater (align_affine)
					e = up_h - open_s;
					float c = up_e - gs;
					if (c > e) { e = c; ee = 1; }
					f = a1 - open_t;
					c = f1 - gt;
					if (c > f) { f = c; fe = 1; }
					if (e > best) { best = e; dir = LQ_UP; }
					if (f > best) { best = f; dir = LQ_LEFT; }
				} else {
					// general gaps: H[u - k][v] - w_s(k), k = 1 .. u, then H[u][v - k] - w_t(k), k = 1 .. v (align_general); the trip counts are
					// the wave's (lanes beyond their own range sit out)
					// (eight candidates at a time: their loads first -- addresses clamped into the matrix, no loads under branches --, then the
					// compares in the oracle's order; one load per trip of a branchy loop waited out an LDS round trip per candidate)
					const int ku = u0 + cnt;   // (across the blocks before this one)
					const int vc = v < 1 ? 1 : v > LT ? LT : v;   // this lane's row of the matrix, clamped for the lanes that sit out
					for (int k0 = 1; k0 <= ku; k0 += 8) {
						float src[8];
#pragma unroll
						for (int i = 0; i < 8; i++) { const int l2 = u - 1 - (k0 + i); src[i] = Hm[vc * LS + (l2 < 0 ? 0 : l2)]; }
#pragma unroll
						for (int i = 0; i < 8; i++) {
							const int k = k0 + i;
							const float c = (k == u ? border_t(v) : src[i]) - p.ws[k < len_s ? k : len_s];
							if (act && k <= u && k <= ku && c > best) { best = c; dir = LQ_UP; kk = k; }
						}
					}
					// (scoring pass under a table that saturates -- w_t(k) = w_t(tail) for every k >= tail, exp5: from 126 on --: the candidates
					// further back than `tail` columns all cost the same and are ONE running maximum per lane, tail_max; the scan stops at tail - 1)
					const int tail = (!FLOW && p.wt_tail > 0) ? p.wt_tail : LT + 1;
					int kv = dg - 1 < LT ? dg - 1 : LT;
					if (kv > tail - 1) kv = tail - 1;
					for (int k0 = 1; k0 <= kv; k0 += 8) {
						float src[8];
#pragma unroll
						for (int i = 0; i < 8; i++) { const int r2 = vc - (k0 + i); src[i] = Hm[(r2 < 1 ? 1 : r2) * LS + u - 1]; }
#pragma unroll
						for (int i = 0; i < 8; i++) {
							const int k = k0 + i;
							const float c = (k == v ? border_s(u) : src[i]) - p.wt[k <= LT ? k : LT];
							if (act && k <= v && k <= kv && c > best) { best = c; dir = LQ_LEFT; kk = k; }
						}
					}
					if (!FLOW && p.wt_tail > 0 && act && v >= tail) {
						const float x = v == tail ? border_s(u) : Hm[(v - tail) * LS + u - 1];   // H[u][v - tail] joins the candidates that far back
						tail_max = fmaxf(tail_max, x);
						const float c = tail_max - p.wt[tail];
						if (c > best) { best = c; dir = LQ_LEFT; }
					}
				}
				if (act) {
					if (GAP == 2) Hm[v * LS + u - 1] = best;
					if (FLOW) Dm[v * LS + u - 1] = (int16_t)(dir | (ee << 2) | (fe << 3) | (kk << 4));
					if (hand_on) { col_out[v] = best; if (GAP == 1) col_out[LT + 1 + v] = e; }
					// start cell: LOCAL over all cells, SEMIGLOBAL over the last row and the last column (start_cell of the oracle)
					if (!global && (local || u == len_s || v == LT) && best > best_v) { best_v = best; best_at = v; }
					a1 = best;
					if (GAP == 1) { e1 = e; f1 = f; }
				}
				if (GAP == 2) {   // the row just stored is read by other lanes on later steps: same wave, in order; pin the compiler to it
					__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
					__builtin_amdgcn_wave_barrier();
					__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
				}
			}

			// ---- the aligner score (and where the traceback starts): first maximum in row-major order = smallest u, then smallest v
			// (block form: an earlier block holds the smaller u -- a later one replaces on strictly greater only)
			if (global) {
				raw = __shfl(a1, len_s - 1 - u0, 64);   // H[len_s][len_t] (block form: the last block's)
				su = len_s; sv = LT;
			} else {
				float m = ucol ? best_v : 0.0f;
#pragma unroll
				for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
				const unsigned long long hit = __ballot(ucol && best_v == m && m > 0.0f);
				if (hit && m > raw) {
					const int first = __builtin_ctzll(hit);
					raw = m;
					su = u0 + first + 1;
					sv = __shfl(best_at, first, 64);
				}
			}
			wave_lds_fence();   // the next block overwrites the strip, and reads the column this one wrote
		}
		if constexpr (!FLOW) {
			if (lane == 0) {
				const float boost = p.boost ? p.boost[g] : 1.0f;
				p.scores[g] = (raw / p.ref_total) * boost;   // Score::value with every query token's weight in the reference score (submatch_weight = 0)
				if (p.raw) p.raw[g] = raw;
			}
		} else {
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
			int16_t *map = p.mapping + (int64_t)item * p.out_stride;
			float *esim = p.edge_sim + (int64_t)item * p.out_stride;
			for (int j = lane; j < LT; j += 64) { map[j] = -1; esim[j] = 0.0f; }
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
			if (lane == 0) {
				p.raw_out[item] = raw;
				int cu = su, cv = sv, state = 0;   // state: 0 = H, 1 = E, 2 = F (the affine solver's walk)
				while (cu > 0 && cv > 0) {
					const int rec = (int)(uint16_t)Dm[cv * LS + (cu - 1)];
					const int d = rec & 3, k = rec >> 4;
					if (GAP == 1 && state == 1) { if (!((rec >> 2) & 1)) state = 0; cu--; continue; }
					if (GAP == 1 && state == 2) { if (!((rec >> 3) & 1)) state = 0; cv--; continue; }
					if (d == LQ_STOP) break;
					if (d == LQ_DIAG) {
						map[cv - 1] = (int16_t)(cu - 1);
						esim[cv - 1] = Su[(cv - 1) * LS + (cu - 1)];   // the unmodified similarity of the edge (metric/alignment.h:339)
						cu--; cv--;
					} else if (d == LQ_UP) {
						if (GAP == 1) state = 1; else cu -= GAP == 2 ? k : 1;
					} else {
						if (GAP == 1) state = 2; else cv -= GAP == 2 ? k : 1;
					}
				}
			}
		}
		wave_lds_fence();   // the next slice overwrites the strip
	}
}

template <bool FLOW>
static hipError_t launch_blocks(const VkLongqParams *p, int grid, size_t smem, hipStream_t stream) {
	void (*kernel)(VkLongqParams) = p->gap_mode == 0 ? vk_longq_blocks_kernel<FLOW, 0> : p->gap_mode == 1 ? vk_longq_blocks_kernel<FLOW, 1> : vk_longq_blocks_kernel<FLOW, 2>;
	if (smem > vk_host::kLongqLdsLimit) return hipErrorInvalidValue;
	if (smem > 64 * 1024) {
		const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
		if (e != hipSuccess) return e;
	}
	kernel<<<grid, 64, smem, stream>>>(*p);
	return hipGetLastError();
}

// The grid: the scoring pass as many workgroups (one wave each) as the CUs hold with this much LDS each, at most one per row of the
// work list; the tracebacks one per winner up to vk_host::kLongqFlowGrid -- a scratch region per workgroup, not per winner
extern "C" int32_t vk_longq_blocks_grid(int32_t len_t, int32_t max_len, int32_t gap_mode, int32_t flow_k, int64_t n_items) {
	if (flow_k > 0) return vk_host::longq_flow_grid(true, flow_k);
	return (int32_t)vk_host::longq_grid(longq_device_cus(), vk_host::longq_geometry_of(len_t, max_len, gap_mode, false, false).launch_lds_bytes, n_items);
}

// flow_k == 0: scores of the p->n_order rows of p->order; flow_k > 0: the flow_k winners of p->keys, of any length.  max_len: the
// corpus's longest slice (65 .. 512 tokens); the host has sized the scratch regions and set dm_off / su_off from the same geometry
extern "C" hipError_t vk_launch_longq_blocks(const VkLongqParams *p, int32_t max_len, int32_t flow_k, hipStream_t stream) {
	const vk_host::longq_geometry g = vk_host::longq_geometry_of(p->len_t, max_len, p->gap_mode, flow_k > 0, p->pos_s != nullptr);
	if (!g.blocks || p->s_stride != g.s_stride || p->dm_off != (int64_t)g.dm_off || p->su_off != (int64_t)g.su_off) return hipErrorInvalidValue;
	if ((p->gap_mode == 2 || flow_k > 0) && (!p->scratch || p->scratch_stride < (int64_t)g.scratch_bytes)) return hipErrorInvalidValue;
	const int grid = vk_longq_blocks_grid(p->len_t, max_len, p->gap_mode, flow_k, p->n_order);
	if (flow_k > 0) return launch_blocks<true>(p, grid, g.launch_lds_bytes, stream);
	if (p->n_order < 1) return hipSuccess;
	return launch_blocks<false>(p, grid, g.launch_lds_bytes, stream);
}
