// vk_score_body.hip.inc -- the body of vk_score_kernel (vk_score.hip.h), as text: included inside the braces of that kernel and of
// vk_score_local_kernel (vk_score_m9f.hip), which is the same kernel with one other DP call.  The including kernel provides
//   VkScoreParams p             its argument
//   MODE, NK32, TAIL, GAP, LT   vk_score_kernel's template parameters (or constants of those names)
//   FULL_LQ                     0: vk_score_kernel.  > 0 (GAP 8 only): local alignment and a query of FULL_LQ tokens -- a group of four
//                               slices of exactly 32 tokens takes the straight-line DP, every other group the general form with the
//                               locality and the column count at compile time (DESIGN 11.12)
// MODE 10 / 11 / 12 (vk_score_m10.hip ..): MODE 1 / 5 / 6 of a contextual handle under an operator chain (DESIGN 19) -- the tile
// product without its clip, then vk_host::contextual_cell: the chain, zeros on the columns past the query, the clip.
// Text and not a __forceinline__ device template on purpose: the compiler simplifies a device function on its own before it inlines
// it, and every kernel of vk_score_m0 .. m9*.hip then came out with another instruction stream (hundreds of instructions apart in
// vk_score_m2, m3 and m8; DESIGN 11.12).  Included, the kernels that were there compile to what they were, byte for byte.
	static_assert(FULL_LQ == 0 || (GAP == 8 && FULL_LQ <= LT), "the straight-line DP is a form of GAP 8");
	extern __shared__ float4 vk_smem4[];
	float *smem = reinterpret_cast<float *>(vk_smem4);
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int nwaves = blockDim.x >> 6;      // 4; 1 in the pass over long slices (group_list)
	// MODE 3: the first NK32 KiB of the dynamic LDS hold the query tile (shared by the block's waves)
	const uint8_t *qlds = reinterpret_cast<const uint8_t *>(smem);
	if constexpr (MODE == 3 || MODE == 4) {
		for (int i = threadIdx.x; i < NK32 * 64; i += blockDim.x)
			vk_smem4[i] = *reinterpret_cast<const float4 *>(p.qtile + i * 16);
		__syncthreads();
		smem += NK32 * 256;
	}
	// MODE 7: the 8-bit query tile and the cells' constants behind it (NK32 KiB + 192 bytes, in a region of NK32 KiB +
	// VK_DEV_BOUND_CONST_BYTES, which the host adds to the launch's dynamic LDS: vk_query.cpp, smem_bound)
	if constexpr (MODE == 7) {
		for (int i = threadIdx.x; i < NK32 * 64 + 12; i += blockDim.x)
			vk_smem4[i] = *reinterpret_cast<const float4 *>(p.qtile + i * 16);
		__syncthreads();
		smem += NK32 * 256 + VK_DEV_BOUND_CONST_BYTES / 4;
	}
	// MODE 8 / 9: the 6-bit query tile (every K-step whole) and the same constants behind it
	if constexpr (MODE == 8 || MODE == 9) {
		for (int i = threadIdx.x; i < VK_DEV_FP6_QTILE_BYTES / 16 + 12; i += blockDim.x)
			vk_smem4[i] = *reinterpret_cast<const float4 *>(p.qtile + i * 16);
		__syncthreads();
		smem += (VK_DEV_FP6_QTILE_BYTES + VK_DEV_BOUND_CONST_BYTES) / 4;
	}
	// MODE 1 (any d, fp32 tiles): the same staging with a runtime size; the K loop then reads the query with ds_read instead of
	// going through L1 for every token tile
	constexpr bool CHAIN = MODE == 10 || MODE == 11 || MODE == 12;
	if constexpr (MODE == 1 || MODE == 5 || MODE == 6 || CHAIN) {
		if (p.q_lds > 0) {
			for (int i = threadIdx.x; i * 16 < p.q_lds; i += blockDim.x)
				vk_smem4[i] = i * 16 < p.tile_bytes ? *reinterpret_cast<const float4 *>(p.qtile + i * 16) : float4{0.0f, 0.0f, 0.0f, 0.0f};
			__syncthreads();
			smem += p.q_lds / 4;
		}
	}
	float *S = smem + wv * p.lds_floats_per_wave;
	float *Hh = S + p.s_rows_per_wave * LT + 16;   // strip rows hold the LT query columns only; 16 floats of slack for lanes >= LT
	const int sigma = lane >> 4, v = lane & 15;

	QFrag<NK32, TAIL> qf;
	if constexpr (MODE == 0) load_qfrag<NK32, TAIL>(qf, p.qtile, lane);

	DpArgs a;
	a.locality = p.locality; a.len_t = p.len_t;
	a.gs = p.gs; a.gt = p.gt; a.a_s = p.a_s; a.a_t = p.a_t; a.open_s = p.open_s; a.open_t = p.open_t;
	a.ws = p.ws; a.wt = p.wt; a.wt0 = p.wt0;
	a.rwmd_symmetric = p.rwmd_symmetric; a.rwmd_normalize_bow = p.rwmd_normalize_bow; a.wmd_bound = p.wmd_bound;
	a.wrd_raw_total = p.wrd_raw_total;
	const float inv_ref = p.ref_total;
	// tag-weighted modifier: this lane's four query columns (MFMA layout: 4*(lane>>4) + r)
	// the bound pass is never taken with tag weights (bound_wanted in vk_route_host.h; the launchers of MODE 7 / 8 refuse pos_s):
	// its kernels do not carry the lane's eight modifier registers through their loops
	constexpr bool TAGS = MODE != 7 && MODE != 8 && MODE != 9;
	float twl[4] = {1.0f, 1.0f, 1.0f, 1.0f};
	int tposl[4] = {0, 0, 0, 0};
	if (TAGS && p.pos_s) {
		const int cbase = (MODE == 2) ? (lane & 3) * 4 : (lane >> 4) * 4;
#pragma unroll
		for (int r = 0; r < 4; r++) { twl[r] = p.tw[cbase + r]; tposl[r] = p.tpos[cbase + r]; }
	}

	// general gap, fast form: gap tables in (scalar) registers for the whole kernel
	// (the flat-tailed forms: w_s[0 .. K] and the tail's cost, which comes by value)
	constexpr bool FLAT = GAP == 8 || GAP == 9;
	static_assert(!FLAT || MODE == 7 || MODE == 8 || MODE == 9, "a flat-tailed table gives a bound, not a score");
	constexpr int WSN = FLAT ? VK_BOUND_TAIL_K + 2 : GAP == 6 ? 65 : 33;
	float wsr[WSN], wtr[LT];
	if (GAP == 3 || GAP == 6 || FLAT) {
#pragma unroll
		for (int k = 0; k < (FLAT ? WSN - 1 : WSN); k++) wsr[k] = p.ws[k];
		if (FLAT) wsr[WSN - 1] = p.bound_tail_cost;
#pragma unroll
		for (int k = 0; k < LT; k++) wtr[k] = p.wt[k];
	}

	// groups of 4 consecutive slices; slices longer than max_short_len sit alone in their group (the host
	// pads the slice table, vk_corpus.cpp set_slices_impl) and are left to a second launch that walks
	// group_list with one wave per workgroup and a larger LDS strip
	// A wave takes runs of VK_RUN consecutive groups: when sentences are not tile-aligned, the tile that
	// straddles two groups is then computed once and its rows are carried over in the strip (ragged corpora:
	// one tile in ten).
	const int n_groups = p.group_list ? p.n_list : (p.n_sent + 3) >> 2;
	const int run = p.group_list ? 1 : VK_RUN;
	const int n_runs = (n_groups + run - 1) / run;
	for (int ri = blockIdx.x * nwaves + wv; ri < n_runs; ri += gridDim.x * nwaves) {
	int prev_tile = -1, prev_row = 0;   // last tile of the previous group of this run, and its place in the strip
	for (int gg = 0; gg < run; gg++) {
		const int gi = ri * run + gg;
		if (gi >= n_groups) break;
		const int grp = p.group_list ? p.group_list[gi] : gi;
		const int s_idx = grp * 4 + sigma;
		const int i0 = s_idx < p.n_sent ? s_idx : p.n_sent;       // entries >= n_sent are empty slices
		const int t_a = p.sent_start[i0], t_b = p.sent_end[i0];
		const int len = t_b - t_a;
		const int g_a = __builtin_amdgcn_readlane(t_a, 0);
		const int g_b = __builtin_amdgcn_readlane(t_b, 48);
		int maxlen = __builtin_amdgcn_readlane(len, 0);
		maxlen = max(maxlen, __builtin_amdgcn_readlane(len, 16));
		maxlen = max(maxlen, __builtin_amdgcn_readlane(len, 32));
		maxlen = max(maxlen, __builtin_amdgcn_readlane(len, 48));
		if (!p.group_list && maxlen > p.max_short_len) { prev_tile = -1; continue; }

		int rowbase;
		if (MODE == 2) {
			// gather: lane handles token (lane >> 2) + 16*it, 4 query columns (lane & 3)
			// two dependent loads per token (id, then the table row): issue them four tokens deep so that the
			// L2 latencies overlap instead of adding up
			const int ntok = g_b - g_a;
			for (int it0 = 0; it0 * 16 < ntok; it0 += 4) {
				int id[4];
				float4 val[4];
#pragma unroll
				for (int q4 = 0; q4 < 4; q4++) {
					const int tk = (it0 + q4) * 16 + (lane >> 2);
					id[q4] = p.tok_id[g_a + (tk < ntok ? tk : 0)];
				}
#pragma unroll
				for (int q4 = 0; q4 < 4; q4++)
					val[q4] = *reinterpret_cast<const float4 *>(p.table + (int64_t)id[q4] * 16 + (lane & 3) * 4);
#pragma unroll
				for (int q4 = 0; q4 < 4; q4++) {
					const int tk = (it0 + q4) * 16 + (lane >> 2);
					if (tk < ntok) {
						float4 vq = val[q4];
						if (p.pos_s) {
							const int ps = p.pos_s[g_a + tk];
							vq.x = tag_weighted(vq.x, twl[0], ps, tposl[0], p.tw_keep, p.tw_threshold);
							vq.y = tag_weighted(vq.y, twl[1], ps, tposl[1], p.tw_keep, p.tw_threshold);
							vq.z = tag_weighted(vq.z, twl[2], ps, tposl[2], p.tw_keep, p.tw_threshold);
							vq.w = tag_weighted(vq.w, twl[3], ps, tposl[3], p.tw_keep, p.tw_threshold);
						}
						if ((lane & 3) * 4 < LT) *reinterpret_cast<float4 *>(S + tk * LT + (lane & 3) * 4) = vq;
					}
				}
			}
			rowbase = t_a - g_a;
		} else {
			const int tile0 = g_a >> 4;
			const int ntiles = ((g_b + 15) >> 4) - tile0;
			const uint8_t *tp = p.tiles + (int64_t)tile0 * p.tile_bytes;
			int ti0 = 0;
			if (ntiles > 0 && tile0 == prev_tile) {
				// the previous group ended inside this tile: its 16 rows are in the strip already
				if (prev_row != 0) {
					float4 keep = {0.0f, 0.0f, 0.0f, 0.0f};
					if (lane < 4 * LT) keep = reinterpret_cast<const float4 *>(S)[prev_row * 4 * LT + lane];   // 16 rows of LT floats
					wave_lds_fence();
					if (lane < 4 * LT) reinterpret_cast<float4 *>(S)[lane] = keep;
				}
				ti0 = 1;
				tp += p.tile_bytes;
			}
			if (ntiles > 0) { prev_tile = tile0 + ntiles - 1; prev_row = ntiles - 1; }
			if constexpr (MODE == 8 || MODE == 9) {
				// VK_FP6_TILES tiles per trip while the group has that many left, all their loads ahead of the first MFMA; then what
				// is left (fewer than T; with ti0 = 1 a group may have no tile at all) one tile per trip.  Both bounds are
				// wave-uniform: a tile past the group's last is neither loaded nor written to the strip
				// the 64-row history (GAP 6) keeps one tile per trip: with two its forms allocate 128 registers, past the 120 that the
				// 32-row forms keep to; no corpus of that shape has been measured either way
				// the flat-tailed forms keep K + 1 rows of history: VK_FP6_TILES_TAIL / VK_FP6_TILES_TAIL64 (vk_score_m8t.hip)
				constexpr int T = GAP == 6 ? 1 : GAP == 8 ? VK_FP6_TILES_TAIL : GAP == 9 ? VK_FP6_TILES_TAIL64 : VK_FP6_TILES;
				const auto tiles = [&](auto tc, int ti) {
					constexpr int N = decltype(tc)::value;
					f32x4 ub[N];
					sim_tiles_fp6<N, MODE == 9>(ub, qlds, tp, p.tile_bytes, lane, p.bound_live);
#pragma unroll
					for (int i = 0; i < N; i++)
						if ((lane >> 4) * 4 < LT) *reinterpret_cast<f32x4 *>(S + ((ti + i) * 16 + (lane & 15)) * LT + (lane >> 4) * 4) = ub[i];
					tp += (int64_t)N * p.tile_bytes;
				};
				int ti = ti0;
				for (; ti + T <= ntiles; ti += T) tiles(std::integral_constant<int, T>{}, ti);
				if constexpr (T > 1)
					for (; ti < ntiles; ti++) tiles(std::integral_constant<int, 1>{}, ti);
			} else
			for (int ti = ti0; ti < ntiles; ti++) {
				f32x4 acc;
				if constexpr (MODE == 0) acc = sim_tile<NK32, TAIL>(qf, tp, lane);
				else if constexpr (MODE == 3) acc = sim_tile_qlds<NK32, TAIL>(qlds, tp, lane);
				else if constexpr (MODE == 4) acc = sim_tile_f32_qlds<NK32>(qlds, tp, lane);
				else if constexpr (MODE == 7) acc = sim_tile_i8<NK32>(qlds, tp, lane, p.bound_live);
				else if constexpr (CHAIN) {
					constexpr bool DEEP = MODE == 11 || MODE == 12;
					constexpr int PREC = MODE == 12 ? 1 : 0;
					if (p.q_lds > 0) acc = sim_tile_generic<DEEP, PREC, false>(qlds, tp, p.nk32, p.tail, lane);
					else acc = sim_tile_generic<DEEP, PREC, false>(p.qtile, tp, p.nk32, p.tail, lane);
					// lane l holds query columns 4 (l >> 4) .. + 3: the chain on those the query holds, zeros behind them, the clip
#pragma unroll
					for (int r = 0; r < 4; r++) acc[r] = vk_host::contextual_cell(acc[r], (lane >> 4) * 4 + r < p.len_t, p.sim_ops);
				}
				else {
					// two calls, not one with a selected pointer: an LDS-or-global pointer is a flat pointer, and flat loads count
					// on both wait counters -- every batch of tile loads would be waited for in full
					constexpr bool DEEP = MODE == 5 || MODE == 6;
					constexpr int PREC = MODE == 6 ? 1 : 0;
					if (p.q_lds > 0) acc = sim_tile_generic<DEEP, PREC>(qlds, tp, p.nk32, p.tail, lane);
					else acc = sim_tile_generic<DEEP, PREC>(p.qtile, tp, p.nk32, p.tail, lane);
				}
				if (TAGS && p.pos_s) {
					const int ps = p.pos_s[(tile0 + ti) * 16 + (lane & 15)];
#pragma unroll
					for (int r = 0; r < 4; r++) acc[r] = tag_weighted(acc[r], twl[r], ps, tposl[r], p.tw_keep, p.tw_threshold);
				}
				if ((lane >> 4) * 4 < LT) *reinterpret_cast<f32x4 *>(S + (ti * 16 + (lane & 15)) * LT + (lane >> 4) * 4) = acc;
				tp += p.tile_bytes;
			}
			rowbase = t_a - tile0 * 16;
		}
		wave_lds_fence();
		// tag-weighted vocabulary transport: cells upstream writes twice (static_vocab_fixup).  The four slices of the wave share one
		// strip of rows: over sliding windows a rewritten cell may belong to a neighbour too, and the slices take turns
		int turns = 1;
		bool rewrite = false;
		if constexpr (MODE == 2 && (GAP == 4 || GAP == 7)) {
			if (p.qid_bits) {
				rewrite = len > 0 && static_vocab_shared(len, p.len_t, p.tok_id + t_a, p.tag_s + t_a, p.qid_bits, p.qkey) != 0;
				if (p.slices_overlap && __builtin_amdgcn_ballot_w64(rewrite) != 0) turns = 4;
				else if (rewrite) static_vocab_fixup<16>(S + rowbase * LT, LT, len, p.len_t, p.tok_id + t_a, p.tag_s + t_a, p.pos_s + t_a, p.table, 0,
					p.qid_bits, p.qkey, p.tw, p.tpos, p.tw_keep, p.tw_threshold, v);
				wave_lds_fence();
			}
		}

		const int lenc = len > 0 ? len : 0;
		const int rb = len > 0 ? rowbase : 0;
		auto evaluate = [&]() -> float {
		float raw;
		if constexpr (GAP == 0) raw = dp_linear<LT>(S, rb, lenc, maxlen, v, a);
		else if constexpr (GAP == 1) raw = dp_affine<LT>(S, rb, lenc, maxlen, v, a);
		else if constexpr (GAP == 2) raw = dp_general<LT>(S, Hh, p.h_rows, rb, lenc, maxlen, lane, a);
		else if constexpr (GAP == 3) raw = dp_general_reg<LT, 32>(S, rb, lenc, maxlen, v, a, wsr, wtr);
		// MODE 7 with the 64-row history (config 5 of the benchmark: 768-d rows) keeps the DP's invariants for the kernel's lifetime:
		// 65 KB of LDS per workgroup admit two per CU, so 111 registers buy nothing there where 187 fit, and redoing 80 selects per
		// group cost 1 % of the kernel (4.40 -> 4.44 ms, DESIGN 11.9)
		else if constexpr (GAP == 6) raw = dp_general_reg<LT, 64, MODE != 7>(S, rb, lenc, maxlen, v, a, wsr, wtr);
		else if constexpr (GAP == 8 && FULL_LQ > 0) {
			// wave-uniform: four slices of 32 tokens each (an empty slot past n_sent or a slice the host emptied has len 0)
			if (maxlen == 32 && __builtin_amdgcn_ballot_w64(len != 32) == 0) raw = dp_tail_local_full<LT, FULL_LQ, VK_BOUND_TAIL_K>(S, rowbase, v, a, wsr, wtr);
			else raw = dp_general_tail_reg<LT, 32, VK_BOUND_TAIL_K, true, VK_DEV_LOCAL, FULL_LQ>(S, rb, lenc, maxlen, v, a, wsr, wtr);
		}
		else if constexpr (GAP == 8) raw = dp_general_tail_reg<LT, 32, VK_BOUND_TAIL_K>(S, rb, lenc, maxlen, v, a, wsr, wtr);
		else if constexpr (GAP == 9) raw = dp_general_tail_reg<LT, 64, VK_BOUND_TAIL_K, MODE != 7>(S, rb, lenc, maxlen, v, a, wsr, wtr);
		else if constexpr (GAP == 4) {
			// stage 1 of the full WMD over normalised bags of words = the WRD bound with unit magnitudes
			if (a.wmd_bound == 1) raw = wrd_bound_rows<LT>(S, rb, lenc, maxlen, v, a, nullptr, nullptr, 1.0f / (float)a.len_t);
			else raw = rwmd_rows<LT>(S, rb, lenc, maxlen, v, a);
		}
		else if constexpr (GAP == 7) {
			// masses of the slice's vocabulary entries (static layout: repeated token ids count once, at their
			// first position); stride 0 in the pass over long slices, where only DPP row 0 holds a slice
			float *sm = nullptr;
			if (MODE == 2) {
				sm = Hh + sigma * p.m_rows;
				const float wsum = p.rwmd_normalize_bow ? (float)(lenc > 0 ? lenc : 1) : 1.0f;   // bow[i] /= w_sum (bow.h:262-270): a division, as upstream -- a mass that ties with a capacity must tie here too
				for (int u = v; u < lenc; u += 16) {
					const int id = p.tok_id[t_a + u];
					int cnt = 0;
					bool first = true;
					for (int i = 0; i < lenc; i++) {
						const bool same = p.tok_id[t_a + i] == id && (!p.tag_s || p.tag_s[t_a + i] == p.tag_s[t_a + u]);
						cnt += same ? 1 : 0;
						first = first && !(same && i < u);
					}
					sm[u] = first ? (float)cnt / wsum : 0.0f;
				}
				wave_lds_fence();
			}
			raw = rwmd_fill_rows<LT>(S, sm, rb, lenc, maxlen, lane, a, p.qmass[v]);
		}
		else if constexpr (MODE == 2) raw = wrd_bound_rows<LT>(S, rb, lenc, maxlen, v, a, p.mag, p.tok_id + (len > 0 ? t_a : 0), p.qmass[v]);
		else raw = wrd_bound_rows<LT>(S, rb, lenc, maxlen, v, a, p.mag + (len > 0 ? t_a : 0), nullptr, p.qmass[v]);
		return raw;
		};
		float raw = 0.0f;
		if constexpr (MODE == 2 && (GAP == 4 || GAP == 7)) {
			if (turns > 1) {
				for (int turn = 0; turn < 4; turn++) {
					const bool mine = sigma == turn;
					if (mine && rewrite) static_vocab_fixup<16>(S + rowbase * LT, LT, len, p.len_t, p.tok_id + t_a, p.tag_s + t_a, p.pos_s + t_a, p.table, 0,
						p.qid_bits, p.qkey, p.tw, p.tpos, p.tw_keep, p.tw_threshold, v);
					wave_lds_fence();
					const float r = evaluate();
					if (mine) raw = r;
					wave_lds_fence();
					if (mine && rewrite) static_vocab_fixup<16, false, true>(S + rowbase * LT, LT, len, p.len_t, p.tok_id + t_a, p.tag_s + t_a, p.pos_s + t_a, p.table, 0,
						p.qid_bits, p.qkey, p.tw, p.tpos, p.tw_keep, p.tw_threshold, v);
					wave_lds_fence();
				}
			} else raw = evaluate();
		} else raw = evaluate();

		if (v == 15 && s_idx < p.n_sent) {
			// Score::value = raw / reference_score * boost; reference_score == len_t for
			// submatch_weight == 0 (metric/alignment.h:84-106, match/match.h:302-307)
			float val = VK_NEG_INF, r = VK_NEG_INF;
			if (len >= 1) {   // document.h:160 skips empty slices
				const float boost = p.boost ? p.boost[s_idx] : 1.0f;
				r = raw;
				val = (raw / inv_ref) * boost;
			}
			p.scores[s_idx] = val;
			if (p.raw) p.raw[s_idx] = r;
		}
		wave_lds_fence();
	}
	}
