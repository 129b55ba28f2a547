// vk_query.cpp -- C-ABI: one query against a resident corpus (validation, launches, result assembly) and the
// merge of result sets.
// No CPU compute fallback exists: without a HIP device every entry point that
// would compute returns VK_ERR_NO_DEVICE / VK_ERR_HIP.

#include "vk_internal.h"
#include "vk_guard.h"
#include "vk_transport_host.h"

// The route of a query (vk_route_host.h): the facts it is decided from, copied from the corpus and the query -- one place for
// vk_validate_query, which refuses a shape before anything is enqueued, and for query_run::route().  (bound_pass stays false here: the
// handle's back-off is asked by the query that runs.)
using vk_host::kCanonMargin;   // runners-up selected with the winners where the host restates the winners' scores
static const vk_host::route_fits kRouteFits{vk_score32_waves, vk_wide_ring_rows, vk_wide_lds_demand};
static bool exact_transport(const vk_query_desc *q) { return vk_host::exact_transport(q->algorithm, q->wmd_full != 0); }
static vk_host::route_facts route_facts_of(const vk_corpus *c, const vk_query_desc *q, const vk_topk_out *out) {
	vk_host::route_facts f;
	f.layout = c->desc.layout; f.prec = c->prec; f.nk32 = c->nk32; f.tail = c->tail;
	f.max_len = c->max_len; f.max_short_len = c->max_short_len; f.n_long_groups = c->n_long_groups;
	f.has_apart = c->h_apart && !c->h_apart->empty(); f.has_xlong = c->h_xlong && !c->h_xlong->empty();
	f.max_pair_tiles = c->max_pair_tiles; f.max_short_pair_tiles = c->max_short_pair_tiles; f.uniform_len = c->uniform_len;
	f.has_pos = c->d_pos != nullptr; f.has_tags = c->d_tag != nullptr; f.n_sentences = c->desc.n_sentences;
	f.chained = c->desc.layout == VK_LAYOUT_CONTEXTUAL && c->sim_ops.n > 0;   // vk_corpus_set_contextual_sim_ops
	f.algorithm = q->algorithm; f.wmd_full = q->wmd_full != 0; f.rwmd_injective = q->rwmd_injective != 0; f.len_t = q->len_t;
	if (q->algorithm == VK_ALG_ALIGN) {
		f.gaps = vk_host::classify_gaps(q->gap_s, q->gap_t);
		// (vk_validate_query asks before it has looked at the gap kinds: no table is read under a kind that is none)
		if (f.gaps.gap_mode == 2 && q->gap_s.kind >= VK_GAP_LINEAR && q->gap_s.kind <= VK_GAP_TABLE) f.ws_tail = vk_host::ws_tail_of(q->gap_s, c->max_len);
	}
	f.submatch = q->submatch_weight > 0.0f; f.tagged = q->tag_weights != nullptr; f.has_q_tags = q->q_tags != nullptr; f.has_q_ids = q->q_token_ids != nullptr;
	f.only = q->only_slices != nullptr; f.want_flow = q->want_flow != 0; f.locality = q->locality;
	f.sim_rows = out->sim_rows != nullptr; f.raw_score = out->raw_score != nullptr; f.boost = q->boost != nullptr;
	// the size of the selection.  Winners restated on the host (tracebacks; the relaxed WMD's rows): a few runners-up are selected with
	// them (57 .. 64 matches: the margin takes the selection to the k > 64 path; beyond VK_MAX_MATCHES: every score is sorted, never
	// more winners than rows)
	const int k = q->max_matches;
	const bool restated = (q->want_flow && q->algorithm == VK_ALG_ALIGN) || (q->algorithm == VK_ALG_RWMD && !q->wmd_full && q->want_flow && out->sim_rows);
	f.kk = f.only ? q->n_only : (int)std::min<int64_t>(!restated ? k : (k <= VK_MAX_MATCHES ? std::min(k + kCanonMargin, VK_MAX_MATCHES) : k + kCanonMargin), std::max<int64_t>(c->n_entries, 1));
	return f;
}

int vk_validate_query(const vk_corpus *c, const vk_query_desc *q, const vk_topk_out *out) {
	if (!c || !q || !out) return fail(VK_ERR_INVALID, "null argument");
	if (!c->finalized) return fail(VK_ERR_STATE, "corpus not finalized");
	if (q->len_t < 1) return fail(VK_ERR_INVALID, "empty query");
	if (q->len_t > VK_MAX_LONG_QUERY_LEN) return fail(VK_ERR_UNSUPPORTED, "query longer than VK_MAX_LONG_QUERY_LEN (512) tokens");
	if (c->span_sim.active()) {
		// a span corpus under its span similarity (vk_corpus_set_span_sim): vk_span_sim_kernel / vk_span_ops_kernel score one query row
		// against one-row slices and nothing else does -- decided here, before anything is enqueued (vk_span_sim_host.h)
		vk_host::span_sim_query s;
		s.algorithm = q->algorithm; s.locality = q->locality; s.len_t = q->len_t; s.uniform_len = c->uniform_len;
		s.tagged = q->tag_weights != nullptr; s.submatch = q->submatch_weight != 0.0f; s.boost = q->boost != nullptr;
		s.want_flow = q->want_flow != 0; s.only = q->only_slices != nullptr; s.sim_rows = out->sim_rows != nullptr;
		if (const char *what = vk_host::span_sim_refusal(s))
			return fail(VK_ERR_UNSUPPORTED, std::string("a handle under a span similarity (vk_corpus_set_span_sim) answers one-row local alignment queries over one-row slices, score = sim(span, query): this query asks for ") + what);
	}
	if (q->len_t > VK_MAX_QUERY_LEN) {
		// 65 .. 512 tokens: the role-swapped one-wave-per-slice kernel (vk_longq_kernel) -- alignments over slices of at most
		// VK_MAX_SENT_LEN tokens (those of more than 64: its block form)
		if (c->desc.layout == VK_LAYOUT_CONTEXTUAL && c->sim_ops.n > 0) {   // under an operator chain: the router's refusal, by name
			const vk_host::query_route r = vk_host::route_query(route_facts_of(c, q, out), vk_host::route_switches{}, kRouteFits);
			return fail(r.status, r.message);
		}
		if (q->algorithm != VK_ALG_ALIGN) return fail(VK_ERR_UNSUPPORTED, "queries of more than VK_MAX_QUERY_LEN (64) tokens: alignments only (the transports keep a lane per query token)");
		if (c->max_len > VK_MAX_SENT_LEN) return fail(VK_ERR_UNSUPPORTED, "queries of more than 64 tokens over a corpus that holds a slice of more than VK_MAX_SENT_LEN (512) tokens: the state of such a slice does not fit a workgroup's LDS");
		if (q->submatch_weight != 0.0f) return fail(VK_ERR_UNSUPPORTED, "queries of more than 64 tokens with a submatch weight");
		if (out->sim_rows) return fail(VK_ERR_UNSUPPORTED, "queries of more than 64 tokens: similarity rows of the winners are not returned");
		if (q->max_matches > VK_MAX_MATCHES) return fail(VK_ERR_UNSUPPORTED, "queries of more than 64 tokens: max_matches <= VK_MAX_MATCHES");
	}
	if (q->len_t <= VK_MAX_QUERY_LEN) {   // (the switches a refusal reads: none)
		const vk_host::route_facts facts = route_facts_of(c, q, out);
		const vk_host::query_route r = vk_host::route_query(facts, vk_host::route_switches{}, kRouteFits);
		if (r.status != VK_OK && (!r.fits32 || facts.chained)) return fail(r.status, r.message);   // (under an operator chain: every refusal of the route)
	}
	// Slices of more than VK_MAX_SENT_LEN tokens (whole documents as slices, up to VK_MAX_DOC_LEN): alignments -- the
	// one-wave-per-slice kernel with the slice's state in global memory (vk_wide_kernel, global-state form; the same form takes a
	// query of more than 16 tokens whose state over the corpus's longest slice exceeds the LDS: VK_ERR_UNSUPPORTED in round 2) --
	if (c->max_len > VK_MAX_SENT_LEN && q->algorithm != VK_ALG_ALIGN) {
		// ... and the relaxed word mover's distance in its 1:1 form (a stream of row / column minima; the winners' rows restated
		// tile by tile, vk_canon_rows_kernel); the 1:n form and the exact transports keep a slice's bag of words in LDS
		const bool relaxed_11 = q->algorithm == VK_ALG_RWMD && !q->wmd_full && q->rwmd_injective;
		if (!relaxed_11)
			return fail(VK_ERR_UNSUPPORTED, "slices of more than VK_MAX_SENT_LEN (512) tokens: alignments and the relaxed 1:1 word mover's distance only (the 1:n form and the exact transports keep a slice's bag of words in LDS)");
		if (c->desc.layout == VK_LAYOUT_STATIC && q->tag_weights && q->q_tags && q->q_token_ids && c->d_tag)
			return fail(VK_ERR_UNSUPPORTED, "slices of more than VK_MAX_SENT_LEN (512) tokens: tag-weighted vocabulary transports keyed by (id, tag) rewrite cells of a slice's rows in LDS");
	}
	if (!q->q_vectors) return fail(VK_ERR_INVALID, "q_vectors is null");
	if (c->mixed()) {   // a combinator (vk_corpus_set_sim_mix): every operand's rows of this query, and no magnitudes
		if (q->algorithm == VK_ALG_WRD)
			return fail(VK_ERR_UNSUPPORTED, "VK_ALG_WRD on a mixed handle: the reference leaves the magnitudes of a token similarity combinator unwritten");
		for (int m = 1; m < c->sim_mix.n; m++) {
			const auto &pending = c->mixop[m - 1].pending;
			if ((size_t)c->q_operand_at >= pending.size())
				return fail(VK_ERR_STATE, "mixed handle: no rows of operand " + std::to_string(m) + " for this query (vk_corpus_set_query_operand)");
			if (pending[(size_t)c->q_operand_at].len_t != q->len_t)
				return fail(VK_ERR_STATE, "mixed handle: operand " + std::to_string(m) + " was given " + std::to_string(pending[(size_t)c->q_operand_at].len_t) +
					" rows for a query of " + std::to_string(q->len_t) + " tokens");
		}
	}
	if (q->q_dtype != VK_F32 && q->q_dtype != VK_BF16) return fail(VK_ERR_INVALID, "bad q_dtype");
	if (q->max_matches < 1 || q->max_matches > VK_MAX_MATCHES_SORTED) return fail(VK_ERR_INVALID, "max_matches out of range");
	// beyond VK_MAX_MATCHES: every score sorted on the device -- alignments (with or without their tracebacks), no submatch weight;
	// the transports' candidate rounds and row buffers are sized for VK_MAX_MATCHES
	if (q->max_matches > VK_MAX_MATCHES && !q->only_slices && (q->algorithm != VK_ALG_ALIGN || q->submatch_weight != 0.0f || out->sim_rows))
		return fail(VK_ERR_UNSUPPORTED, "max_matches beyond VK_MAX_MATCHES (1024): alignments without a submatch weight only");
	if (out->capacity < q->max_matches) return fail(VK_ERR_INVALID, "output capacity smaller than max_matches");
	if (!out->score || !out->sentence) return fail(VK_ERR_INVALID, "output arrays missing");
	// (the batched paths copy 64 rows per winner into sim_rows at a stride of rows_per_winner: never below 64)
	if (out->sim_rows && out->rows_per_winner != 0 && (out->rows_per_winner < VK_FAST_SENT_LEN || out->rows_per_winner % 64 != 0 || out->rows_per_winner > VK_MAX_DOC_LEN + 1))
		return fail(VK_ERR_INVALID, "rows_per_winner must be 0 or a multiple of 64 (64 .. VK_MAX_DOC_LEN + 1)");
	if (!(q->submatch_weight >= 0.0f)) return fail(VK_ERR_INVALID, "submatch_weight must be >= 0 (pow of a zero base, metric/alignment.h:97-99)");
	if (q->only_slices) {
		if (q->n_only < 1 || q->n_only > VK_MAX_MATCHES || q->n_only > out->capacity) return fail(VK_ERR_INVALID, "only_slices: n_only out of range (1 .. min(VK_MAX_MATCHES, capacity))");
		const bool relaxed = q->algorithm == VK_ALG_RWMD && !q->wmd_full && out->sim_rows != nullptr;   // restated on the host from the rows
		const bool exact = exact_transport(q);  // every listed slice solved
		// (a submatch weight: alignments only -- the score of a listed slice is its aligner score over the reference score of its own
		// traceback, metric/alignment.h:84-106, no candidate rounds; the transports' reference score does not depend on it)
		if (!(q->algorithm == VK_ALG_ALIGN || relaxed || exact) || !q->want_flow || (q->submatch_weight != 0.0f && q->algorithm != VK_ALG_ALIGN))
			return fail(VK_ERR_UNSUPPORTED, "only_slices states alignments, relaxed WMD with sim_rows, or exact transports, with want_flow (and submatch_weight = 0 for the transports)");
		for (int i = 0; i < q->n_only; i++)
			if (q->only_slices[i] < 0 || q->only_slices[i] >= c->desc.n_sentences) return fail(VK_ERR_INVALID, "only_slices: slice index out of range");
	}
	if (q->bidirectional) return fail(VK_ERR_UNSUPPORTED, "bidirectional is not implemented (unused upstream, query.cpp:81-83)");
	// the two checks every algorithm makes, each at its own place among the others (which error a doubly wrong query gets)
	int rc = VK_OK;
	const auto tag_weights = [&]() -> int {   // TagWeightedSlice wraps any slice, whatever the matcher (match/instantiate.cpp:173-189)
		if (!q->tag_weights) return VK_OK;
		if (!q->q_pos) return fail(VK_ERR_INVALID, "tag-weighted query without q_pos");
		if (!c->d_pos) return fail(VK_ERR_STATE, "tag-weighted query needs vk_corpus_set_token_pos");
		if (q->similarity_threshold < 0.0f) return fail(VK_ERR_INVALID, "similarity_threshold must be >= 0 (slice/static.h:209)");
		return VK_OK;
	};
	const auto flow_arrays = [&]() -> int {
		return (q->want_flow && (!out->mapping || !out->edge_sim)) ? fail(VK_ERR_INVALID, "want_flow needs mapping and edge_sim arrays") : VK_OK;
	};
	if (q->algorithm == VK_ALG_ALIGN) {
		if (q->locality < VK_LOCAL || q->locality > VK_SEMIGLOBAL) return fail(VK_ERR_INVALID, "bad locality");
		for (const vk_gap *g : {&q->gap_s, &q->gap_t}) {
			if (g->kind < VK_GAP_LINEAR || g->kind > VK_GAP_TABLE) return fail(VK_ERR_INVALID, "bad gap kind");
			if (g->kind == VK_GAP_TABLE && (!g->table || g->n_table < 1)) return fail(VK_ERR_INVALID, "gap table missing");
		}
		if (q->gap_s.kind == VK_GAP_TABLE && q->gap_s.n_table <= c->max_len) return fail(VK_ERR_INVALID, "gap_s table shorter than the longest sentence");
		if (q->gap_t.kind == VK_GAP_TABLE && q->gap_t.n_table <= q->len_t) return fail(VK_ERR_INVALID, "gap_t table shorter than the query");
		if ((rc = flow_arrays())) return rc;
		if ((rc = tag_weights())) return rc;
	} else if (q->algorithm == VK_ALG_RWMD) {
		if ((rc = tag_weights())) return rc;
		if (q->tag_weights) {
			if (q->q_tags && c->desc.layout == VK_LAYOUT_STATIC) {
				// vocabulary keys (token id, tag) as id * 256 + tag in 32 bits, ordered as upstream's signed pairs: ids below 2^23, tags 0 .. 127
				if (c->desc.vocab_size > (1 << 23)) return fail(VK_ERR_UNSUPPORTED, "tag-weighted transport with q_tags over the static layout: vocabularies of more than 2^23 entries overflow the (id, tag) keys");
				for (int j = 0; j < q->len_t; j++) {
					if (q->q_tags[j] < 0) return fail(VK_ERR_INVALID, "q_tags: tag codes must be 0 .. 127");
					// (words the corpus does not hold carry ids of their own above the vocabulary, QueryVocabulary: they key entries too)
					if (q->q_token_ids && q->q_token_ids[j] >= (1 << 23)) return fail(VK_ERR_UNSUPPORTED, "q_token_ids: ids of 2^23 and more overflow the (id, tag) keys");
				}
			}
			if (q->q_tags && !q->rwmd_injective && !q->wmd_full && c->desc.layout == VK_LAYOUT_STATIC && !c->d_tag)
				return fail(VK_ERR_STATE, "tag-weighted 1:n RWMD over the static layout with q_tags needs vk_corpus_set_token_tags (its vocabulary is keyed by (token, tag), bow.h:150-176)");
		}
		if (q->rwmd_symmetric && !q->rwmd_normalize_bow)
			return fail(VK_ERR_INVALID, "cannot run symmetric mode WMD with bow (needs nbow)");   // wmd.h:441-449
		if (q->wmd_full) {
			if (q->rwmd_injective) return fail(VK_ERR_INVALID, "non-relaxed WMD with injective mapping is not supported");      // wmd.h:201-204
			if (q->rwmd_symmetric) return fail(VK_ERR_INVALID, "non-relaxed WMD with symmetric computation is not supported");  // wmd.h:206-209
		}
		if ((rc = flow_arrays())) return rc;
	} else if (q->algorithm == VK_ALG_WRD) {
		if ((rc = tag_weights())) return rc;
		if (!c->d_mag) return fail(VK_ERR_STATE, "VK_ALG_WRD needs a corpus created with keep_magnitudes = 1");
		if ((rc = flow_arrays())) return rc;
	} else {
		return fail(VK_ERR_INVALID, "bad algorithm");
	}
	return VK_OK;
}

// Vectors.normalized for the query rows, then bf16 (RNE), then tile order (16 rows,
// rows >= len_t zero).  Same arithmetic as oracle/vk_oracle.c vko_normalize_rows_bf16.
void vk_pack_query_rows(int d, int tile_bytes, int prec, const void *q_vectors, int q_dtype, int q_normalize, int len_t, std::vector<uint8_t> &tile, float *mags) {
	tile.assign((size_t)tile_bytes * (size_t)((len_t + 15) / 16), 0);   // tile i / 16 holds row i % 16
	std::vector<float> row((size_t)d);
	for (int i = 0; i < len_t; i++) {
		for (int k = 0; k < d; k++)
			row[(size_t)k] = q_dtype == VK_F32 ? ((const float *)q_vectors)[(size_t)i * d + k]
			                                    : bf16_to_f32(((const uint16_t *)q_vectors)[(size_t)i * d + k]);
		double acc = 0.0;
		for (int k = 0; k < d; k++) acc += (double)row[(size_t)k] * (double)row[(size_t)k];
		float m = (float)std::sqrt(acc);
		if (m != m) m = 0.0f;
		mags[i] = m;
		if (q_normalize) {
			for (int k = 0; k < d; k++) {
				float v = row[(size_t)k] / m;
				if (v != v) v = 0.0f;
				row[(size_t)k] = v;
			}
		}
		for (int k = 0; k < d; k++) {
			if (prec) {   // fp32 tile: block k >> 4, lane 16 (k & 3) + row, element (k & 15) >> 2
				const size_t off = (size_t)(i >> 4) * tile_bytes + (size_t)(k >> 4) * 1024 + (size_t)((k & 3) * 16 + (i & 15)) * 16 + (size_t)((k & 15) >> 2) * 4;
				memcpy(&tile[off], &row[(size_t)k], 4);
				continue;
			}
			const uint16_t b = f32_to_bf16(row[(size_t)k]);
			const int t = k >> 5, g = (k & 31) >> 3, j = k & 7;
			const size_t off = (size_t)(i >> 4) * tile_bytes + (size_t)t * 1024 + (size_t)(g * 16 + (i & 15)) * 16 + (size_t)j * 2;
			memcpy(&tile[off], &b, 2);
		}
	}
}

void vk_pack_query(const vk_corpus *c, const vk_query_desc *q, std::vector<uint8_t> &tile, float *mags, std::vector<uint8_t> *bound_tile) {
	const int d = c->desc.d;
	vk_pack_query_rows(d, c->tile_bytes, c->prec, q->q_vectors, q->q_dtype, q->q_normalize, q->len_t, tile, mags);
	// The bound pass: the rows as stored (bf16), read back from the tile, in the format of the corpus's shadow with the
	// cells' constants behind them (vk_host::pack_bound_query)
	if (!bound_tile || !c->shadow || c->prec || q->len_t > VK_FAST_QUERY_LEN) return;
	std::vector<float> stored((size_t)q->len_t * d);
	for (int i = 0; i < q->len_t; i++)
		for (int k = 0; k < d; k++) {
			uint16_t b;
			memcpy(&b, &tile[(size_t)(k >> 5) * 1024 + (size_t)(((k & 31) >> 3) * 16 + i) * 16 + (size_t)(k & 7) * 2], 2);
			stored[(size_t)i * d + k] = bf16_to_f32(b);
		}
	vk_host::pack_bound_query(c->shadow_format, stored.data(), q->len_t, c->shadow_n, c->shadow_x, *bound_tile);
}

// The bound pass and its two rounds in place of the exact pass `p` over every slice: afterwards d_scores (and d_raw when
// p.raw) hold today's floats for every slice that can be among the kk best above sel_floor, and something below the kk-th best
// (-inf, or the exact score of a contender's neighbour in its group of four) everywhere else.  Records ev[2] right after the bound
// kernel: the peer's turn begins there.  smem_list: the dynamic LDS of the exact kernel with one wave per workgroup (group_list).
// gap_s, tail: general gaps with the flat tail wanted (bound_tail_wanted) -- the bound kernel scores under the caller's slice-gap table made
// flat beyond the K its unit was compiled with, an upper bound of the bound (vk_host::bound_tail_cost)
static int score_bounded(vk_corpus *c, const VkScoreParams &p, int grid, size_t smem, size_t smem_bound, size_t smem_list, int kk, float sel_floor,
	const vk_gap &gap_s, bool tail, vk_host_keep &keep, hipStream_t st, const uint64_t **d_sel) {
	*d_sel = nullptr;
	const int64_t n = c->n_entries;
	vk_corpus::bound_state &b = c->bp;
	const int64_t most = std::max<int64_t>(n / 16, kBoundRound2Floor);   // slices round 2 may rescore
	// Round 1 takes the M largest bounds, M >= 2 kk where a block of the selection holds that many.  THE largest, through the block
	// selection (sorts of 2,048 keys in LDS, a few stages): then theta >= (the kk-th largest bound) - slack >= (the kk-th best exact
	// score) - slack, whatever the order of the rows, which is what tests/test_gpu_bound_pass.py holds round 2 against.  (The wave
	// selection's last stage is one wave's serial work and starves beside the peer's bound pass: 1.4 ms where 0.16 ms were measured alone.)
	const int M = kk <= 32 ? 64 : kk <= 256 ? 512 : VK_MAX_MATCHES;
	int rc;
	if ((rc = c->d_ub.reserve((size_t)n + 8, &c->device_bytes))) return rc;
	if ((rc = c->d_bound_groups.reserve((size_t)std::max<int64_t>(most, kTopkChunk), &c->device_bytes))) return rc;
	if ((rc = c->d_bound_keys.reserve((size_t)2 * kTopkChunk, &c->device_bytes))) return rc;
	if ((rc = c->d_counter.reserve(4, &c->device_bytes))) return rc;
	VkScoreParams pb = p;
	const vk_host::shadow_format &sf = c->shadow_format;
	pb.tiles = c->shadow; pb.nk32 = sf.steps; pb.tail = 0; pb.tile_bytes = sf.tile_bytes(); pb.bound_bits = sf.bits; pb.bound_live = sf.live; pb.bound_compact = sf.compact;
	pb.q_mode3 = 0; pb.q_lds = 0; pb.qtile = c->d_qtile8; pb.scores = c->d_ub; pb.raw = nullptr;
	b.tail_k = 0;
	if (tail && (p.gap_mode == 3 || p.gap_mode == 6)) {
		const int rows = p.gap_mode == 3 ? 32 : 64, K = sf.bits == 6 ? vk_score_m8t_tail_k() : vk_score_m7t_tail_k();
		float w[65];
		for (int j = 0; j <= rows; j++) w[j] = gap_cost(gap_s, j);
		pb.gap_mode = p.gap_mode == 3 ? 8 : 9;
		pb.bound_tail_cost = vk_host::bound_tail_cost(w, K, rows);
		b.tail_k = K;
	}
	// the launch vk_launch_score_m9t hands to vk_score_local_kernel: asked here as it is asked there (vk_bound_pass_dp reports it)
	b.fast_dp = sf.bits == 6 && sf.compact && vk_score_m9f_takes(&pb) ? 1 : 0;
	VK_HIP(vk_launch_score(&pb, grid, smem_bound, st));
	VK_HIP(hipEventRecord(c->ev[2], st));
	c->ev2_recorded = true;
	b.ran = 1; b.queries++;
	VK_HIP(hipMemsetD32Async(static_cast<hipDeviceptr_t>(c->d_scores), (int)0xff800000u, (size_t)n, st));
	if (p.raw) VK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.raw), (int)0xff800000u, (size_t)n, st));
	VkScoreParams pl = p;
	pl.group_list = c->d_bound_groups;
	// round 1: their groups scored exactly; theta = the kk-th best of those exact scores (the floor when there
	// are fewer), which stays on the device: round 2 follows without a trip to the host
	const uint64_t *d_first = nullptr;
	if ((rc = select_blocks(c, sel_floor, M, st, &d_first, c->d_ub))) return rc;
	VK_HIP(vk_launch_key_groups(d_first, M, c->d_bound_groups, st));
	pl.n_list = M;
	VK_HIP(vk_launch_score(&pl, M, smem_list, st));
	uint64_t *d_exact = c->d_bound_keys, *d_best = c->d_bound_keys + kTopkChunk;
	VK_HIP(vk_launch_rekey(d_first, M, c->d_scores, sel_floor, d_exact, st));
	VK_HIP(vk_launch_topk_unsorted(d_exact, M, kk, d_best, st));   // (one block: its kk best, sorted)
	// round 2: every slice whose bound reaches theta (those of round 1 among them: the same floats again)
	VK_HIP(vk_launch_select_ge_key(c->d_ub, n, d_best + (kk - 1), sel_floor, c->d_keys[0], c->d_counter, (uint32_t)most, st));
	uint32_t &count = *keep.array<uint32_t>(1);
	VK_HIP(hipMemcpyAsync(&count, c->d_counter, 4, hipMemcpyDeviceToHost, st));
	VK_HIP(hipStreamSynchronize(st));
	b.round1 = M;
	bool fell = false;
	if ((int64_t)count > most) {
		fell = true;   // the bounds do not separate the contenders: the exact pass over every slice, as without a shadow
		VK_HIP(vk_launch_score(&p, grid, smem, st));
	} else if (count > 0) {
		VK_HIP(vk_launch_key_groups(c->d_keys[0], (int32_t)count, c->d_bound_groups, st));
		pl.n_list = (int32_t)count;
		VK_HIP(vk_launch_score(&pl, (int32_t)count, smem_list, st));
	}
	if (!fell && count <= (uint32_t)kTopkChunk) {
		// the kk best are among the slices of round 2 (a slice that reaches theta has a bound that does): selected from those keys by one
		// block -- the same keys in the same order as the selection over every row's score gives
		VK_HIP(vk_launch_rekey(c->d_keys[0], (int32_t)count, c->d_scores, sel_floor, d_exact, st));
		VK_HIP(vk_launch_topk_unsorted(d_exact, (int32_t)count, kk, d_best, st));
		*d_sel = d_best;
	}
	b.round2 = count;
	if (!fell) b.survivors += count;
	b.fell_back = fell ? 1 : 0;
	if (fell) b.fallbacks++;
	// most of the last eight bound passes fell back: the next 64 queries go without one (worst case)
	if (bound_pass_mode() == 0) b.backoff.record(fell);
	b.pruned = !fell;
	b.full = p; b.full_grid = grid; b.full_smem = smem;
	return VK_OK;
}

// One query of at most VK_MAX_QUERY_LEN tokens: what every stage reads, filled once (route(), prepare()) in the order of the members,
// and the stages over it.  The parameter structs `p` and `wp` are built once, by prepare(); a launch that differs from them
// (the multi-block kernel, the fused launch's carve-up, a pass's work list and state) works on a copy.  Every host buffer that is the
// source or the destination of an asynchronous copy lives in `keep`, which the entry point (vk_query below) owns: when a stage returns
// an error with copies still in flight, the entry point synchronises the stream before the buffers die (vk_guard.h).
struct query_run {
	vk_corpus_t *c; const vk_query_desc *q; vk_topk_out *out;
	vk_host_keep &keep; hipStream_t st;
	vk_host::route_switches sw; vk_host::route_facts facts; vk_host::query_route r;
	int bound_mode = 0;
	int64_t n = 0;           // rows of the slice table (== n_sentences unless long slices were padded)
	int k = 0, kk = 0;       // max_matches; the size of the selection (known before the scoring pass: the bound pass prunes against it)
	float sel_floor = 0.0f; int nq = 0;
	bool is_static = false, is_align = false, do_flow = false, canon_tr = false;
	bool only = false;       // state the listed slices: no scoring pass, no selection
	int64_t table_stride = 0; const int32_t *to_slice = nullptr;
	float qmags[VK_MAX_QUERY_LEN] = {0};
	float qmass_all[VK_MAX_QUERY_LEN] = {0};   // masses of the query tokens (transport algorithms), all 64 columns
	int32_t qkey_all[VK_MAX_QUERY_LEN];
	VkScoreParams p{};
	VkWideParams wp{};
	bool bounded = false;   // the scoring pass is the bound pass and its rounds (score_bounded)
	const uint64_t *d_sel_bounded = nullptr;   // ... which selected the kk best among their candidates already

	query_run(vk_corpus_t *c, const vk_query_desc *q, vk_topk_out *out, vk_host_keep &keep) : c(c), q(q), out(out), keep(keep), st(c->stream) {}

	// ---- the route: which kernels this query runs on, decided here and read by the stages (vk_route_host.h).  The bound pass may
	// take the query where the corpus has a shadow, VK_BOUND_PASS and the corpus's size allow it and the handle's back-off agrees
	int route() {
		sw = vk_host::read_route_switches();
		facts = route_facts_of(c, q, out);
		bound_mode = bound_pass_mode();
		facts.bound_pass = !facts.chained && c->shadow && bound_mode >= 0 && (bound_mode > 0 || c->desc.n_sentences >= kBoundPassMinSentences) && vk_host::bound_pass_takes(facts) &&
			(bound_mode != 0 || c->bp.backoff.take());
		r = vk_host::route_query(facts, sw, kRouteFits);
		if (r.status != VK_OK) return fail(r.status, r.message);
		const int64_t route_state[VK_QR_COUNT] = {r.plan, r.gap_mode, r.wide_gap_mode, r.score32_gap_mode, r.wave_tiles, r.pass[vk_host::CLASS_SHORT],
			r.pass[vk_host::CLASS_MID], r.pass[vk_host::CLASS_XLONG], r.list, r.ring_rows, r.flow, r.ostride, r.raw, r.span_skip_raw};
		memcpy(c->query_route, route_state, sizeof route_state);
		n = c->n_entries; k = q->max_matches; kk = facts.kk; nq = (q->len_t + 15) / 16;
		is_static = c->desc.layout == VK_LAYOUT_STATIC; is_align = q->algorithm == VK_ALG_ALIGN; only = q->only_slices != nullptr;
		table_stride = (int64_t)c->n_tiles * 16 * 16;
		to_slice = slice_of_row(c); do_flow = q->want_flow && is_align;
		// Relaxed word mover's distance: likewise -- the rows of the winners come back in the canonical arithmetic (vk_rows_kernel) and
		// the host restates each winner's score from them in the reference's order of operations (vk_transport_host.h): the scores of the
		// result set are the oracle's floats, whichever kernel ranked the slices (per query, batched GEMM, a shard of the corpus).
		canon_tr = q->algorithm == VK_ALG_RWMD && !q->wmd_full && q->want_flow && out->sim_rows != nullptr;
		// (a span similarity: admission is score > max(min_score, 0) -- its scores are no clipped cosines, NaN and negative values are no matches)
		sel_floor = c->span_sim.active() ? vk_host::span_sim_floor(q->min_score) : (do_flow || canon_tr) ? vk_host::restated_floor(q->min_score) : q->min_score;
		return VK_OK;
	}

	// what vk_wrd_exact_kernel / vk_rows_kernel need to restate the similarity rows of a slice (tag weights included)
	void fill_transport(VkWrdParams &w) const {
		corpus_fields_ids(w, c);
		w.table = c->d_table; w.table_stride = (int64_t)c->n_tiles * 16 * 16;
		w.qtile = c->d_qtile; w.nq = (q->len_t + 15) / 16; w.len_t = q->len_t; w.mag = c->d_mag;
		w.d = c->desc.d; w.q_ids = is_static ? (int32_t *)c->d_qids : nullptr;   // canonical similarity rows (sim_canon)
		tag_weight_fields(w, c, q, VK_MAX_QUERY_LEN);
		if (q->tag_weights && is_static && q->algorithm == VK_ALG_RWMD && q->q_tags && q->q_token_ids && c->d_tag && c->d_qbits) {
			// the cells upstream writes twice (static_vocab_fixup); d_qbits holds this query's bitmap (set before the scoring launch)
			w.tag_s = c->d_tag; w.qid_bits = c->d_qbits;
			for (int j = 0; j < VK_MAX_QUERY_LEN; j++)
				w.qkey[j] = (j < q->len_t && q->q_token_ids[j] >= 0 && q->q_token_ids[j] < c->desc.vocab_size) ? q->q_token_ids[j] * 256 + ((int32_t)q->q_tags[j] & 255) : -1;
		}
	}
	// the WRD parameter block of the exact solvers (listed slices, candidate rounds)
	void transport_params(VkWrdParams &w) const {
		fill_transport(w);
		w.mass_mode = q->algorithm == VK_ALG_WRD ? 0 : (q->rwmd_normalize_bow ? 1 : 2);
		memcpy(w.qmass, qmass_all, sizeof w.qmass);
		w.raw_masses = (q->algorithm == VK_ALG_WRD && !q->wrd_normalize_magnitudes) ? 1 : 0;
		w.boost = p.boost; w.raw_out = c->d_wrd_raw; w.val_out = c->d_wrd_val;
	}
	// transport algorithms: similarity rows (and, for exact transport, the optimal plan) of the winners, from which
	// the host states their SparseFlow / DenseFlow.  rows_idx: rows of the slice table, best first.
	// solver: an exact transport's parameter block (transport_params) -- the plans of the winners too
	int transport_flows(const std::vector<int64_t> &rows_idx, const VkWrdParams *solver = nullptr, float *rows_dst = nullptr) {
		const bool exact = solver != nullptr;
		if (!q->want_flow || !out->sim_rows || rows_idx.empty()) return VK_OK;
		if (!rows_dst) rows_dst = out->sim_rows;
		const int nqw = (q->len_t + 15) / 16, W = 16 * nqw;   // columns of a similarity row: the query length padded to 16
		const int R = out->rows_per_winner > 0 ? out->rows_per_winner : VK_FAST_SENT_LEN;   // rows per winner (longer winners: zero rows)
		if (R % 64 != 0 || R > VK_MAX_DOC_LEN + 1 || (exact && R > VK_MAX_SENT_LEN))
			return fail(VK_ERR_INVALID, "rows_per_winner must be a multiple of 64, at most VK_MAX_SENT_LEN (rows without plans: VK_MAX_DOC_LEN + 1)");
		int rc2;
		const int cnt = (int)rows_idx.size();
		const size_t need = (size_t)cnt * R * W;
		if ((rc2 = c->d_rows_out.reserve(need, &c->device_bytes))) return rc2;
		if ((rc2 = c->d_plan_out.reserve(need, &c->device_bytes))) return rc2;
		if ((rc2 = c->d_wrd_raw.reserve((size_t)VK_MAX_MATCHES, &c->device_bytes))) return rc2;
		if ((rc2 = c->d_wrd_val.reserve((size_t)VK_MAX_MATCHES, &c->device_bytes))) return rc2;
		std::vector<uint64_t> &hk = keep.vec<uint64_t>((size_t)cnt);
		for (int i = 0; i < cnt; i++) hk[(size_t)i] = vk_host::key_of_row(rows_idx[(size_t)i]);
		VK_HIP(hipMemcpyAsync(c->d_keys[1], hk.data(), hk.size() * 8, hipMemcpyHostToDevice, c->stream));
		VkWrdParams w{};
		fill_transport(w);
		w.keys = c->d_keys[1]; w.rows_out = c->d_rows_out; w.rows_len = R;
		if (R > VK_MAX_SENT_LEN) {   // rows of whole documents: one wave per 16 tokens of a winner (vk_canon_rows_kernel)
			VK_HIP(hipMemsetAsync(c->d_rows_out, 0, need * 4, c->stream));
			VK_HIP(vk_launch_canon_rows(&w, cnt, (c->max_len + 15) / 16 + 1, c->stream));
		} else VK_HIP(vk_launch_rows(&w, cnt, c->stream));
		VK_HIP(hipMemcpyAsync(rows_dst, c->d_rows_out, need * 4, hipMemcpyDeviceToHost, c->stream));
		if (exact && out->plan) {
			w.mass_mode = solver->mass_mode; w.raw_masses = solver->raw_masses;
			memcpy(w.qmass, solver->qmass, sizeof w.qmass);
			w.raw_out = c->d_wrd_raw; w.val_out = c->d_wrd_val; w.plan_out = c->d_plan_out;
			VK_HIP(hipMemsetAsync(c->d_plan_out, 0, need * 4, c->stream));   // a solver writes the columns of its winner's tokens only
			// (winners of 65 .. R tokens: the long solver restates their plans)
			if ((rc2 = launch_wrd_exact_both(c, w, cnt, nullptr, R > VK_FAST_SENT_LEN && c->max_len > VK_FAST_SENT_LEN, c->stream))) return rc2;
			VK_HIP(hipMemcpyAsync(out->plan, c->d_plan_out, need * 4, hipMemcpyDeviceToHost, c->stream));
		}
		VK_HIP(hipStreamSynchronize(c->stream));
		return VK_OK;
	}

	// masses of the query tokens (the transports) or the gap costs' form (alignments) into p
	void fill_masses() {
		if (q->algorithm == VK_ALG_WRD) {
			float sum_t = 0.0f;
			for (int j = 0; j < q->len_t; j++) sum_t += qmags[j];           // wrd.h:99-102, float sum in order
			const bool rawm = !q->wrd_normalize_magnitudes;   // wrd.h:99-102: masses stay the magnitudes
			for (int j = 0; j < VK_MAX_QUERY_LEN; j++) qmass_all[j] = j < q->len_t ? (rawm ? qmags[j] : qmags[j] / sum_t) : 0.0f;
			memcpy(p.qmass, qmass_all, sizeof p.qmass);
			p.wrd_raw_total = rawm ? sum_t : 0.0f;
			p.mag = c->d_mag;
		} else if (q->algorithm == VK_ALG_RWMD) {
			p.rwmd_symmetric = q->rwmd_symmetric;
			p.rwmd_normalize_bow = q->rwmd_normalize_bow;
			if (q->wmd_full) {
				p.wmd_bound = q->rwmd_normalize_bow ? 1 : 2;
				for (int j = 0; j < q->len_t; j++) qmass_all[j] = q->rwmd_normalize_bow ? 1.0f / (float)q->len_t : 1.0f;
			}
			else if (!q->rwmd_injective) {
				// 1:n form: masses of the query's vocabulary entries (count / len at the first occurrence of a token id)
				const bool ids = c->desc.layout == VK_LAYOUT_STATIC && q->q_token_ids;
				for (int j = 0; j < VK_MAX_QUERY_LEN; j++) {
					float mass = 0.0f;
					if (j < q->len_t) {
						int cnt = 1;
						bool first = true;
						// (tag-weighted with q_tags: the entries are (token id, tag) pairs, TaggedTokenFactory, bow.h:150-176)
						const bool tagged = q->tag_weights && q->q_tags;
						if (ids && q->q_token_ids[j] >= 0)
							for (int i = 0; i < q->len_t; i++)
								if (i != j && q->q_token_ids[i] == q->q_token_ids[j] && (!tagged || q->q_tags[i] == q->q_tags[j])) { cnt++; if (i < j) first = false; }
						mass = first ? (q->rwmd_normalize_bow ? (float)cnt / (float)q->len_t : (float)cnt) : 0.0f;
					}
					qmass_all[j] = mass;
				}
				memcpy(p.qmass, qmass_all, sizeof p.qmass);
				if (ids && q->tag_weights && q->q_tags) p.tag_s = c->d_tag;
			}
		} else gap_fields(p, facts.gaps);
	}
	// wp, where a pass or a traceback of the one-wave-per-slice family reads it (after p: it takes p's gap, tag and boost fields)
	void build_wide() {
		if (r.flow == vk_host::FLOW_NARROW && r.list == vk_host::LIST_NONE) return;
		corpus_fields_ids(wp, c);
		wp.table = c->d_table; wp.table_stride = table_stride; wp.n_sent = (int32_t)n;
		wp.qtile = c->d_qtile; wp.nq = nq; wp.len_t = q->len_t; wp.locality = q->locality; wp.max_len = c->max_len;
		wp.gap_mode = r.wide_gap_mode;
		wp.rwmd_symmetric = p.rwmd_symmetric; wp.rwmd_normalize_bow = p.rwmd_normalize_bow;
		gap_fields(wp, p);
		wp.ws = c->d_ws; wp.wt = c->d_wt; wp.wt0 = c->d_wt;
		wp.ws_tail = facts.ws_tail;   // the constant tail of w_s (a saturated table): from which k on
		tag_weight_fields(wp, c, q, VK_MAX_QUERY_LEN);
		wp.tag_s = p.tag_s; wp.qid_bits = p.qid_bits; wp.slices_overlap = p.slices_overlap; memcpy(wp.qkey, qkey_all, sizeof wp.qkey);
		wp.boost = p.boost; wp.scores = c->d_scores; wp.raw = r.raw ? (float *)c->d_raw : nullptr;
		wp.d = c->desc.d; wp.q_ids = is_static ? (int32_t *)c->d_qids : nullptr;   // FLOW: canonical similarity rows (sim_canon)
		if (r.plan != vk_host::PLAN_MULTI_BLOCK) return;
		// ... under the multi-block kernel: the masses of an exact transport's bound (stage 1) or of the 1:n form
		const bool exact = exact_transport(q);
		if (exact || r.score32_gap_mode == 7) memcpy(wp.qmass, qmass_all, sizeof wp.qmass);
		if (exact) {
			wp.mag = q->algorithm == VK_ALG_WRD ? c->d_mag : nullptr;
			wp.wrd_raw_total = p.wrd_raw_total; wp.wmd_bound = q->algorithm == VK_ALG_WRD ? 0 : p.wmd_bound;
		}
	}

	// ---- prepare: query tile, gap tables, boost, static table; the peer's turn; the parameter structs
	int prepare() {
		int rc;
		VK_HIP(hipEventRecord(c->ev[0], st));
		std::vector<uint8_t> &qtile = keep.vec<uint8_t>();
		bool bound_ok = r.plan == vk_host::PLAN_BOUNDED;   // ... unless a query row is not finite or a boost is negative (below)
		std::vector<uint8_t> &qtile8 = keep.vec<uint8_t>();
		vk_pack_query(c, q, qtile, qmags, bound_ok ? &qtile8 : nullptr);
		VK_HIP(hipMemcpyAsync(c->d_qtile, qtile.data(), qtile.size(), hipMemcpyHostToDevice, st));
		bound_ok = bound_ok && !qtile8.empty();
		if (bound_ok) {
			if ((rc = c->d_qtile8.reserve(qtile8.size(), &c->device_bytes))) return rc;
			VK_HIP(hipMemcpyAsync(c->d_qtile8, qtile8.data(), qtile8.size(), hipMemcpyHostToDevice, st));
		}

		// a span similarity beside the cosine: the query's row as given too -- q_normalize is the cosine tile's alone
		if (c->span_sim.sourced() && (rc = upload_source_query(c, q, keep, st))) return rc;

		const size_t n_ws = std::max<size_t>((size_t)kGapTable, (size_t)c->max_len + 2);   // w_s up to the longest slice
		std::vector<float> &ws = keep.vec<float>(n_ws);
		float *wt = keep.array<float>(160);   // wt[0..79]: w_t as given; wt[80..159]: its subadditive closure (vk_result_host.h)
		fill_masses();
		p.gap_mode = r.gap_mode;
		for (size_t i = 0; i < n_ws; i++) ws[i] = (is_align && (int64_t)i <= c->max_len) ? gap_cost(q->gap_s, (int)i) : 0.0f;
		if ((rc = c->d_ws.reserve(n_ws, &c->device_bytes))) return rc;
		vk_host::wt_with_closure(wt, q->gap_t, q->len_t, is_align);
		VK_HIP(hipMemcpyAsync(c->d_ws, ws.data(), n_ws * sizeof(float), hipMemcpyHostToDevice, st));
		VK_HIP(hipMemcpyAsync(c->d_wt, wt, 160 * sizeof(float), hipMemcpyHostToDevice, st));

		bool boost_nonneg = true;   // a score is monotone in its cells only under a boost >= 0: looked at where the boost is uploaded
		if (q->boost && (rc = upload_boost(c, q->boost, keep, st, bound_ok ? &boost_nonneg : nullptr))) return rc;
		bounded = bound_ok && boost_nonneg;   // the scoring pass will be the bound pass and its rounds

		if (is_static) {
			int32_t *ids = keep.array<int32_t>(80);
			for (int j = 0; j < 80; j++) ids[j] = (q->q_token_ids && j < q->len_t) ? q->q_token_ids[j] : -1;
			VK_HIP(hipMemcpyAsync(c->d_qids, ids, 80 * sizeof(int32_t), hipMemcpyHostToDevice, st));
			if ((rc = fill_query_tables(c, q, c->d_qtile, q->q_token_ids ? (const int32_t *)c->d_qids : nullptr, c->d_table, table_stride, only, keep, st))) return rc;
		}

		// handles on one corpus take turns: this scoring kernel starts when the peer's has finished (its selection and
		// traceback then run beside this kernel); the wait is on the device, the host does not block
		VK_HIP(hipEventRecord(c->ev[5], st));
		if ((rc = vk_wait_peer_turn(c, st))) return rc;
		VK_HIP(hipEventRecord(c->ev[1], st));
		corpus_fields_ids(p, c);
		p.table = c->d_table; p.n_sent = (int32_t)n;
		p.qtile = c->d_qtile; p.len_t = q->len_t; p.locality = q->locality;
		p.ws = c->d_ws; p.wt = c->d_wt + 80; p.wt0 = c->d_wt;
		p.boost = c->dev_boost(q->boost);
		p.scores = c->d_scores; p.raw = c->d_raw;
		tag_weight_fields(p, c, q, VK_FAST_QUERY_LEN);
		// vocabulary transports with tag weights over the static layout: the cells upstream writes twice (static_vocab_fixup,
		// vk_common.hip.h) -- needs the (id, tag) keys of both sides: q_tags and vk_corpus_set_token_tags
		for (int j = 0; j < VK_MAX_QUERY_LEN; j++) qkey_all[j] = -1;
		const bool vocab_fix = is_static && q->algorithm == VK_ALG_RWMD && q->tag_weights && q->q_tags && q->q_token_ids && c->d_tag && c->d_pos;
		if (vocab_fix) {
			const size_t words = ((size_t)c->desc.vocab_size + 31) / 32 + 1;
			if ((rc = c->d_qbits.reserve(words, &c->device_bytes))) return rc;
			std::vector<uint32_t> &bits = keep.vec<uint32_t>(words, 0u);
			for (int j = 0; j < q->len_t; j++) {
				const int32_t id = q->q_token_ids[j];
				if (id < 0 || id >= c->desc.vocab_size) continue;
				bits[(size_t)id >> 5] |= 1u << (id & 31);
				qkey_all[j] = id * 256 + ((int32_t)q->q_tags[j] & 255);
			}
			VK_HIP(hipMemcpyAsync(c->d_qbits, bits.data(), words * 4, hipMemcpyHostToDevice, st));
			VK_HIP(hipStreamSynchronize(st));   // `bits` leaves scope
			p.qid_bits = c->d_qbits; p.tag_s = c->d_tag; p.slices_overlap = c->overlapping ? 1 : 0;
			for (int j = 0; j < VK_FAST_QUERY_LEN; j++) p.qkey[j] = qkey_all[j];
		}
		build_wide();
		return VK_OK;
	}

	// The work list of a pass of the one-wave-per-slice family, longest first (wd.order): every non-empty row of the slice table (the
	// others carry no score: preset), the slices of more than 64 tokens, or those beyond VK_MAX_SENT_LEN -- built when first needed
	int wide_order(VkWideParams &wd, vk_host::route_list list) {
		const bool all = list == vk_host::LIST_ALL, apart = list == vk_host::LIST_APART;
		vk_devbuf<int32_t> &d_ord = all ? c->d_wide_order : apart ? c->d_apart_order : c->d_xlong_order;
		int32_t &n_ord = all ? c->n_wide_order : apart ? c->n_apart_order : c->n_xlong_order;
		if (n_ord < 0) {
			std::vector<int32_t> ord;
			if (all) { for (int64_t e = 0; e < n; e++) if ((*c->h_end)[(size_t)e] > (*c->h_start)[(size_t)e]) ord.push_back((int32_t)e); }
			else if (apart && c->h_apart) ord = *c->h_apart;
			else if (!apart && c->h_xlong) ord = *c->h_xlong;
			rows_longest_first(c, ord);
			if (int rcw = d_ord.reserve(ord.size() + 1, &c->device_bytes)) return rcw;
			VK_HIP(hipMemcpy(d_ord, ord.data(), ord.size() * 4, hipMemcpyHostToDevice));
			n_ord = (int32_t)ord.size();
		}
		wd.order = d_ord; wd.n_order = n_ord;
		if (all) {
			VK_HIP(hipMemsetD32Async(static_cast<hipDeviceptr_t>(c->d_scores), (int)0xff800000u, (size_t)n, st));
			if (wd.raw) VK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(wd.raw), (int)0xff800000u, (size_t)n, st));
		}
		return VK_OK;
	}
	// vk_wide_kernel's state for a scoring pass over the route's list (flow_k 0) or for flow_k tracebacks: in LDS where the route says
	// so, else one region of scratch per workgroup, sized here (with room for the records of the route's traceback kernel)
	int wide_state(VkWideParams &wd, int flow_k) {
		const bool flow = flow_k > 0;
		const vk_host::route_list list = flow ? vk_host::LIST_NONE : r.list;
		wd.scratch = nullptr; wd.scratch_stride = 0; wd.h_ring = 0; wd.order = nullptr; wd.n_order = 0;
		if (flow ? r.wide_lds_flow : r.wide_lds_score)
			return list == vk_host::LIST_APART || list == vk_host::LIST_XLONG ? wide_order(wd, list) : VK_OK;   // (state in LDS, but still only the long slices)
		wd.h_ring = r.ring_rows;   // a saturated gap table: the column history is a ring in LDS
		size_t per = vk_wide_scratch_bytes(c->max_len, nq, wd.gap_mode, flow, wd.h_ring);
		if (flow && r.flow == vk_host::FLOW_DOC) per = std::max(per, vk_doc_scratch_bytes(c->max_len, wd.gap_mode));   // (vk_doc_kernel's records of a winner)
		if (flow && r.flow == vk_host::FLOW_DOCW) per = std::max(per, vk_docw_scratch_bytes(c->max_len, nq));
		if (flow && r.flow == vk_host::FLOW_DOCG) per = std::max(per, vk_docg_scratch_bytes(c->max_len));
		const size_t blocks = (size_t)vk_wide_gs_blocks(c->max_len, nq, wd.gap_mode, flow_k, n, wd.h_ring);
		const size_t need = per * blocks;
		if (need > ((size_t)16 << 30)) return fail(VK_ERR_UNSUPPORTED, "traceback state of this many slices this long exceeds 16 GiB of scratch");
		if (int rcw = c->d_wide_scratch.reserve(need, &c->device_bytes)) return rcw;
		wd.scratch = c->d_wide_scratch; wd.scratch_stride = (int64_t)per;
		return list != vk_host::LIST_NONE ? wide_order(wd, list) : VK_OK;
	}
	// the doc / docw / docg / wide pass over the route's list
	int list_pass() {
		VkWideParams wd = wp;
		const vk_host::route_pass pass = r.wide_pass;
		if (int rcw = (pass == vk_host::PASS_WIDE || pass == vk_host::PASS_DOC) ? wide_state(wd, 0) : wide_order(wd, r.list)) return rcw;
		if (wd.order && wd.n_order == 0) return VK_OK;
		if (pass == vk_host::PASS_DOCW) VK_HIP(vk_launch_docw(&wd, 0, st));
		else if (pass == vk_host::PASS_DOCG) VK_HIP(vk_launch_docg(&wd, 0, st));
		else if (pass == vk_host::PASS_DOC) VK_HIP(vk_launch_doc(&wd, 0, st));
		else VK_HIP(vk_launch_wide(&wd, 0, st));
		return VK_OK;
	}

	// a query of 17 .. 64 tokens: the multi-block kernel over the slices of at most 64 tokens (17 .. 32 tokens: two column blocks;
	// 33 .. 64: one slice per wave and four), then a pass of their own over the slices it skips
	int score_multi_block() {
		VkWideParams mb = wp;   // (the kernels of the one-wave-per-slice family know gap modes 0 / 1 / 2 / 4 and walk the caller's w_t: wp's)
		mb.gap_mode = r.score32_gap_mode;
		if (r.wide_gap_mode == 2) mb.wt = c->d_wt + 80;   // register history of 32 / 64 rows, closure of w_t
		VK_HIP(vk_launch_score32(&mb, r.wave_tiles, st));
		if (r.pass[vk_host::CLASS_MID] == vk_host::PASS_LONG_RWMD_FILL) VK_HIP(vk_launch_long_rwmd_fill(&mb, c->d_long_groups, c->n_long_groups, (int32_t)n, st));
		else if (r.pass[vk_host::CLASS_MID] == vk_host::PASS_LONG_BOUND) {
			// exact transport over a corpus with long slices: the multi-block kernel skips them (their groups are padded, vk_corpus.cpp)
			VkWrdParams lw{};
			fill_transport(lw);
			lw.mag = q->algorithm == VK_ALG_WRD ? c->d_mag : nullptr;
			memcpy(lw.qmass, qmass_all, sizeof lw.qmass);
			lw.wrd_raw_total = p.wrd_raw_total; lw.wmd_bound = wp.wmd_bound;
			lw.group_list = c->d_long_groups; lw.n_list = c->n_long_groups; lw.n_entries = (int32_t)n;
			lw.scores = c->d_scores; lw.raw = c->d_raw; lw.boost = p.boost;
			VK_HIP(vk_launch_long_bound(&lw, st));
		}
		return r.wide_pass != vk_host::PASS_NONE ? list_pass() : VK_OK;
	}
	// span-embedding index: one vector per slice, one query vector -> the clipped cosine is the local alignment score.
	// The aligner scores are written only if something reads them: the traceback kernel restates those of the winners, and
	// without a booster the score IS the aligner score ((raw / 1) * 1)
	int score_span() {
		if (!c->span_sim.active()) {
			VkScoreParams ps = p;
			if (r.span_skip_raw) ps.raw = nullptr;
			VK_HIP(vk_launch_span(&ps, st));
			return VK_OK;
		}
		// ... under a span similarity: the score is ops(src(span, q)), unclipped; no raw array (vk_validate_query has
		// refused boosters, so r.span_skip_raw holds: the aligner score of a winner is its score)
		VkSpanSimParams sp{};
		sp.src = c->span_sim.src; sp.ops = c->span_sim.ops;
		sp.tiles = c->d_tiles; sp.qtile = c->d_qtile; sp.tile_bytes = c->tile_bytes; sp.nk32 = c->nk32; sp.tail = c->tail; sp.prec = c->prec;
		sp.n = n; sp.scores = c->d_scores;
		if (c->span_sim.sourced()) {
			if (!c->raw_rows) return fail(VK_ERR_STATE, "span similarity beside the cosine without the copy of the unmodified rows");
			// the query's row as the caller gives it (uploaded with the query tile, above) and sum_k |q_k|, as the table kernel's
			std::vector<float> &qrow = keep.vec<float>((size_t)c->desc.d);
			for (int kf = 0; kf < c->desc.d; kf++)
				qrow[(size_t)kf] = q->q_dtype == VK_F32 ? ((const float *)q->q_vectors)[kf] : bf16_to_f32(((const uint16_t *)q->q_vectors)[kf]);
			sp.raw_tiles = *c->raw_rows; sp.raw_tile_bytes = c->raw_tile_bytes; sp.d = c->desc.d;
			sp.q_row = c->d_qraw; sp.q_abs_sum = vk_host::sim_src_abs_sum(qrow.data(), c->desc.d);
		}
		VK_HIP(vk_launch_span_sim(&sp, st));
		return VK_OK;
	}
	// the fused kernel over the slices of at most 64 tokens (or the bound pass and its rounds in its place), its long-slice pass and the
	// route's pass over longer slices: the one place that carves up the fused launch's LDS
	int score_fused() {
		int rc;
		VkScoreParams f = p;
		f.max_short_len = VK_FAST_SENT_LEN;
		// the aligner scores of all slices: read by the submatch bound and, without traceback, for the winners; with traceback the
		// flow kernel restates those of the winners
		// (exact transport: the solver states them); a second output array costs the stream 1 % (2.90 -> 2.87 ms per 1 M x 32 x 300-d)
		if (!r.raw) f.raw = nullptr;
		f.s_rows_per_wave = is_static ? (c->max_group_tokens + 15) / 16 * 16 : c->max_group_tiles * 16;
		f.h_rows = c->max_short_len + 1;
		const int lt = q->len_t <= 4 ? 4 : q->len_t <= 8 ? 8 : q->len_t <= 12 ? 12 : 16;   // strip rows hold the padded query columns (launch_score_lt)
		int lds_floats = f.s_rows_per_wave * lt + 16;
		if (f.gap_mode == 2) lds_floats += 4 * f.h_rows * 16;   // column history of dp_general
		f.m_rows = (c->max_short_len + 4) / 4 * 4;
		if (f.gap_mode == 7) lds_floats += 4 * f.m_rows;       // vocabulary masses of the 4 slices (static layout)
		f.lds_floats_per_wave = lds_floats;
		size_t smem = (size_t)lds_floats * 4 * 4;   // 4 waves per block
		// 300-d rows with general gaps (register history): the register form of the kernel takes 160 VGPRs, three waves per SIMD
		// leave 32, and the traceback kernel of the previous query has to wait until this kernel has drained (2.3 - 2.8 ms); with
		// the query tile in LDS the kernel takes 136 and runs at the same speed, the neighbours beside it.
		// Linear / affine gaps take 112 registers in the register form.  VK_QREG=1 / VK_QLDS=1 force one or the other.
		// Under an operator chain every width takes the generic tile form (MODE 10 / 11 / 12): no specialised query tile
		const bool reg_history = f.gap_mode == 3 || f.gap_mode == 6;
		const bool chained = facts.chained;
		if (!chained && !is_static && c->prec == 0 && c->nk32 == 10 && c->tail == 1)
			f.q_mode3 = sw.qlds ? 1 : sw.qreg ? 0 : (reg_history ? 1 : 0);
		if (!chained && !is_static && c->prec == 1 && c->nk32 == 19 && !sw.no_f32_special) f.q_mode3 = 1;   // fp32 rows at 300-d: MODE 4 (all 19 blocks of a tile in flight)
		const size_t qlds = (!chained && !is_static && ((c->prec == 0 && c->nk32 == 24 && c->tail == 0) || f.q_mode3)) ? (size_t)c->nk32 * 1024 : 0;   // MODE 3 / 4: query tile in LDS
		smem += qlds;
		// the generic contextual kernel (MODE 1: fp32 tiles, or a d without a specialised form) stages the query tile in LDS when it fits
		// beside the strips of at least two workgroups per CU
		if (!is_static && qlds == 0 && (chained || !(c->prec == 0 && c->nk32 == 10 && c->tail == 1))) {
			const size_t qb = ((size_t)c->tile_bytes + 1023) / 1024 * 1024;
			if (2 * (smem + qb) <= 160 * 1024 && !sw.no_qlds1) { f.q_lds = (int32_t)qb; smem += qb; }
		}
		if (smem > 160 * 1024) return fail(VK_ERR_UNSUPPORTED, "LDS demand exceeds 160 KiB per workgroup");
		const int64_t n_groups = (n + 3) / 4;
		const int grid = (int)std::min<int64_t>((n_groups + 3) / 4, (int64_t)1 << 20);   // capped to residency by the launcher
		// the 8-bit bound pass and exact scores of the contenders only, or the exact pass over every slice
		if (!bounded && r.plan == vk_host::PLAN_BOUNDED) c->query_route[VK_QR_PLAN] = vk_host::PLAN_FUSED;
		if (bounded) {
			// the bound kernel: the four waves' strips as above, and in place of the exact kernel's query tile the 8-bit one with the
			// cells' constants behind it -- the region MODE 7 of vk_score_kernel steps over (NK32 KiB + VK_DEV_BOUND_CONST_BYTES)
			const size_t smem_strips = smem - qlds - (size_t)f.q_lds;
			// (MODE 8: the 6-bit query tile, VK_DEV_FP6_QTILE_BYTES)
			const size_t smem_bound = smem_strips + (size_t)c->shadow_format.qtile_bytes() + VK_DEV_BOUND_CONST_BYTES;
			// the exact kernel over a group_list: one wave per workgroup, its strip and the exact query tile
			const size_t smem_list = (size_t)lds_floats * 4 + qlds + (size_t)f.q_lds;
			if ((rc = score_bounded(c, f, grid, smem, smem_bound, smem_list, kk, sel_floor, q->gap_s, bound_tail_wanted(bound_mode), keep, st, &d_sel_bounded))) return rc;
		} else if (r.plan != vk_host::PLAN_LISTED) VK_HIP(vk_launch_score(&f, grid, smem, st));
		if (r.pass[vk_host::CLASS_MID] == vk_host::PASS_FUSED_LONG) {
			// slices longer than VK_FAST_SENT_LEN: one per wave, one wave per workgroup, LDS strip for the longest;
			// general gaps take the LDS-history form (the four DPP rows share one history: only row 0 is active)
			VkScoreParams pl = f;
			pl.group_list = c->d_long_groups; pl.n_list = c->n_long_groups;
			if (pl.gap_mode == 3 || pl.gap_mode == 6) pl.gap_mode = 2;
			pl.s_rows_per_wave = is_static ? (c->long_group_tokens + 15) / 16 * 16 : c->long_group_tiles * 16;
			pl.h_rows = 0;
			int lf = pl.s_rows_per_wave * lt + 16;
			if (pl.gap_mode == 2) lf += (c->max_long_len + 1) * 16;
			pl.m_rows = 0;
			if (pl.gap_mode == 7) lf += (c->max_long_len + 4) / 4 * 4;
			pl.lds_floats_per_wave = lf;
			const size_t smem_l = (size_t)lf * 4 + qlds + (size_t)pl.q_lds;
			if (smem_l > 160 * 1024) return fail(VK_ERR_UNSUPPORTED, "LDS demand of the long-slice pass exceeds 160 KiB");
			VK_HIP(vk_launch_score(&pl, c->n_long_groups, smem_l, st));
		}
		// slices beyond VK_MAX_SENT_LEN (whole documents), or every slice of more than 64 tokens: one wave per slice, longest first
		// (linear / affine gaps: the skewed sweep of vk_doc_kernel -- no in-row dependency, a fifth of the time per row; round 4)
		if (r.wide_pass != vk_host::PASS_NONE && (rc = list_pass())) return rc;
		return VK_OK;
	}
	int score() {
		switch (r.plan) {
		case vk_host::PLAN_MULTI_BLOCK: return score_multi_block();
		// (the multi-block kernel does not take this query or this corpus: every slice on the one-wave-per-slice family)
		case vk_host::PLAN_DOCW_ALL: case vk_host::PLAN_DOCG_ALL: case vk_host::PLAN_WIDE_ALL: return list_pass();
		case vk_host::PLAN_SPAN: return score_span();
		default: return q->len_t <= VK_FAST_QUERY_LEN ? score_fused() : VK_OK;   // (listed slices under a query of 17 .. 64 tokens: no pass)
		}
	}

	// ---- only_slices: the listed slices solved exactly, in the caller's order (no bound pass ran, nothing is pruned)
	int listed_transports() {
		const int cnt = q->n_only;
		if (int rc = c->d_wrd_raw.reserve((size_t)VK_MAX_MATCHES, &c->device_bytes)) return rc;
		if (int rc = c->d_wrd_val.reserve((size_t)VK_MAX_MATCHES, &c->device_bytes)) return rc;
		const uint64_t *hk = nullptr;
		if (int rc = upload_listed_keys(c, q, keep, st, false, &hk)) return rc;
		std::vector<int64_t> rows_idx((size_t)cnt);
		for (int i = 0; i < cnt; i++) rows_idx[(size_t)i] = (int64_t)vk_host::key_row(hk[i]);
		VkWrdParams w{};
		transport_params(w);
		w.keys = c->d_keys[0];
		VK_HIP(hipMemsetAsync(c->d_wrd_raw, 0xff, (size_t)cnt * 4, st));   // NaN: a slice no solver takes (empty) stays marked
		VK_HIP(hipMemsetAsync(c->d_wrd_val, 0xff, (size_t)cnt * 4, st));
		if (int rc = launch_wrd_exact_both(c, w, cnt, nullptr, c->max_len > VK_FAST_SENT_LEN, st)) return rc;
		std::vector<float> &vals = keep.vec<float>((size_t)cnt), &raws = keep.vec<float>((size_t)cnt);
		VK_HIP(hipMemcpyAsync(vals.data(), c->d_wrd_val, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
		VK_HIP(hipMemcpyAsync(raws.data(), c->d_wrd_raw, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
		VK_HIP(hipStreamSynchronize(st));
		if (int rc = transport_flows(rows_idx, &w)) return rc;
		vk_host::selected sel;
		sel.keys = hk; sel.cap = cnt; sel.slice_of_row = to_slice;
		vk_host::result_set rs;
		vk_host::score_selected(sel, rs, q->min_score, cnt, true, [&](int i) {   // (an empty slice: no solver took it)
			const bool empty = (*c->h_end)[(size_t)rows_idx[(size_t)i]] - (*c->h_start)[(size_t)rows_idx[(size_t)i]] < 1;
			return empty ? std::make_pair(-INFINITY, -INFINITY) : std::make_pair(raws[(size_t)i], vals[(size_t)i]);
		});
		vk_host::write_result_set(out, sel, rs, q->len_t, true);
		return VK_OK;
	}

	// ---- stage 2 of an exact transport: exact EMD on the candidates with the largest bounds, until the k-th best
	// exact score is above every remaining bound (then no unsolved sentence can enter)
	int transport_rounds() {
		VK_HIP(hipEventRecord(c->ev[2], st));
		if (sw.wrd_turns) c->ev2_recorded = true;   // experiment: bound passes take turns like the alignment kernels
		// (no turn-taking between handles here: ev2_recorded stays unset.  Two bound passes sharing the chip, each with its
		// long epilogue, fill each other's gaps: 336 M pairs/s with three handles against 302 M/s when they queue)
		// Round 1: the M largest bounds.  Its k-th best exact score theta prunes: every row whose bound is below
		// theta is out; all others are solved in one launch (round 2), which then fills the GPU instead of a
		// trickle of M-candidate rounds.
		const int M = 512;
		const size_t cap = ((size_t)((n + kTopkChunk - 1) / kTopkChunk) + 1) * VK_MAX_MATCHES;   // keys d_keys[0] holds
		if (int rc = c->d_wrd_raw.reserve(cap, &c->device_bytes)) return rc;
		if (int rc = c->d_wrd_val.reserve(cap, &c->device_bytes)) return rc;
		if (int rc = c->d_counter.reserve(4, &c->device_bytes)) return rc;
		std::vector<vk_host::candidate> best, round;
		std::vector<uint64_t> &keys = keep.vec<uint64_t>();
		std::vector<float> &vals = keep.vec<float>(), &raws = keep.vec<float>();
		VkWrdParams w{};
		transport_params(w);
		// solves the `count` candidates whose keys sit at d_keys, merges them into `best`; ub_last: the smallest bound among them, n_cand: how many
		float ub_last = INFINITY;
		int n_cand = 0;
		auto solve = [&](const uint64_t *d_keys, int count) -> int {
			w.keys = d_keys;
			if (int rc3 = launch_wrd_exact_both(c, w, count, c->d_scores, c->max_len > VK_FAST_SENT_LEN, st)) return rc3;   // (long: candidates of 65 .. 512 tokens)
			keys.resize((size_t)count); vals.resize((size_t)count); raws.resize((size_t)count);
			VK_HIP(hipMemcpyAsync(keys.data(), d_keys, (size_t)count * 8, hipMemcpyDeviceToHost, st));
			VK_HIP(hipMemcpyAsync(vals.data(), c->d_wrd_val, (size_t)count * 4, hipMemcpyDeviceToHost, st));
			VK_HIP(hipMemcpyAsync(raws.data(), c->d_wrd_raw, (size_t)count * 4, hipMemcpyDeviceToHost, st));
			VK_HIP(hipStreamSynchronize(st));
			n_cand = vk_host::count_keys(keys.data(), count);
			ub_last = INFINITY;
			for (int i = 0; i < n_cand; i++) {
				ub_last = std::min(ub_last, vk_host::key_score(keys[(size_t)i]));
				round.push_back({vals[(size_t)i], raws[(size_t)i], (int64_t)vk_host::key_row(keys[(size_t)i]), {}, {}});
			}
			vk_host::keep_best(best, round, q->min_score, k);
			return VK_OK;
		};
		const uint64_t *d_first = nullptr;
		if (int rc = select_blocks(c, q->min_score, M, st, &d_first)) return rc;
		if (int rc = solve(d_first, M)) return rc;
		bool done = n_cand < M || ((int)best.size() == k && best.back().val > ub_last);
		while (!done) {
			const float theta = (int)best.size() == k ? best.back().val : -INFINITY;
			VK_HIP(vk_launch_select_ge(c->d_scores, n, theta, q->min_score, c->d_keys[0], c->d_counter, (uint32_t)cap, st));
			uint32_t &count = *keep.array<uint32_t>(1);
			VK_HIP(hipMemcpyAsync(&count, c->d_counter, 4, hipMemcpyDeviceToHost, st));
			VK_HIP(hipStreamSynchronize(st));
			if (count == 0) break;
			if (sw.debug_candidates) fprintf(stderr, "[vk] exact transport: round 2 solves %u candidates (theta %.6f, n %lld)\n", count, theta, (long long)n);
			const int take = (int)std::min<size_t>(count, cap);
			if (int rc = solve(c->d_keys[0], take)) return rc;
			done = (size_t)count <= cap;   // every row that could still enter has been solved
		}
		VK_HIP(hipEventRecord(c->ev[3], st));
		std::vector<int64_t> rows_idx;
		for (const vk_host::candidate &b : best) rows_idx.push_back(b.row);
		if (int rc = transport_flows(rows_idx, &w)) return rc;
		VK_HIP(hipEventRecord(c->ev[4], st));
		VK_HIP(hipStreamSynchronize(st));
		vk_host::write_best(out, best, to_slice, q->len_t, q->want_flow != 0);
		state_timings(c, false);
		return VK_OK;
	}

	// ---- flow (traceback) of `count` slices named by device keys: narrow or wide kernel
	int launch_flow(const uint64_t *d_keys, int count) {
		if (r.flow != vk_host::FLOW_NARROW) {   // the one-wave-per-slice family: VkWideParams
			VkWideParams wd = wp;
			wd.keys = d_keys; wd.raw_out = c->d_out_raw; wd.mapping = c->d_out_map; wd.edge_sim = c->d_out_sim;
			if (int rcw = wide_state(wd, count)) return rcw;
			wd.dp_rows = nullptr; wd.dp_rows_len = 0;
			if (c->max_len > VK_MAX_SENT_LEN || r.flow != vk_host::FLOW_WIDE) {
				// Long winners: their similarities (canonical arithmetic, tag weights applied) restated beforehand by one wave per 16
				// tokens, so that the serial sweep of a winner is its recurrence alone (5,000 tokens: 8.4 ms of a 12 ms query were the
				// sweep restating 313 tiles one after the other; 3.6 ms since).  Within 2 GiB; else the sweep restates them itself.
				const int R = (c->max_len + 63) / 64 * 64, Wq = 16 * nq;
				const size_t need = (size_t)count * R * Wq;
				if (need * 4 <= ((size_t)2 << 30)) {
					if (int rcw = c->d_rows_out.reserve(need, &c->device_bytes)) return rcw;
					if (int rcw = c->d_plan_out.reserve(need, &c->device_bytes)) return rcw;
					VkWrdParams w{};
					fill_transport(w);
					w.keys = d_keys; w.rows_out = c->d_rows_out; w.rows_len = R;
					VK_HIP(hipMemsetAsync(c->d_rows_out, 0, need * 4, st));
					VK_HIP(vk_launch_canon_rows(&w, count, (c->max_len + 15) / 16 + 1, st));
					wd.dp_rows = c->d_rows_out; wd.dp_rows_len = R;
				}
			}
			// (the route's kernel where its rows and scratch came about, else vk_wide_kernel)
			if (r.flow == vk_host::FLOW_DOCW && wd.dp_rows && wd.scratch && wd.scratch_stride >= (int64_t)vk_docw_scratch_bytes(c->max_len, nq)) VK_HIP(vk_launch_docw(&wd, count, st));
			else if (r.flow == vk_host::FLOW_DOCG && wd.dp_rows && wd.scratch && wd.scratch_stride >= (int64_t)vk_docg_scratch_bytes(c->max_len)) VK_HIP(vk_launch_docg(&wd, count, st));
			else if (r.flow == vk_host::FLOW_DOC && wd.dp_rows && wd.scratch && wd.scratch_stride >= (int64_t)vk_doc_scratch_bytes(c->max_len, wd.gap_mode)) VK_HIP(vk_launch_doc(&wd, count, st));
			else VK_HIP(vk_launch_wide(&wd, count, st));
			return VK_OK;
		}
		VkFlowParams f{};
		corpus_fields_ids(f, c);
		f.table = c->d_table;
		f.qtile = c->d_qtile; f.len_t = q->len_t; f.locality = q->locality; f.gap_mode = (p.gap_mode == 3 || p.gap_mode == 6) ? 2 : p.gap_mode;
		f.max_len = c->max_len;
		gap_fields(f, p);
		f.ws = c->d_ws; f.wt = c->d_wt;
		f.pos_s = p.pos_s; f.tw_keep = p.tw_keep; f.tw_threshold = p.tw_threshold;
		memcpy(f.tw, p.tw, sizeof f.tw);
		memcpy(f.tpos, p.tpos, sizeof f.tpos);
		f.d = c->desc.d; f.q_ids = is_static ? (int32_t *)c->d_qids : nullptr;   // canonical similarity rows (sim_canon)
		f.keys = d_keys; f.raw_out = c->d_out_raw; f.mapping = c->d_out_map; f.edge_sim = c->d_out_sim;
		VK_HIP(vk_launch_flow(&f, count, st));
		return VK_OK;
	}

	// ---- submatch_weight: bound from raw, then exact scores of the candidates from their tracebacks, until the
	// k-th best exact score is above every remaining bound (vk_submatch_bound_kernel)
	int submatch_rounds() {
		const int ostride = r.ostride;
		VK_HIP(hipEventRecord(c->ev[2], st));
		c->ev2_recorded = true;
		const float wsub = q->submatch_weight, total = p.ref_total;
		const float m_star = total * (1.0f - powf(1.0f / (wsub + 1.0f), 1.0f / wsub));
		VK_HIP(vk_launch_submatch_bound(c->d_raw, p.boost, n, total, wsub, m_star, c->d_scores, st));
		const int M = 512;
		std::vector<vk_host::candidate> best, round;
		selected_host got(keep, c, M, ostride, true);   // (the next round overwrites the buffers a round's candidates came back in)
		const vk_host::selected &cand = got.sel;
		vk_host::result_set scored;
		for (;;) {
			const uint64_t *d_cand = nullptr;
			if (int rc = select_blocks(c, q->min_score, M, st, &d_cand)) return rc;
			if (int rc = launch_flow(d_cand, M)) return rc;
			VK_HIP(vk_launch_mark(d_cand, M, c->d_scores, st));
			if (int rc = fetch_selected(d_cand, c->d_out_raw, c->d_out_map, c->d_out_sim, got, st)) return rc;
			// the round's candidates above min_score, with their tracebacks (the next round overwrites the buffers they came back in)
			vk_host::score_selected(cand, scored, q->min_score, M, false, vk_host::by_traceback{cand, q->len_t, q->tag_weights, total, wsub, q->boost});
			const int n_cand = (int)scored.val.size();
			const float ub_last = n_cand > 0 ? vk_host::key_score(got.keys[(size_t)n_cand - 1]) : INFINITY;   // the smallest bound among them
			for (const int i : scored.order)
				round.push_back({scored.val[(size_t)i], scored.raw[(size_t)i], cand.row(i), {got.map.begin() + (size_t)i * ostride, got.map.begin() + (size_t)i * ostride + q->len_t},
					{got.sim.begin() + (size_t)i * ostride, got.sim.begin() + (size_t)i * ostride + q->len_t}});
			vk_host::keep_best(best, round, q->min_score, k);
			if (n_cand < M) break;
			if ((int)best.size() == k && best.back().val > ub_last) break;
		}
		VK_HIP(hipEventRecord(c->ev[3], st));
		VK_HIP(hipEventRecord(c->ev[4], st));
		VK_HIP(hipStreamSynchronize(st));
		vk_host::write_best(out, best, to_slice, q->len_t, q->want_flow != 0);
		if (out->sim_rows && !best.empty()) {   // similarity rows of the winners on request (debug hook)
			std::vector<int64_t> rows_idx;
			for (const vk_host::candidate &b : best) rows_idx.push_back(b.row);
			if (int rc = transport_flows(rows_idx)) return rc;
		}
		state_timings(c, false);
		return VK_OK;
	}

	// The relaxed word mover's distance of the n_sel selected slices restated on the host from their similarity rows (*rows_all: rows_R
	// x rows_W floats per slice, in the handle's pinned staging -- a std::vector made the copy of a document corpus's winners, 12 MB for
	// 18 x 5,056 rows x 32 columns, go through the runtime's bounce buffers: 2 - 4 ms of a 5.7 ms query)
	int score_relaxed(const vk_host::selected &sel, selected_host &got, int n_sel, int limit, vk_host::result_set &rs) {
		const int rows_R = out->rows_per_winner > 0 ? out->rows_per_winner : VK_FAST_SENT_LEN, rows_W = 16 * nq;
		const size_t rows_bytes = (size_t)n_sel * rows_R * rows_W * 4;
		if (int rc = c->h_brows.reserve(rows_bytes / 4, nullptr)) return rc;
		float *const rows_all = c->h_brows;
		std::vector<int64_t> rows_idx;
		for (int i = 0; i < n_sel; i++) rows_idx.push_back(sel.row(i));
		if (int rc = transport_flows(rows_idx, nullptr, rows_all)) return rc;
		// vocabulary keys (static layout): token ids, or (id, tag) pairs when the similarity is tag-weighted (alignment/bow.h:106-127, 150-176)
		const bool vocab = is_static && q->q_token_ids && c->h_tok;
		const bool tagged = vocab && q->tag_weights && q->q_tags && c->h_tag;
		std::vector<int32_t> key_t((size_t)q->len_t), key_s;
		for (int j = 0; vocab && j < q->len_t; j++) key_t[(size_t)j] = tagged ? q->q_token_ids[j] * 256 + (int32_t)(uint8_t)q->q_tags[j] : q->q_token_ids[j];
		const float total = ref_total_of(q);
		// no rows for a slice that is empty or longer than the caller's room: it keeps the scoring pass's values (listed: no scoring pass
		// ran -- an empty slice has no score, a longer one cannot be stated)
		const auto len_of = [&](int i) { return (*c->h_end)[(size_t)rows_idx[(size_t)i]] - (*c->h_start)[(size_t)rows_idx[(size_t)i]]; };
		for (int i = 0; i < n_sel && !only; i++)
			if (len_of(i) < 1 || len_of(i) > rows_R) VK_HIP(hipMemcpy(&got.raw[(size_t)i], c->d_raw + rows_idx[(size_t)i], 4, hipMemcpyDeviceToHost));
		vk_host::score_selected(sel, rs, q->min_score, limit, only, [&](int i) -> std::pair<float, float> {
			const int32_t t_a = (*c->h_start)[(size_t)rows_idx[(size_t)i]], len_s = len_of(i);
			if (len_s < 1 || len_s > rows_R) {
				const float none = len_s < 1 ? -INFINITY : NAN;
				return only ? std::make_pair(none, none) : std::make_pair(got.raw[(size_t)i], vk_host::key_score(sel.keys[i]));
			}
			if (vocab) {
				key_s.resize((size_t)len_s);
				for (int u = 0; u < len_s; u++)
					key_s[(size_t)u] = tagged ? (*c->h_tok)[(size_t)(t_a + u)] * 256 + (int32_t)(uint8_t)(*c->h_tag)[(size_t)(t_a + u)] : (*c->h_tok)[(size_t)(t_a + u)];
			}
			const float raw_i = vk_host::rwmd_from_rows(rows_all + (size_t)i * rows_R * rows_W, rows_W, len_s, q->len_t,
				vocab ? key_s.data() : nullptr, vocab ? key_t.data() : nullptr, q->rwmd_injective != 0, q->rwmd_symmetric != 0, q->rwmd_normalize_bow != 0);
			// reference_score with every query token matched: the sum of the weights (match.h:165-176)
			return {raw_i, (raw_i / total) * (q->boost ? q->boost[sel.slice(i)] : 1.0f)};
		});
		for (int i = 0; i < rs.n_out; i++)   // the rows of the winners, in their final order
			memcpy(out->sim_rows + (size_t)i * rows_R * rows_W, rows_all + (size_t)rs.order[(size_t)i] * rows_R * rows_W, (size_t)rows_R * rows_W * 4);
		return VK_OK;
	}

	// ---- the selected result set: selection, tracebacks, winners to the host, their scores, rows on request
	int selected_result() {
		int rc;
		if (!bounded) VK_HIP(hipEventRecord(c->ev[2], st));   // (a pruned query recorded it after its bound pass)
		c->ev2_recorded = true;
		const bool rows_on_request = out->sim_rows != nullptr;   // alignments: similarity rows of the winners only on request (debug hook)
		// Alignments with traceback: the scores of the scoring pass rest on MFMA cosines and differ from the oracle's in the last
		// bits; the flow kernel restates every winner in the canonical arithmetic (aligner score, mapping, edge similarities: the
		// oracle's, bit for bit).  So that the result SET is the oracle's too, a few runners-up are retraced with the winners
		// (kCanonMargin more slices; the floor of the selection is lowered by the rounding slack likewise) and the k best canonical
		// scores are kept: exact unless more than kCanonMargin slices sit within rounding (~2e-6) of the k-th score.
		const uint64_t *d_sel = nullptr;   // the selected keys on the device, best first
		// the winners' device arrays: grown to this result set
		if ((rc = c->d_out_raw.reserve((size_t)kk, &c->device_bytes))) return rc;
		if ((rc = c->d_out_sim.reserve((size_t)kk * 64, &c->device_bytes))) return rc;
		if ((rc = c->d_out_map.reserve((size_t)kk * 64, &c->device_bytes))) return rc;
		// ... the listed slices' keys, every row's sorted, the bound pass's, or a selection's
		if (only) {
			if ((rc = upload_listed_keys(c, q, keep, st, true))) return rc;
			d_sel = c->d_keys[0];
		} else if (kk > VK_MAX_MATCHES) {
			// more matches than the block selection keeps per 2,048 keys: the keys of all n rows, sorted
			if ((rc = c->d_sort[0].reserve((size_t)n + 64, &c->device_bytes))) return rc;
			if ((rc = c->d_sort[1].reserve((size_t)n + 64, &c->device_bytes))) return rc;
			size_t temp_bytes = 0;
			uint64_t *sorted = nullptr;
			VK_HIP(vk_launch_sort_all(nullptr, n, sel_floor, c->d_sort[0], c->d_sort[1], nullptr, &temp_bytes, &sorted, st));
			if ((rc = c->d_sort_temp.reserve(temp_bytes, &c->device_bytes))) return rc;
			VK_HIP(vk_launch_sort_all(c->d_scores, n, sel_floor, c->d_sort[0], c->d_sort[1], c->d_sort_temp, &temp_bytes, &sorted, st));
			d_sel = sorted;
		} else if (d_sel_bounded) d_sel = d_sel_bounded;
		else if ((rc = kk <= 64 ? select_waves(c, sel_floor, kk, st, &d_sel) : select_blocks(c, sel_floor, kk, st, &d_sel))) return rc;

		// ---- flow of the winners ------------------------------------------------
		VK_HIP(hipEventRecord(c->ev[3], st));
		if (do_flow && (rc = launch_flow(d_sel, kk))) return rc;
		VK_HIP(hipEventRecord(c->ev[4], st));

		// ---- results to host ------------------------------------------------------
		selected_host got(keep, c, kk, r.ostride, do_flow);
		vk_host::selected &sel = got.sel;
		if ((rc = fetch_selected(d_sel, c->d_out_raw, c->d_out_map, c->d_out_sim, got, st))) return rc;
		const int n_sel = vk_host::count_keys(sel.keys, kk), limit = only ? q->n_only : k;   // (n_sel: the rows below are fetched before anything is scored)
		vk_host::result_set rs;
		// the winners' scores from their canonical aligner scores (searches with a submatch weight take the candidate rounds above)
		if (do_flow) vk_host::score_selected(sel, rs, q->min_score, limit, only, vk_host::by_traceback{sel, q->len_t, q->tag_weights, p.ref_total, only ? q->submatch_weight : 0.0f, q->boost});
		else if (!(canon_tr && n_sel > 0)) {
			// the aligner scores of the winners from the scoring pass's array (a large result set: the whole array in one copy); the span
			// pass that wrote none: the score itself
			if (out->raw_score && n_sel > 0 && !r.span_skip_raw) {
				if ((rc = gather_raw(c, sel, n_sel, 256, got, keep, st))) return rc;
				sel.raw = got.raw.data();
			}
			vk_host::score_selected(sel, rs, q->min_score, kk, only);
		}
		if (canon_tr && n_sel > 0 && (rc = score_relaxed(sel, got, n_sel, limit, rs))) return rc;   // (and their similarity rows)
		vk_host::write_result_set(out, sel, rs, q->len_t, q->want_flow != 0);
		c->have_scores = !only;
		if (!canon_tr && (q->algorithm == VK_ALG_RWMD || (is_align && rows_on_request)) && rs.n_out > 0) {
			std::vector<int64_t> rows_idx;
			for (int i = 0; i < rs.n_out; i++) rows_idx.push_back(sel.row(rs.order[(size_t)i]));
			if ((rc = transport_flows(rows_idx))) return rc;
		}

		state_timings(c, true);
		return VK_OK;
	}
};

// One query: the handle's per-query state reset, queries of more than 64 tokens handed on, then the stages and one of the four exits
static int query_body(vk_corpus_t *c, const vk_query_desc *q, vk_topk_out *out, vk_host_keep &keep) {
	VK_HIP(hipSetDevice(c->device));
	c->bp.pruned = false; c->bp.ran = c->bp.round1 = c->bp.round2 = c->bp.fell_back = c->bp.tail_k = c->bp.fast_dp = 0;
	for (int64_t &x : c->query_route) x = -1;
	if (q->len_t > VK_MAX_QUERY_LEN) return vk_longq_query(c, q, out, keep);   // 65 .. 512 tokens (vk_longq_host.cpp)
	out->n_out = 0;
	c->have_scores = false;
	if (c->n_entries == 0) return VK_OK;
	query_run run(c, q, out, keep);
	int rc;
	if ((rc = run.route()) || (rc = run.prepare()) || (rc = run.score())) return rc;
	if (exact_transport(q)) return run.only ? run.listed_transports() : run.transport_rounds();
	if (run.is_align && q->submatch_weight != 0.0f && !run.only) return run.submatch_rounds();
	return run.selected_result();
}

extern "C" {

int vk_query(vk_corpus_t *c, const vk_query_desc *q, vk_topk_out *out) {
	// the rows vk_corpus_set_query_operand left belong to this query, however it ends (a batch run query by query drops its own)
	struct consume { vk_corpus_t *c; ~consume() { if (c && !c->in_batch) c->drop_query_operands(); } } consumed{c};
	// a query without a boost of its own runs under the handle's resident one (vk_corpus_set_saliency), as if it had passed that array
	vk_query_desc q_res;
	if (c && q && !q->boost && c->resident_boost()) { q_res = *q; q_res.boost = c->resident_boost(); q = &q_res; }
	const int rc = vk_validate_query(c, q, out);
	if (rc) return rc;
	if (q->abort && *q->abort) { out->n_out = 0; return fail(VK_ERR_ABORTED, "query aborted by the caller"); }
	// Under an operator chain (vk_corpus_set_sim_ops, vk_corpus_set_contextual_sim_ops) the winners of an alignment are restated in the canonical arithmetic whether
	// or not the caller wants their tracebacks: an operator such as THRESHOLD makes a score discontinuous in its cells, so the sums of
	// the scoring pass (matrix pipe order) state no score to within a rounding error as they do for the plain cosine.  The query runs
	// with tracebacks into arrays of its own; the caller's mapping / edge_sim stay untouched, as without a chain.
	vk_query_desc q_flow;
	vk_topk_out out_flow;
	std::vector<int16_t> own_map;
	std::vector<float> own_sim;
	bool restate = false;
	// (A source that is not the cosine or a combinator, chain or none: likewise.  The table's cell is the canonical cell there, but the scoring
	// kernels' sums over a slice are not stated to be the tracebacks' sums.)
	if ((c->sim_ops.n > 0 || c->table_is_canonical()) && q->algorithm == VK_ALG_ALIGN && !q->want_flow && !q->only_slices && q->submatch_weight == 0.0f) {
		q_flow = *q; q_flow.want_flow = 1;
		out_flow = *out;
		own_map.assign((size_t)out->capacity * (size_t)q->len_t, (int16_t)-1);
		own_sim.assign((size_t)out->capacity * (size_t)q->len_t, 0.0f);
		out_flow.mapping = own_map.data(); out_flow.edge_sim = own_sim.data();
		restate = vk_validate_query(c, &q_flow, &out_flow) == VK_OK;   // (a result set too large to retrace stays on the scoring pass's scores)
	}
	const vk_query_desc *q_run = restate ? &q_flow : q;
	vk_topk_out *out_run = restate ? &out_flow : out;
	// an error inside the body leaves no copy in flight behind: the stream is drained before the body's host buffers die
	const int rc2 = vk_run_guarded([&](vk_host_keep &keep) { return query_body(c, q_run, out_run, keep); },
		[&]() { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); },
		[](const char *what) { return fail(VK_ERR_INVALID, std::string("vk_query: ") + what); });
	if (restate) out->n_out = out_flow.n_out;
	return rc2;
}

int vk_merge_topk(const vk_topk_out *sets, int32_t n_sets, int32_t len_t, int32_t max_matches, vk_topk_out *out) {
	if (!sets || !out || n_sets < 0) return fail(VK_ERR_INVALID, "null argument");
	if (max_matches < 1 || out->capacity < max_matches) return fail(VK_ERR_INVALID, "output capacity smaller than max_matches");
	struct Ref { float score; int64_t sent; int set, idx; };
	std::vector<Ref> all;
	// (a NaN score -- records arrive from other ranks unchecked -- would break the strict weak order std::sort needs: it ranks last,
	// as -inf; the kernels never produce one, degenerate vectors score 0)
	for (int s = 0; s < n_sets; s++)
		for (int i = 0; i < sets[s].n_out; i++) all.push_back({sets[s].score[i] == sets[s].score[i] ? sets[s].score[i] : -INFINITY, sets[s].sentence[i], s, i});
	std::sort(all.begin(), all.end(), [](const Ref &a, const Ref &b) { return vk_host::ranks_before(a.score, a.sent, b.score, b.sent); });
	const int n_out = (int)std::min<size_t>(all.size(), (size_t)max_matches);
	for (int i = 0; i < n_out; i++) {
		const Ref &r = all[(size_t)i];
		const vk_topk_out &src = sets[r.set];
		vk_host::write_winner(out, i, len_t, r.score, r.sent, src.raw_score ? src.raw_score[r.idx] : 0.0f, nullptr, nullptr, false);
		vk_host::merge_rows(out, i, len_t, src.mapping ? src.mapping + (size_t)r.idx * len_t : nullptr, src.edge_sim ? src.edge_sim + (size_t)r.idx * len_t : nullptr);
	}
	out->n_out = n_out;
	return VK_OK;
}

int vk_rwmd_from_rows(const float *S, int32_t ld, int32_t len_s, int32_t len_t, const int32_t *key_s, const int32_t *key_t,
	int32_t injective, int32_t symmetric, int32_t normalize_bow, float *score_out) {
	if (!S || !score_out) return fail(VK_ERR_INVALID, "null argument");
	if (len_s < 0 || len_t < 0 || ld < len_t) return fail(VK_ERR_INVALID, "rows narrower than the query");
	if ((key_s == nullptr) != (key_t == nullptr)) return fail(VK_ERR_INVALID, "vocabulary keys for both sides or for neither");
	if (symmetric && !normalize_bow) return fail(VK_ERR_INVALID, "the symmetric relaxed WMD needs normalised bags of words (alignment/wmd.h:441-449)");
	*score_out = vk_host::rwmd_from_rows(S, ld, len_s, len_t, key_s, key_t, injective != 0, symmetric != 0, normalize_bow != 0);
	return VK_OK;
}

static inline int record_w(int len_t) { return (std::max(1, len_t) + 15) / 16 * 16; }

int32_t vk_record_words(int32_t len_t) {
	const int w = record_w(len_t);
	return (5 + w / 2 + w + 3) / 4 * 4;
}

int vk_pack_records(const vk_topk_out *set, int32_t len_t, int32_t k, int64_t sentence_offset, int32_t *records) {
	if (!set || !records || k < 0 || len_t < 1) return fail(VK_ERR_INVALID, "null argument");
	if (set->n_out > k) return fail(VK_ERR_INVALID, "result set larger than k records");
	const int w = record_w(len_t), words = vk_record_words(len_t);
	memset(records, 0, (size_t)k * words * 4);
	for (int i = 0; i < set->n_out; i++) {
		int32_t *r = records + (size_t)i * words;
		r[0] = 1;
		memcpy(r + 1, set->score + i, 4);
		if (set->raw_score) memcpy(r + 2, set->raw_score + i, 4);
		const int64_t g = set->sentence[i] + sentence_offset;
		memcpy(r + 3, &g, 8);
		int16_t *m = (int16_t *)(r + 5);
		for (int j = 0; j < w; j++) m[j] = -1;
		if (set->mapping) memcpy(m, set->mapping + (size_t)i * len_t, (size_t)len_t * 2);
		if (set->edge_sim) memcpy(r + 5 + w / 2, set->edge_sim + (size_t)i * len_t, (size_t)len_t * 4);
	}
	return VK_OK;
}

int vk_merge_records(const int32_t *records, int32_t n_sets, int32_t len_t, int32_t k, vk_topk_out *out) {
	if (!records || !out || n_sets < 0 || k < 1 || len_t < 1) return fail(VK_ERR_INVALID, "null argument");
	if (out->capacity < k) return fail(VK_ERR_INVALID, "output capacity smaller than k");
	const int w = record_w(len_t), words = vk_record_words(len_t);
	struct Ref { float score; int64_t sent; const int32_t *rec; };
	std::vector<Ref> all;
	all.reserve((size_t)n_sets * k);
	for (size_t i = 0; i < (size_t)n_sets * k; i++) {
		const int32_t *r = records + i * words;
		if (!r[0]) continue;
		Ref e;
		memcpy(&e.score, r + 1, 4);
		if (e.score != e.score) e.score = -INFINITY;   // NaN ranks last (see vk_merge_topk): a strict weak order whatever arrives
		memcpy(&e.sent, r + 3, 8);
		e.rec = r;
		all.push_back(e);
	}
	// the order of vk_merge_topk (and of the selection on one GPU): score descending, ties by slice index descending
	std::sort(all.begin(), all.end(), [](const Ref &a, const Ref &b) { return vk_host::ranks_before(a.score, a.sent, b.score, b.sent); });
	const int n_out = (int)std::min<size_t>(all.size(), (size_t)k);
	for (int i = 0; i < n_out; i++) {
		const int32_t *r = all[(size_t)i].rec;
		float raw;
		memcpy(&raw, r + 2, 4);
		vk_host::write_winner(out, i, len_t, all[(size_t)i].score, all[(size_t)i].sent, raw, nullptr, nullptr, false);
		vk_host::merge_rows(out, i, len_t, (const int16_t *)(r + 5), (const float *)(r + 5 + w / 2));
	}
	out->n_out = n_out;
	return VK_OK;
}

} // extern "C"
