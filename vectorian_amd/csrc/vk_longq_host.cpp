// vk_longq_host.cpp -- C-ABI: alignments of queries of 65 .. VK_MAX_LONG_QUERY_LEN tokens (vk_longq_kernel: roles swapped, one wave
// per slice, anti-diagonal sweep).  Called by vk_query's body for such queries; the same stages as there -- scoring pass over all
// slices (MFMA similarities), selection of k + 8, canonical retrace of those, the k best returned -- with buffers of their own.
// A corpus that holds slices of 65 .. VK_MAX_SENT_LEN tokens: the scoring pass leaves them at -inf and a second launch, the kernel's
// block form over the list of those rows, overwrites that; the winners all go through the block form.
// No CPU compute fallback exists.

#include "vk_internal.h"
#include "vk_guard.h"
#include "vk_longq_host.h"

int vk_longq_query(vk_corpus_t *c, const vk_query_desc *q, vk_topk_out *out, vk_host_keep &keep) {
	int rc = VK_OK;
	hipStream_t st = c->stream;
	const int64_t n = c->n_entries;
	const int k = q->max_matches, LT = q->len_t, nq = (LT + 15) / 16, LTP = 16 * nq;
	const bool only = q->only_slices != nullptr;
	const bool is_static = c->desc.layout == VK_LAYOUT_STATIC;
	auto &lq = c->lq;
	out->n_out = 0;
	c->have_scores = false;
	if (n == 0) return VK_OK;

	// ---- prepare: query tiles, gap tables, tag weights, token ids, static tables
	VK_HIP(hipEventRecord(c->ev[0], st));
	std::vector<uint8_t> &qtile = keep.vec<uint8_t>();
	std::vector<float> &qmags = keep.vec<float>((size_t)LTP);
	vk_pack_query(c, q, qtile, qmags.data());
	if ((rc = lq.qt.reserve((size_t)nq * c->tile_bytes, &c->device_bytes))) return rc;
	VK_HIP(hipMemcpyAsync(lq.qt, qtile.data(), qtile.size(), hipMemcpyHostToDevice, st));

	VkLongqParams p{};
	const vk_host::gap_form g = vk_host::classify_gaps(q->gap_s, q->gap_t);
	p.gap_mode = g.gap_mode;
	gap_fields(p, g);
	// slices of more than 64 tokens (at most VK_MAX_SENT_LEN: vk_validate_query): the block form takes them, `short_len` is the longest
	// slice of the pass over the others
	const bool blocks = c->max_len > VK_FAST_SENT_LEN;
	const int short_len = blocks ? c->max_short_len : c->max_len;
	// one host block for the small per-query arrays: w_s[0 .. longest slice + pad] (at least [0 .. 64 + pad]), w_t[0 .. LT], tag
	// weights, POS codes, token ids
	const size_t n_ws = blocks ? ((size_t)c->max_len + 63) / 64 * 64 + 16 : 80, n_wt = (size_t)LT + 16;
	std::vector<float> &fl = keep.vec<float>(n_ws + n_wt + (size_t)LTP);
	std::vector<int32_t> &il = keep.vec<int32_t>(2 * (size_t)LTP);
	for (size_t i = 0; i < n_ws; i++) fl[i] = (int)i <= c->max_len ? gap_cost(q->gap_s, (int)i) : 0.0f;
	for (size_t i = 0; i < n_wt; i++) fl[n_ws + i] = (int)i <= LT ? gap_cost(q->gap_t, (int)i) : 0.0f;
	float total = (float)LT;
	if (q->tag_weights) {
		total = 0.0f;
		for (int j = 0; j < LT; j++) total += q->tag_weights[j];
	}
	for (int j = 0; j < LTP; j++) {
		fl[n_ws + n_wt + j] = (q->tag_weights && j < LT) ? q->tag_weights[j] : 0.0f;
		il[(size_t)j] = (q->tag_weights && j < LT) ? (int32_t)q->q_pos[j] : -1;
		il[(size_t)LTP + j] = (q->q_token_ids && j < LT) ? q->q_token_ids[j] : -1;
	}
	if ((rc = lq.fl.reserve(fl.size(), &c->device_bytes))) return rc;
	if ((rc = lq.il.reserve(il.size(), &c->device_bytes))) return rc;
	VK_HIP(hipMemcpyAsync(lq.fl, fl.data(), fl.size() * 4, hipMemcpyHostToDevice, st));
	VK_HIP(hipMemcpyAsync(lq.il, il.data(), il.size() * 4, hipMemcpyHostToDevice, st));

	if (q->boost && (rc = upload_boost(c, q->boost, keep, st))) return rc;
	const int64_t table_stride = (int64_t)c->n_tiles * 16 * 16;
	if (is_static) {   // (where the table's cell is the canonical cell the tracebacks read the tables: listed slices need them too)
		if (!only || c->table_is_canonical())
			if ((rc = lq.table.reserve((size_t)nq * (size_t)table_stride, &c->device_bytes))) return rc;
		if ((rc = fill_query_tables(c, q, lq.qt, q->q_token_ids ? (const int32_t *)lq.il + LTP : nullptr, lq.table, table_stride, only, keep, st))) return rc;
	}

	corpus_fields_ids(p, c);
	p.table = lq.table; p.table_stride = table_stride; p.n_sent = (int32_t)n;
	p.qtile = lq.qt; p.nq = nq; p.len_t = LT; p.locality = q->locality; p.s_stride = vk_longq_stride(short_len);
	p.ws = lq.fl; p.wt = lq.fl + n_ws;
	if (q->tag_weights) {
		p.pos_s = c->d_pos; p.tw = lq.fl + n_ws + n_wt; p.tpos = lq.il;
		p.tw_keep = 1.0f - q->pos_mismatch_penalty; p.tw_threshold = q->similarity_threshold;
	}
	p.ref_total = total;
	p.boost = c->dev_boost(q->boost);
	p.scores = c->d_scores; p.raw = q->want_flow ? nullptr : (float *)c->d_raw;   // with traceback the retrace restates the winners' aligner scores
	p.d = c->desc.d; p.q_ids = is_static ? lq.il + LTP : nullptr;

	// ---- the scoring pass (handles on one corpus take turns, as in vk_query)
	VK_HIP(hipEventRecord(c->ev[5], st));
	if ((rc = vk_wait_peer_turn(c, st))) return rc;
	VK_HIP(hipEventRecord(c->ev[1], st));
	if (!only) {
		if (p.gap_mode == 2) {
			// the constant tail of w_t (a saturated table): from which k on
			int kt_ = LT;
			while (kt_ > 1 && fl[n_ws + (size_t)kt_ - 1] == fl[n_ws + (size_t)LT]) kt_--;
			if (kt_ < LT) p.wt_tail = kt_;
			if (!vk_longq_hm_in_lds(LT, short_len)) {   // the matrix of the scans: in LDS behind the strip where it fits, else a region per workgroup
				const size_t per = vk_longq_scratch_bytes(LT, 2, 0, 0);
				if ((rc = lq.scratch.reserve(per * (size_t)vk_longq_blocks(LT, short_len, n, 0), &c->device_bytes))) return rc;
				p.scratch = lq.scratch; p.scratch_stride = (int64_t)per;
			}
		}
		VK_HIP(vk_launch_longq(&p, 0, st));
		if (blocks) {
			// ... then the rows it left at -inf, longest first (the list follows the slice table: built when first needed)
			if (lq.n_order < 0) {
				std::vector<int32_t> ord;
				for (int32_t e : *c->h_apart) if ((*c->h_end)[(size_t)e] - (*c->h_start)[(size_t)e] > VK_FAST_SENT_LEN) ord.push_back(e);
				rows_longest_first(c, ord);
				if ((rc = lq.order.reserve(ord.size() + 1, &c->device_bytes))) return rc;
				VK_HIP(hipMemcpyAsync(lq.order, ord.data(), ord.size() * 4, hipMemcpyHostToDevice, st));
				VK_HIP(hipStreamSynchronize(st));
				lq.n_order = (int32_t)ord.size();
			}
			VkLongqParams b = p;
			const vk_host::longq_geometry geo = vk_host::longq_geometry_of(LT, c->max_len, p.gap_mode, false, false);
			b.s_stride = geo.s_stride; b.order = lq.order; b.n_order = lq.n_order; b.dm_off = (int64_t)geo.dm_off; b.su_off = (int64_t)geo.su_off;
			b.scratch = nullptr; b.scratch_stride = 0;
			if (p.gap_mode == 2) {
				if ((rc = lq.bscratch.reserve(geo.scratch_bytes * (size_t)vk_longq_blocks_grid(LT, c->max_len, 2, 0, lq.n_order), &c->device_bytes))) return rc;
				b.scratch = lq.bscratch; b.scratch_stride = (int64_t)geo.scratch_bytes;
			}
			VK_HIP(vk_launch_longq_blocks(&b, c->max_len, 0, st));
		}
	}
	VK_HIP(hipEventRecord(c->ev[2], st));
	c->ev2_recorded = true;

	// ---- bounded result set: k + kCanonMargin slices selected, all of them retraced canonically, the k best kept (vk_result_host.h)
	const bool do_flow = q->want_flow != 0;
	const int kk = only ? q->n_only : (int)std::min<int64_t>(do_flow ? std::min(k + vk_host::kCanonMargin, VK_MAX_MATCHES) : k, n);
	const float sel_floor = do_flow ? vk_host::restated_floor(q->min_score) : q->min_score;
	const uint64_t *d_sel = c->d_keys[0];   // the selected keys on the device, best first
	if (only) {
		if ((rc = upload_listed_keys(c, q, keep, st, false))) return rc;   // (the fetch below synchronises)
	} else if ((rc = kk <= 64 ? select_waves(c, sel_floor, kk, st, &d_sel) : select_blocks(c, sel_floor, kk, st, &d_sel))) return rc;
	VK_HIP(hipEventRecord(c->ev[3], st));

	// ---- the winners' tracebacks
	if (do_flow) {
		// a scratch region per workgroup: one per winner, the block form at most vk_host::kLongqFlowGrid of them (MBs each)
		const vk_host::longq_geometry geo = vk_host::longq_geometry_of(LT, blocks ? c->max_len : VK_FAST_SENT_LEN, p.gap_mode, true, q->tag_weights != nullptr);
		const size_t per = geo.scratch_bytes;
		if ((rc = lq.fscratch.reserve(per * (size_t)(blocks ? vk_longq_blocks_grid(LT, c->max_len, p.gap_mode, kk, kk) : kk), &c->device_bytes))) return rc;
		if ((rc = lq.raw.reserve((size_t)kk, &c->device_bytes))) return rc;
		if ((rc = lq.map.reserve((size_t)kk * LTP, &c->device_bytes))) return rc;
		if ((rc = lq.sim.reserve((size_t)kk * LTP, &c->device_bytes))) return rc;
		VkLongqParams f = p;
		f.wt_tail = 0;   // (the tracebacks meet every candidate, in the oracle's order)
		f.keys = d_sel; f.n_keys = kk; f.raw_out = lq.raw; f.mapping = lq.map; f.edge_sim = lq.sim; f.out_stride = LTP;
		f.scratch = lq.fscratch; f.scratch_stride = (int64_t)per;
		if (blocks) {
			f.s_stride = geo.s_stride; f.dm_off = (int64_t)geo.dm_off; f.su_off = (int64_t)geo.su_off;
			VK_HIP(vk_launch_longq_blocks(&f, c->max_len, kk, st));
		} else VK_HIP(vk_launch_longq(&f, kk, st));
	}
	VK_HIP(hipEventRecord(c->ev[4], st));

	// ---- results to the host
	selected_host got(keep, c, kk, LTP, do_flow);
	vk_host::selected &sel = got.sel;
	if ((rc = fetch_selected(d_sel, lq.raw, lq.map, lq.sim, got, st))) return rc;
	vk_host::result_set rs;
	// the winners' scores from their canonical aligner scores (no submatch weight with such queries)
	if (do_flow) vk_host::score_selected(sel, rs, q->min_score, only ? q->n_only : k, only, vk_host::by_traceback{sel, LT, q->tag_weights, total, 0.0f, q->boost});
	else if (vk_host::score_selected(sel, rs, q->min_score, kk, only) > 0 && out->raw_score) {
		if ((rc = gather_raw(c, sel, rs.n_out, 0, got, keep, st))) return rc;   // (always the whole array)
		std::copy(got.raw.begin(), got.raw.begin() + rs.n_out, rs.raw.begin());
	}
	vk_host::write_result_set(out, sel, rs, LT, do_flow);
	c->have_scores = !only;

	state_timings(c, true);
	return VK_OK;
}
