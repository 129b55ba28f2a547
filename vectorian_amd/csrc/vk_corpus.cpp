// vk_corpus.cpp -- C-ABI (include/vectorian_hip.h): library state, corpus handles and their residency in HBM.
// No CPU compute fallback exists: without a HIP device every entry point that
// would compute returns VK_ERR_NO_DEVICE / VK_ERR_HIP.

#include "vk_internal.h"
#include "vk_pool_host.h"
#include "vk_saliency_host.h"

#include <functional>

static_assert(vk_host::kSalMaxSignals == VK_MAX_SIGNALS && vk_host::SAL_FILTER_MAX == VK_SIGNAL_FILTER_MAX && vk_host::SAL_FILTER_CONV == VK_SIGNAL_FILTER_CONV, "vk_saliency_host.h and the C-ABI");
static_assert(vk_host::POOL_MEAN == VK_POOL_MEAN && vk_host::POOL_MIN == VK_POOL_MIN && vk_host::POOL_MAX == VK_POOL_MAX, "vk_pool_host.h and the C-ABI");
static_assert(vk_host::POOL_INVALID == VK_ERR_INVALID && vk_host::POOL_UNSUPPORTED == VK_ERR_UNSUPPORTED, "vk_pool_host.h and the C-ABI");

std::string &vk_error_slot() {
	static thread_local std::string err;
	return err;
}

std::mutex &vk_ring_mutex() {
	static std::mutex mu;
	return mu;
}

void vk_devblock::release(void *p) {
	if (!p) return;
	{
		std::lock_guard<std::mutex> g(mu);
		ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), p), ptrs.end());
	}
	(void)hipFree(p);
}

vk_devblock::~vk_devblock() {
	(void)hipSetDevice(device);
	for (void *p : ptrs) if (p) (void)hipFree(p);
}

// vk_devbuf.h's allocator: device memory, or pinned host memory for staging
int vk_devbuf_alloc(void **p, size_t bytes, bool pinned) {
	if (pinned) VK_HIP(hipHostMalloc(p, bytes, hipHostMallocDefault));
	else VK_HIP(hipMalloc(p, bytes));
	return VK_OK;
}

void vk_devbuf_free(void *p, bool pinned) {
	if (pinned) (void)hipHostFree(p);
	else (void)hipFree(p);   // synchronises the device: a query before may still be reading the workspace
}

// The workspaces every handle starts with: the query's tiles and small tables, the winners' outputs (grown on demand by the queries)
static int reserve_query_workspaces(vk_corpus *c) {
	int rc;
	int64_t *live = &c->device_bytes;
	if (c->desc.layout == VK_LAYOUT_STATIC && (rc = c->d_table.reserve((size_t)c->n_tiles * 16 * 16 * 4, live))) return rc;   // one [V_pad x 16] table per query tile
	if ((rc = c->d_qtile.reserve((size_t)c->tile_bytes * 4, live))) return rc;   // up to 4 tiles of 16 query rows
	if ((rc = c->d_ws.reserve(kGapTable, live))) return rc;
	if ((rc = c->d_wt.reserve(160, live))) return rc;
	if ((rc = c->d_qids.reserve(80, live))) return rc;
	if ((rc = c->d_out_raw.reserve(VK_MAX_MATCHES, live))) return rc;
	if ((rc = c->d_out_sim.reserve((size_t)VK_MAX_MATCHES * 64, live))) return rc;
	return c->d_out_map.reserve((size_t)VK_MAX_MATCHES * 64, live);
}

// ... and those sized by the slice table: scores of every row, keys of the block selection
static int reserve_table_workspaces(vk_corpus *c, int64_t n_entries) {
	int rc;
	int64_t *live = &c->device_bytes;
	if ((rc = c->d_scores.reserve((size_t)n_entries + 8, live))) return rc;
	if ((rc = c->d_raw.reserve((size_t)n_entries + 8, live))) return rc;
	const size_t nblk = (size_t)((n_entries + kTopkChunk - 1) / kTopkChunk) + 1;
	if ((rc = c->d_keys[0].reserve(nblk * VK_MAX_MATCHES + kTopkChunk, live))) return rc;
	return c->d_keys[1].reserve((nblk * VK_MAX_MATCHES) / 2 + 2 * kTopkChunk, live);
}

int vk_wait_peer_turn(vk_corpus *c, hipStream_t st) {
	std::lock_guard<std::mutex> g(vk_ring_mutex());
	vk_corpus *p = c->peer;
	if (p && p->ev2_recorded.load()) VK_HIP(hipStreamWaitEvent(st, p->ev[2], 0));
	return VK_OK;
}

extern "C" {

int vk_abi_version(void) { return VK_ABI_VERSION; }

const char *vk_last_error(void) { return vk_error_slot().c_str(); }

int vk_device_count(int *count) {
	if (!count) return fail(VK_ERR_INVALID, "count is null");
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess) { *count = 0; return fail(VK_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
	*count = n;
	return VK_OK;
}

int vk_init(int device) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(VK_ERR_NO_DEVICE, "no HIP device available");
	if (device < 0 || device >= n) return fail(VK_ERR_INVALID, "device index out of range");
	VK_HIP(hipSetDevice(device));
	hipDeviceProp_t prop;
	VK_HIP(hipGetDeviceProperties(&prop, device));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return fail(VK_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
	return VK_OK;
}

int vk_corpus_create(const vk_corpus_desc *desc, vk_corpus_t **out) {
	if (!desc || !out) return fail(VK_ERR_INVALID, "null argument");
	if (desc->layout != VK_LAYOUT_CONTEXTUAL && desc->layout != VK_LAYOUT_STATIC) return fail(VK_ERR_INVALID, "bad layout");
	if (desc->d < 1 || desc->d > 8192) return fail(VK_ERR_INVALID, "embedding dimension out of range");
	if (desc->n_tokens < 0 || desc->n_tokens >= (1ll << 31) - 64) return fail(VK_ERR_INVALID, "n_tokens must be < 2^31 per shard");
	if (desc->n_sentences < 0 || desc->n_sentences >= (1ll << 31) - 8) return fail(VK_ERR_INVALID, "n_sentences out of range");
	if (desc->layout == VK_LAYOUT_STATIC && desc->vocab_size < 1) return fail(VK_ERR_INVALID, "static layout needs vocab_size >= 1");
	if (desc->precision != VK_PREC_BF16 && desc->precision != VK_PREC_F32) return fail(VK_ERR_INVALID, "bad precision");

	int dev = 0;
	VK_HIP(hipGetDevice(&dev));
	vk_corpus *c = new vk_corpus();
	c->desc = *desc;
	c->device = dev;
	c->shared = std::make_shared<vk_devblock>();
	c->shared->device = dev;
	c->resident = std::make_shared<vk_resident_boost>();
	c->d_pad = (desc->d + 15) / 16 * 16;
	c->prec = desc->precision == VK_PREC_F32 ? 1 : 0;
	if (c->prec) {
		c->nk32 = c->d_pad / 16;          // fp32 tiles: blocks of 16 features, 1 KiB each
		c->tail = 0;
		c->tile_bytes = c->d_pad * 64;
	} else {
		c->nk32 = (c->d_pad + 31) / 32;   // K=32 steps; the last one is half filled when tail
		c->tail = (c->d_pad % 32) ? 1 : 0;
		c->tile_bytes = c->d_pad * 32;
	}
	c->rows_total = desc->layout == VK_LAYOUT_STATIC ? desc->vocab_size : desc->n_tokens;
	c->n_tiles = (c->rows_total + 15) / 16 + 1;   // + one zero tile: waves may read one tile past the end

	int rc = VK_OK;
	do {
		if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(VK_ERR_HIP, "hipStreamCreate failed"); break; }
		for (auto &e : c->ev) if (hipEventCreate(&e) != hipSuccess) { rc = fail(VK_ERR_HIP, "hipEventCreate failed"); break; }
		if (rc) break;
		if ((rc = alloc_shared(c, &c->d_tiles, (size_t)c->n_tiles * c->tile_bytes))) break;
		if (hipMemsetAsync(c->d_tiles, 0, (size_t)c->n_tiles * c->tile_bytes, c->stream) != hipSuccess) { rc = fail(VK_ERR_HIP, "memset failed"); break; }
		if (desc->keep_magnitudes && (rc = alloc_shared(c, &c->d_mag, (size_t)c->rows_total + 16))) break;
		if (desc->layout == VK_LAYOUT_STATIC) {
			if ((rc = alloc_shared(c, &c->d_tok_id, (size_t)desc->n_tokens + 64))) break;
		}
		rc = reserve_query_workspaces(c);
	} while (0);
	if (rc) { vk_corpus_free(c); return rc; }
	*out = c;
	return VK_OK;
}

// A second handle on the same resident corpus: shares the read-only arrays (tiles, magnitudes, token ids, POS codes,
// slice table) and owns a stream, events and workspaces.  Two handles serve two queries at a time from two host
// threads: the selection, traceback and host part of one query overlap the scoring kernel of the next.
int vk_corpus_view(vk_corpus_t *src, vk_corpus_t **out) {
	if (!src || !out) return fail(VK_ERR_INVALID, "null argument");
	if (!src->finalized) return fail(VK_ERR_STATE, "corpus not finalized");
	if (src->is_view) return fail(VK_ERR_INVALID, "views are taken from the owning handle");
	VK_HIP(hipSetDevice(src->device));
	vk_corpus *c = new vk_corpus();
	static_cast<vk_corpus_shape &>(*c) = *src;   // (the owning blocks among it: the arrays live as long as any handle names them)
	c->finalized = true;
	c->is_view = true;
	int rc = VK_OK;
	do {
		if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(VK_ERR_HIP, "hipStreamCreate failed"); break; }
		for (auto &e : c->ev) if (hipEventCreate(&e) != hipSuccess) { rc = fail(VK_ERR_HIP, "hipEventCreate failed"); break; }
		if (rc) break;
		if ((rc = reserve_query_workspaces(c))) break;
		rc = reserve_table_workspaces(c, c->n_entries);
	} while (0);
	if (rc) { vk_corpus_free(c); return rc; }
	{   // into the ring of the handles on this corpus, once the handle is complete
		std::lock_guard<std::mutex> g(vk_ring_mutex());
		c->peer = src->peer ? src->peer : src;
		src->peer = c;
	}
	*out = c;
	return VK_OK;
}

// Frees this handle's own stream, events and workspaces.  The arrays it shares with other handles (a corpus and its views, the
// vocabulary of a filtered static corpus) belong to refcounted blocks and go with the last handle: any order of frees is fine, and
// a peer that is inside vk_query on another thread keeps everything it reads.  (Calls on ONE handle are the caller's to serialise.)
int vk_corpus_free(vk_corpus_t *c) {
	if (!c) return VK_OK;
	(void)hipSetDevice(c->device);
	{   // out of the ring first: from here on no peer reaches this handle's events
		std::lock_guard<std::mutex> g(vk_ring_mutex());
		if (c->peer) {
			vk_corpus *p = c->peer;
			while (p->peer != c) p = p->peer;
			p->peer = c->peer == p ? nullptr : c->peer;
			c->peer = nullptr;
		}
	}
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
	if (c->stream) (void)hipStreamDestroy(c->stream);
	delete c;   // the workspaces go with it (vk_devbuf), after the stream has drained
	return VK_OK;
}

int vk_corpus_device_bytes(const vk_corpus_t *c, int64_t *bytes) {
	if (!c || !bytes) return fail(VK_ERR_INVALID, "null argument");
	*bytes = c->device_bytes;
	return VK_OK;
}

int vk_corpus_append_vectors(vk_corpus_t *c, const void *rows, int64_t n_rows, int32_t dtype, int32_t mem, int32_t normalize) {
	if (!c || (!rows && n_rows > 0)) return fail(VK_ERR_INVALID, "null argument");
	if (c->finalized) return fail(VK_ERR_STATE, "corpus already finalized");
	if (dtype != VK_F32 && dtype != VK_BF16) return fail(VK_ERR_INVALID, "bad dtype");
	if (n_rows < 0 || c->rows_appended + n_rows > c->rows_total) return fail(VK_ERR_INVALID, "more rows appended than declared");
	VK_HIP(hipSetDevice(c->device));
	const size_t esz = dtype == VK_F32 ? 4 : 2;
	const size_t row_bytes = esz * (size_t)c->desc.d;
	if (mem == VK_MEM_DEVICE) {
		VK_HIP(vk_launch_pack(rows, dtype == VK_BF16, n_rows, c->desc.d, c->d_pad, c->rows_appended, c->d_tiles, c->d_mag,
			normalize, c->prec, c->stream));
		if (c->raw_rows)   // a source that is not the cosine: the rows once more, unmodified, as fp32 tiles
			VK_HIP(vk_launch_pack(rows, dtype == VK_BF16, n_rows, c->desc.d, c->raw_tile_bytes / 64, c->rows_appended, *c->raw_rows, nullptr, 0, 1, c->stream));
		VK_HIP(hipStreamSynchronize(c->stream));
		c->rows_appended += n_rows;
		return VK_OK;
	}
	if (mem != VK_MEM_HOST) return fail(VK_ERR_INVALID, "bad memory kind");
	if (int rc = c->d_stage.reserve((size_t)kStageBytes, &c->device_bytes)) return rc;
	const int64_t rows_per_chunk = std::max<int64_t>(1, kStageBytes / (int64_t)row_bytes);
	for (int64_t r = 0; r < n_rows; r += rows_per_chunk) {
		const int64_t nr = std::min(rows_per_chunk, n_rows - r);
		VK_HIP(hipMemcpyAsync(c->d_stage, (const uint8_t *)rows + (size_t)r * row_bytes, (size_t)nr * row_bytes, hipMemcpyHostToDevice, c->stream));
		VK_HIP(vk_launch_pack(c->d_stage, dtype == VK_BF16, nr, c->desc.d, c->d_pad, c->rows_appended + r, c->d_tiles, c->d_mag,
			normalize, c->prec, c->stream));
		if (c->raw_rows)
			VK_HIP(vk_launch_pack(c->d_stage, dtype == VK_BF16, nr, c->desc.d, c->raw_tile_bytes / 64, c->rows_appended + r, *c->raw_rows, nullptr, 0, 1, c->stream));
		VK_HIP(hipStreamSynchronize(c->stream));
	}
	c->rows_appended += n_rows;
	return VK_OK;
}

// Span vectors pooled from token rows on the device (vk_pool_host.h, vk_pool.hip), appended as vk_corpus_append_vectors
// appends rows in device memory.  Everything is validated before anything is enqueued; the rows, ids, spans and aggregates live in
// buffers of this call, which die after the stream has drained -- on every path (vk_guard.h).
static int append_pooled_body(vk_corpus *c, const void *rows, int64_t n_rows, int32_t dtype, int32_t mem, const int32_t *ids, int64_t n_ids,
	const int64_t *start, const int64_t *end, int64_t n_spans, int32_t agg, int32_t normalize, float *pooled_out,
	vk_devbuf<uint8_t> &d_rows, vk_devbuf<int32_t> &d_ids, vk_devbuf<int64_t> &d_spans, vk_devbuf<float> &d_pooled) {
	if (n_spans == 0) return VK_OK;
	const int d = c->desc.d;
	const size_t row_bytes = (dtype == VK_F32 ? 4 : 2) * (size_t)d;
	VK_HIP(hipSetDevice(c->device));
	const void *dev_rows = rows;
	if (mem == VK_MEM_HOST) {
		if (int rc = d_rows.reserve((size_t)n_rows * row_bytes, nullptr)) return rc;
		if (n_rows > 0) VK_HIP(hipMemcpyAsync(d_rows, rows, (size_t)n_rows * row_bytes, hipMemcpyHostToDevice, c->stream));
		dev_rows = d_rows;
	}
	if (ids) {
		if (int rc = d_ids.reserve((size_t)n_ids, nullptr)) return rc;
		if (n_ids > 0) VK_HIP(hipMemcpyAsync(d_ids, ids, (size_t)n_ids * 4, hipMemcpyHostToDevice, c->stream));
	}
	if (int rc = d_spans.reserve(2 * (size_t)n_spans, nullptr)) return rc;
	VK_HIP(hipMemcpyAsync(d_spans, start, (size_t)n_spans * 8, hipMemcpyHostToDevice, c->stream));
	VK_HIP(hipMemcpyAsync(d_spans + n_spans, end, (size_t)n_spans * 8, hipMemcpyHostToDevice, c->stream));
	if (int rc = d_pooled.reserve((size_t)n_spans * (size_t)d, nullptr)) return rc;
	VK_HIP(vk_launch_pool_spans(dev_rows, dtype == VK_BF16, ids ? (const int32_t *)d_ids : nullptr, d_spans, d_spans + n_spans, n_spans, d, agg,
		d_pooled, c->stream));
	VK_HIP(vk_launch_pack(d_pooled, 0, n_spans, d, c->d_pad, c->rows_appended, c->d_tiles, c->d_mag, normalize, c->prec, c->stream));
	if (c->raw_rows)   // a span similarity beside the cosine: the aggregates once more, unmodified (a row of NaN stays NaN), as fp32 tiles
		VK_HIP(vk_launch_pack(d_pooled, 0, n_spans, d, c->raw_tile_bytes / 64, c->rows_appended, *c->raw_rows, nullptr, 0, 1, c->stream));
	if (pooled_out) VK_HIP(hipMemcpyAsync(pooled_out, d_pooled, (size_t)n_spans * (size_t)d * 4, hipMemcpyDeviceToHost, c->stream));
	VK_HIP(hipStreamSynchronize(c->stream));
	c->rows_appended += n_spans;
	return VK_OK;
}

int vk_corpus_append_pooled(vk_corpus_t *c, const void *rows, int64_t n_rows, int32_t dtype, int32_t mem, const int32_t *ids, int64_t n_ids,
	const int64_t *start, const int64_t *end, int64_t n_spans, int32_t agg, int32_t normalize, float *pooled_out) {
	if (!c || (!rows && n_rows > 0) || ((!start || !end) && n_spans > 0)) return fail(VK_ERR_INVALID, "null argument");
	if (c->finalized) return fail(VK_ERR_STATE, "corpus already finalized");
	if (c->is_view) return fail(VK_ERR_STATE, "rows are appended to the owning handle, before taking views");
	if (c->desc.layout != VK_LAYOUT_CONTEXTUAL)
		return fail(VK_ERR_UNSUPPORTED, "pooled span vectors are appended to a VK_LAYOUT_CONTEXTUAL handle (one row per span): this corpus is VK_LAYOUT_STATIC");
	// (a span similarity -- vk_corpus_set_span_sim -- is no such source: its copy of the unmodified rows is packed below)
	if (c->sim_src.kind != VK_SIMSRC_COSINE || c->mixed() || (c->raw_rows && !c->span_sim.sourced()))
		return fail(VK_ERR_UNSUPPORTED, "pooled span vectors under a similarity source or combinator: the span corpus computes the cosine");
	if (dtype != VK_F32 && dtype != VK_BF16) return fail(VK_ERR_INVALID, "bad dtype");
	if (mem != VK_MEM_HOST && mem != VK_MEM_DEVICE) return fail(VK_ERR_INVALID, "bad memory kind");
	if (!vk_host::pool_agg_ok(agg)) return fail(VK_ERR_INVALID, "unknown aggregate " + std::to_string(agg) + " (VK_POOL_MEAN, VK_POOL_MIN, VK_POOL_MAX)");
	if (n_rows < 0 || n_spans < 0 || (ids && n_ids < 0)) return fail(VK_ERR_INVALID, "a negative count");
	if (c->rows_appended + n_spans > c->rows_total) return fail(VK_ERR_INVALID, "more rows appended than declared");
	const char *why = "";
	if (const int bad = vk_host::pool_check_spans(n_rows, ids, n_ids, start, end, n_spans, &why))
		return fail(bad == vk_host::POOL_UNSUPPORTED ? VK_ERR_UNSUPPORTED : VK_ERR_INVALID, std::string("vk_corpus_append_pooled: ") + why);
	// (declared here: they are freed after the guard has drained the stream)
	vk_devbuf<uint8_t> d_rows;
	vk_devbuf<int32_t> d_ids;
	vk_devbuf<int64_t> d_spans;
	vk_devbuf<float> d_pooled;
	return vk_run_guarded(
		[&](vk_host_keep &) { return append_pooled_body(c, rows, n_rows, dtype, mem, ids, n_ids, start, end, n_spans, agg, normalize, pooled_out, d_rows, d_ids, d_spans, d_pooled); },
		[&]() { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); },
		[](const char *what) { return fail(VK_ERR_INVALID, std::string("vk_corpus_append_pooled: ") + what); });
}

int vk_corpus_set_token_ids(vk_corpus_t *c, const int32_t *ids, int64_t n, int32_t mem) {
	if (!c || !ids) return fail(VK_ERR_INVALID, "null argument");
	if (c->desc.layout != VK_LAYOUT_STATIC) return fail(VK_ERR_STATE, "token ids belong to the static layout");
	if (c->finalized) return fail(VK_ERR_STATE, "corpus already finalized");
	if (n != c->desc.n_tokens) return fail(VK_ERR_INVALID, "token id count differs from n_tokens");
	VK_HIP(hipSetDevice(c->device));
	if (mem == VK_MEM_HOST) {
		for (int64_t i = 0; i < n; i++)
			if (ids[i] < 0 || ids[i] >= c->desc.vocab_size) return fail(VK_ERR_INVALID, "token id outside the vocabulary");
	}
	VK_HIP(hipMemcpyAsync(c->d_tok_id, ids, (size_t)n * 4, mem == VK_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
	VK_HIP(hipStreamSynchronize(c->stream));
	c->h_tok = std::make_shared<std::vector<int32_t>>((size_t)n);
	if (mem == VK_MEM_DEVICE) VK_HIP(hipMemcpy(c->h_tok->data(), c->d_tok_id, (size_t)n * 4, hipMemcpyDeviceToHost));
	else memcpy(c->h_tok->data(), ids, (size_t)n * 4);
	c->have_ids = true;
	return VK_OK;
}

static int set_token_codes(vk_corpus_t *c, int8_t **slot, const int8_t *codes, int64_t n, int32_t mem, const char *what) {
	if (!c || !codes) return fail(VK_ERR_INVALID, "null argument");
	if (n != c->desc.n_tokens) return fail(VK_ERR_INVALID, std::string(what) + " count differs from n_tokens");
	if (c->is_view) return fail(VK_ERR_STATE, std::string("set ") + what + " codes on the owning handle, before taking views");
	VK_HIP(hipSetDevice(c->device));
	if (!*slot) {
		int rc = alloc_shared(c, slot, (size_t)n + 64);
		if (rc) return rc;
		VK_HIP(hipMemsetAsync(*slot, 0, (size_t)n + 64, c->stream));
	}
	VK_HIP(hipMemcpyAsync(*slot, codes, (size_t)n, mem == VK_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
	VK_HIP(hipStreamSynchronize(c->stream));
	return VK_OK;
}

int vk_corpus_set_token_pos(vk_corpus_t *c, const int8_t *pos, int64_t n, int32_t mem) {
	return set_token_codes(c, c ? &c->d_pos : nullptr, pos, n, mem, "POS");
}

int vk_corpus_set_token_tags(vk_corpus_t *c, const int8_t *tags, int64_t n, int32_t mem) {
	// The (token id, tag) vocabulary keys of tag-weighted transports are built as id * 256 + tag and must order like upstream's
	// signed pairs (TaggedTokenFactory, alignment/bow.h:150-176): tag codes have to be 0 .. 127.  Host arrays are checked here.
	if (c && tags && mem != VK_MEM_DEVICE && n == c->desc.n_tokens)
		for (int64_t i = 0; i < n; i++)
			if (tags[i] < 0) return fail(VK_ERR_INVALID, "tag codes must be 0 .. 127 (they key the vocabulary of tag-weighted transports as id * 256 + tag)");
	const int rc = set_token_codes(c, c ? &c->d_tag : nullptr, tags, n, mem, "tag");
	if (rc) return rc;
	c->h_tag = std::make_shared<std::vector<int8_t>>((size_t)n);
	if (mem == VK_MEM_DEVICE) VK_HIP(hipMemcpy(c->h_tag->data(), c->d_tag, (size_t)n, hipMemcpyDeviceToHost));
	else memcpy(c->h_tag->data(), tags, (size_t)n);
	return VK_OK;
}

static int set_slices_impl(vk_corpus_t *c, const int64_t *start, const int64_t *end, int64_t n_sentences, bool contiguous) {
	int max_len = 0, max_short = 0, max_long = 0;
	int64_t n_long = 0;
	for (int64_t s = 0; s < n_sentences; s++) {
		const int64_t len = end[s] - start[s];
		if (start[s] < 0 || end[s] > c->desc.n_tokens || len < 0) return fail(VK_ERR_INVALID, "slice outside the token stream");
		if (s > 0 && (start[s] < start[s - 1] || end[s] < end[s - 1])) return fail(VK_ERR_INVALID, "slice starts and ends must be non-decreasing");
		if (len > VK_MAX_DOC_LEN) {   // (65 .. VK_MAX_SENT_LEN: every algorithm; beyond: alignments, vk_validate_query)
			char buf[128];
			snprintf(buf, sizeof buf, "slice %lld has %lld tokens; the HIP path handles at most %d", (long long)s, (long long)len, VK_MAX_DOC_LEN);
			return fail(VK_ERR_UNSUPPORTED, buf);
		}
		max_len = std::max(max_len, (int)len);
		if (len > VK_FAST_SENT_LEN) n_long++;
		else max_short = std::max(max_short, (int)len);
		if (len > VK_FAST_SENT_LEN && len <= VK_MAX_SENT_LEN) max_long = std::max(max_long, (int)len);
	}
	VK_HIP(hipSetDevice(c->device));

	// ---- the slice table.  Without long slices it is the caller's table.  A long slice gets a group of 4 rows
	// of its own ([L, empty, empty, empty]); the group before it is closed with empty rows, so that no group of
	// the main launch spans the tokens of a long slice.  Rows stay in slice order (ties are broken by row).
	// apart_groups: every group that holds a slice of more than 64 tokens; long_groups: those of them the long pass takes (65 .. 512
	// tokens, LDS strips); the slices beyond (whole documents) are left to the one-wave-per-slice kernel (xlong_entries: their rows)
	std::vector<int32_t> st32, en32, long_groups, apart_groups;
	auto xlong_entries = std::make_shared<std::vector<int32_t>>();
	auto apart_entries = std::make_shared<std::vector<int32_t>>();   // the rows of every group apart (general gaps: all of them take the one-wave-per-slice pass)
	c->entry_sent.clear(); c->sent_entry.clear();
	if (n_long == 0) {
		st32.resize((size_t)n_sentences); en32.resize((size_t)n_sentences);
		for (int64_t s = 0; s < n_sentences; s++) { st32[(size_t)s] = (int32_t)start[s]; en32[(size_t)s] = (int32_t)end[s]; }
	} else {
		if (n_sentences + 3 * n_long + 3 >= (1ll << 31) - 16) return fail(VK_ERR_INVALID, "slice table too large");
		auto push = [&](int32_t a, int32_t b, int32_t sent) { st32.push_back(a); en32.push_back(b); c->entry_sent.push_back(sent); };
		for (int64_t s = 0; s < n_sentences; s++) {
			if (end[s] - start[s] > VK_FAST_SENT_LEN) {
				while (st32.size() % 4) push(en32.back(), en32.back(), -1);
				apart_groups.push_back((int32_t)(st32.size() / 4));
				for (int i = 0; i < 4; i++) apart_entries->push_back((int32_t)st32.size() + i);
				if (end[s] - start[s] > VK_MAX_SENT_LEN) {
					// (the four rows of its group: no other pass writes the scores of the three empty ones)
					for (int i = 0; i < 4; i++) xlong_entries->push_back((int32_t)st32.size() + i);
				} else long_groups.push_back((int32_t)(st32.size() / 4));
				push((int32_t)start[s], (int32_t)end[s], (int32_t)s);
				for (int i = 0; i < 3; i++) push((int32_t)end[s], (int32_t)end[s], -1);
			} else {
				push((int32_t)start[s], (int32_t)end[s], (int32_t)s);
			}
		}
	}
	const int64_t n_entries = (int64_t)st32.size();
	const int32_t tail = n_entries > 0 ? en32.back() : 0;
	for (int i = 0; i < 8; i++) { st32.push_back(tail); en32.push_back(tail); }   // padding: empty slices at the end

	// ---- device arrays sized by the table (re-created when the slices are set again)
	for (void *p : {(void *)c->d_sent_start, (void *)c->d_sent_end, (void *)c->d_long_groups}) c->shared->release(p);
	c->d_scores.reset(); c->d_raw.reset(); c->d_keys[0].reset(); c->d_keys[1].reset(); c->d_boost.reset();
	c->d_sent_start = c->d_sent_end = nullptr; c->d_long_groups = nullptr;
	int rc;
	if ((rc = alloc_shared(c, &c->d_sent_start, st32.size()))) return rc;
	if ((rc = alloc_shared(c, &c->d_sent_end, en32.size()))) return rc;
	if ((rc = reserve_table_workspaces(c, n_entries))) return rc;
	if (!long_groups.empty()) {
		if ((rc = alloc_shared(c, &c->d_long_groups, long_groups.size()))) return rc;
		VK_HIP(hipMemcpy(c->d_long_groups, long_groups.data(), long_groups.size() * 4, hipMemcpyHostToDevice));
	}
	VK_HIP(hipMemcpy(c->d_sent_start, st32.data(), st32.size() * 4, hipMemcpyHostToDevice));
	VK_HIP(hipMemcpy(c->d_sent_end, en32.data(), en32.size() * 4, hipMemcpyHostToDevice));
	c->h_start = std::make_shared<std::vector<int32_t>>(st32);
	c->h_end = std::make_shared<std::vector<int32_t>>(en32);
	c->n_entries = n_entries;
	c->d_wide_order.reset(); c->d_xlong_order.reset(); c->d_apart_order.reset();
	c->n_wide_order = c->n_xlong_order = c->n_apart_order = -1;   // the work list of the one-wave-per-slice pass follows the table
	c->lq.order.reset(); c->lq.n_order = -1;                      // ... and that of the long queries' block form
	c->n_long_groups = (int)long_groups.size();
	c->max_len = max_len;
	c->max_short_len = max_short;
	c->max_long_len = max_long;
	c->h_xlong = xlong_entries;
	c->h_apart = apart_entries;
	c->contiguous = contiguous;
	c->overlapping = false;
	for (int64_t s = 1; s < n_sentences && !c->overlapping; s++) c->overlapping = start[s] < end[s - 1] && end[s] > start[s];
	c->uniform_len = 0;
	if (n_sentences > 0 && contiguous) {
		const int64_t l0 = end[0] - start[0];
		bool uni = l0 > 0;
		for (int64_t s = 1; s < n_sentences && uni; s++) uni = (end[s] - start[s]) == l0;
		if (uni) c->uniform_len = (int)l0;
	}
	// per wave: groups of 4 consecutive rows; LDS strips are sized for the main launch and the long one apart
	int mt = 1, mtok = 1, lt = 1, ltok = 1;
	size_t li = 0;
	for (int64_t g = 0; g * 4 < n_entries; g++) {
		const int64_t a = st32[(size_t)(g * 4)], b = en32[(size_t)std::min<int64_t>(g * 4 + 3, n_entries - 1)];
		const int tiles = (int)(((b + 15) >> 4) - (a >> 4));
		if (li < apart_groups.size() && apart_groups[li] == g) {
			li++;
			if (b - a <= VK_MAX_SENT_LEN) {   // (a group apart holds one slice: its tokens are the slice's)
				lt = std::max(lt, tiles);
				ltok = std::max(ltok, (int)(b - a));
			}
		} else {
			mt = std::max(mt, tiles);
			mtok = std::max(mtok, (int)(b - a));
		}
	}
	int pt = 1, spt = 1;
	li = 0;
	for (int64_t g = 0; g * 2 < n_entries; g++) {
		const int64_t a = st32[(size_t)(g * 2)], b = en32[(size_t)std::min<int64_t>(g * 2 + 1, n_entries - 1)];
		const int tiles = (int)(((b + 15) >> 4) - (a >> 4));
		pt = std::max(pt, tiles);
		while (li < apart_groups.size() && apart_groups[li] < g / 2) li++;
		if (!(li < apart_groups.size() && apart_groups[li] == g / 2)) spt = std::max(spt, tiles);
	}
	c->max_pair_tiles = pt;
	c->max_short_pair_tiles = spt;
	c->max_group_tiles = mt;
	c->max_group_tokens = mtok;
	c->long_group_tiles = lt;
	c->long_group_tokens = ltok;
	c->have_sent = true;
	return VK_OK;
}

int vk_corpus_set_sentences(vk_corpus_t *c, const int64_t *sent_off, int64_t n_sentences) {
	if (!c || !sent_off) return fail(VK_ERR_INVALID, "null argument");
	if (c->finalized) return fail(VK_ERR_STATE, "corpus already finalized");
	if (n_sentences != c->desc.n_sentences) return fail(VK_ERR_INVALID, "sentence count differs from n_sentences");
	if (sent_off[0] != 0) return fail(VK_ERR_INVALID, "sentence spans must start at token 0 (document.h:151-168)");
	if (sent_off[n_sentences] != c->desc.n_tokens) return fail(VK_ERR_INVALID, "sentence spans must cover exactly n_tokens");
	for (int64_t s = 0; s < n_sentences; s++)
		if (sent_off[s + 1] < sent_off[s]) return fail(VK_ERR_INVALID, "sentence offsets must be non-decreasing");
	return set_slices_impl(c, sent_off, sent_off + 1, n_sentences, true);
}

int vk_corpus_set_slices(vk_corpus_t *c, const int64_t *start, const int64_t *end, int64_t n_sentences) {
	if (!c || !start || !end) return fail(VK_ERR_INVALID, "null argument");
	if (c->finalized) return fail(VK_ERR_STATE, "corpus already finalized");
	if (n_sentences != c->desc.n_sentences) return fail(VK_ERR_INVALID, "slice count differs from n_sentences");
	return set_slices_impl(c, start, end, n_sentences, false);
}

// The shadow of the token rows in the format vk_host::shadow_format_of gives this corpus -- none for most -- with every slice
// within VK_FAST_SENT_LEN tokens.  Never an error: without the memory (or with a row that is not finite) the corpus has no shadow and
// its queries take the exact pass.
static void build_shadow(vk_corpus *c) {
	const int mode = bound_pass_mode();
	if (mode < 0 || (mode == 0 && c->desc.n_sentences < kBoundPassMinSentences)) return;
	if (c->max_len > VK_FAST_SENT_LEN || c->n_entries < 1) return;
	const vk_host::shadow_format f = vk_host::shadow_format_of(c->desc.d, c->nk32, c->tail, c->prec, c->desc.layout, bound_bits_wanted(mode));
	if (f.bits == 0) return;
	const size_t bytes = (size_t)c->n_tiles * f.tile_bytes();
	uint8_t *sh = nullptr;
	if (c->d_counter.reserve(4, &c->device_bytes) || alloc_shared(c, &sh, bytes)) { (void)hipGetLastError(); return; }
	uint32_t stats[4] = {0, 0, 1, 0};
	const bool ran = vk_launch_shadow(c->d_tiles, c->n_tiles, c->rows_total, c->tile_bytes, &f, sh, c->d_counter, c->stream) == hipSuccess
		&& hipMemcpyAsync(stats, c->d_counter, 16, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
	if (!ran || stats[2] != 0) {
		(void)hipGetLastError();
		c->shared->release(sh);
		c->device_bytes -= (int64_t)bytes;
		return;
	}
	c->shadow = sh; c->shadow_format = f;
	memcpy(&c->shadow_n, &stats[0], 4);
	memcpy(&c->shadow_x, &stats[1], 4);
}

int vk_corpus_finalize(vk_corpus_t *c) {
	if (!c) return fail(VK_ERR_INVALID, "null argument");
	if (c->rows_appended != c->rows_total) return fail(VK_ERR_STATE, "not all vectors were appended");
	if (!c->have_sent) return fail(VK_ERR_STATE, "sentence spans were not set");
	if (c->desc.layout == VK_LAYOUT_STATIC && !c->have_ids) return fail(VK_ERR_STATE, "token ids were not set");
	for (int m = 1; c->mixed() && m < c->sim_mix.n; m++)
		if (c->operands[m - 1].rows_appended != c->rows_total)
			return fail(VK_ERR_STATE, "mixed handle: operand " + std::to_string(m) + " has " + std::to_string(c->operands[m - 1].rows_appended) + " of " + std::to_string(c->rows_total) + " vocabulary rows (vk_corpus_append_operand_vectors)");
	VK_HIP(hipSetDevice(c->device));
	c->d_stage.reset();
	VK_HIP(hipStreamSynchronize(c->stream));
	build_shadow(c);
	c->finalized = true;
	return VK_OK;
}

// The operator chain of a ModifiedVectorSim on the cosine (vk_sim_ops_host.h): host state of the handle, read when a query fills its
// kernels' parameters.  Contextual corpora refuse a chain HERE, as they always have: vk_corpus_set_contextual_sim_ops is theirs.
int vk_corpus_set_sim_ops(vk_corpus_t *c, const int32_t *kinds, const float *args, int32_t n_ops) {
	if (!c || (n_ops > 0 && (!kinds || !args))) return fail(VK_ERR_INVALID, "null argument");
	int bad = -1;
	if (vk_host::sim_ops_check(kinds, args, n_ops, &bad) != VK_OK) {
		if (bad < 0) return fail(VK_ERR_INVALID, "n_ops must be 0 .. VK_MAX_SIM_OPS (8), got " + std::to_string(n_ops));
		return fail(VK_ERR_INVALID, "similarity operator " + std::to_string(bad) + ": unknown kind or an argument that is not finite");
	}
	if (n_ops > 0 && c->desc.layout != VK_LAYOUT_STATIC)
		return fail(VK_ERR_UNSUPPORTED, "similarity operators run over VK_LAYOUT_STATIC only: this corpus is VK_LAYOUT_CONTEXTUAL");
	vk_host::sim_ops ops{};
	ops.n = n_ops;
	for (int i = 0; i < n_ops; i++) { ops.kind[i] = kinds[i]; ops.arg[i] = args[i]; }
	c->sim_ops = ops;
	return VK_OK;
}

// The chain of a VK_LAYOUT_CONTEXTUAL handle: the same host state -- a handle has one layout, so one field serves both --
// read by the router (route_facts::chained), by the scoring launches (VkScoreParams / VkWideParams) and by every kernel that restates
// the winners' cells (sim_ops_field).  The cell is vk_host::contextual_cell.
int vk_corpus_set_contextual_sim_ops(vk_corpus_t *c, const int32_t *kinds, const float *args, int32_t n_ops) {
	if (!c || (n_ops > 0 && (!kinds || !args))) return fail(VK_ERR_INVALID, "null argument");
	int bad = -1;
	if (vk_host::sim_ops_check(kinds, args, n_ops, &bad) != VK_OK) {
		if (bad < 0) return fail(VK_ERR_INVALID, "vk_corpus_set_contextual_sim_ops: n_ops must be 0 .. VK_MAX_SIM_OPS (8), got " + std::to_string(n_ops));
		return fail(VK_ERR_INVALID, "vk_corpus_set_contextual_sim_ops: similarity operator " + std::to_string(bad) + ": unknown kind or an argument that is not finite");
	}
	if (c->desc.layout != VK_LAYOUT_CONTEXTUAL)
		return fail(VK_ERR_UNSUPPORTED, "vk_corpus_set_contextual_sim_ops: this corpus is VK_LAYOUT_STATIC -- its chain is set with vk_corpus_set_sim_ops");
	if (c->span_sim.active())
		return fail(VK_ERR_UNSUPPORTED, "vk_corpus_set_contextual_sim_ops: this handle is under a span similarity (vk_corpus_set_span_sim), which carries the span index's own chain");
	vk_host::sim_ops ops{};
	ops.n = n_ops;
	for (int i = 0; i < n_ops; i++) { ops.kind[i] = kinds[i]; ops.arg[i] = args[i]; }
	c->sim_ops = ops;
	return VK_OK;
}

// The source the chain runs on (vk_sim_src_host.h).  A source that is not the cosine reads the UNMODIFIED rows: the handle allocates a
// second, fp32 copy of them here (fp32 tile layout, zero tile included), which vk_corpus_append_vectors then fills beside the unit
// tiles -- hence before the first append.  Contextual corpora refuse: their similarities come out of the matrix pipe.
int vk_corpus_set_sim_source(vk_corpus_t *c, int32_t kind, float arg) {
	if (!c) return fail(VK_ERR_INVALID, "null argument");
	if (vk_host::sim_src_check(kind, arg) != VK_OK)
		return fail(VK_ERR_INVALID, kind == VK_SIMSRC_PNORM ? "VK_SIMSRC_PNORM: p must be finite and > 0" : "unknown similarity source " + std::to_string(kind));
	if (kind == VK_SIMSRC_COSINE) { c->sim_src = vk_host::sim_src{VK_SIMSRC_COSINE, 0.0f}; return VK_OK; }
	if (c->desc.layout != VK_LAYOUT_STATIC)
		return fail(VK_ERR_UNSUPPORTED, "similarity sources beside the cosine run over VK_LAYOUT_STATIC only: this corpus is VK_LAYOUT_CONTEXTUAL");
	if (c->desc.d > vk_host::kSimSrcMaxD)
		return fail(VK_ERR_UNSUPPORTED, "similarity sources beside the cosine: rows of at most " + std::to_string(vk_host::kSimSrcMaxD) + " features (the table kernel keeps a query tile in LDS)");
	if (!c->raw_rows) {
		if (c->rows_appended > 0 || c->finalized || c->is_view || c->shares_vectors)
			return fail(VK_ERR_STATE, "a similarity source beside the cosine is set before the first vk_corpus_append_vectors: it reads the unmodified rows, and they are gone");
		VK_HIP(hipSetDevice(c->device));
		const int raw_tile_bytes = (c->desc.d + 15) / 16 * 1024;
		const size_t bytes = (size_t)c->n_tiles * (size_t)raw_tile_bytes;
		auto rows = std::make_shared<vk_devbuf<uint8_t>>();
		if (int rc = rows->reserve(bytes, nullptr)) return rc;
		VK_HIP(hipMemsetAsync(*rows, 0, bytes, c->stream));   // (an error leaves the handle without the copy: `rows` frees it)
		VK_HIP(hipStreamSynchronize(c->stream));
		c->raw_rows = rows; c->raw_tile_bytes = raw_tile_bytes;
		c->device_bytes += (int64_t)bytes;
	}
	c->sim_src = vk_host::sim_src{kind, kind == VK_SIMSRC_PNORM ? arg : 0.0f};
	return VK_OK;
}

// The span similarity (vk_span_sim_host.h): a VK_LAYOUT_CONTEXTUAL handle of one-row slices under a VectorSim that is not
// the bare cosine.  Host state in fields of its own (vk_corpus_shape::span_sim); a source that is not the cosine reads the UNMODIFIED
// rows, of which the handle allocates the second, fp32 copy here as vk_corpus_set_sim_source does for a static handle -- hence before
// the first append.  Everything is validated before anything changes: a refused call leaves the handle as it was.
int vk_corpus_set_span_sim(vk_corpus_t *c, int32_t src_kind, float src_arg, const int32_t *op_kinds, const float *op_args, int32_t n_ops) {
	if (!c || (n_ops > 0 && (!op_kinds || !op_args))) return fail(VK_ERR_INVALID, "null argument");
	if (vk_host::sim_src_check(src_kind, src_arg) != VK_OK)
		return fail(VK_ERR_INVALID, src_kind == VK_SIMSRC_PNORM ? "vk_corpus_set_span_sim: VK_SIMSRC_PNORM: p must be finite and > 0" : "vk_corpus_set_span_sim: unknown similarity source " + std::to_string(src_kind));
	int bad = -1;
	if (vk_host::sim_ops_check(op_kinds, op_args, n_ops, &bad) != VK_OK) {
		if (bad < 0) return fail(VK_ERR_INVALID, "vk_corpus_set_span_sim: n_ops must be 0 .. VK_MAX_SIM_OPS (8), got " + std::to_string(n_ops));
		return fail(VK_ERR_INVALID, "vk_corpus_set_span_sim: similarity operator " + std::to_string(bad) + ": unknown kind or an argument that is not finite");
	}
	if (c->desc.layout != VK_LAYOUT_CONTEXTUAL)
		return fail(VK_ERR_UNSUPPORTED, "a span similarity is set on a VK_LAYOUT_CONTEXTUAL handle (one row per span): this corpus is VK_LAYOUT_STATIC (vk_corpus_set_sim_source, vk_corpus_set_sim_ops)");
	if (c->sim_ops.n > 0)
		return fail(VK_ERR_UNSUPPORTED, "vk_corpus_set_span_sim: this handle is under an operator chain of its token similarities (vk_corpus_set_contextual_sim_ops): clear it first");
	vk_host::span_sim sim{};
	sim.src = vk_host::sim_src{src_kind, src_kind == VK_SIMSRC_PNORM ? src_arg : 0.0f};
	sim.ops.n = n_ops;
	for (int i = 0; i < n_ops; i++) { sim.ops.kind[i] = op_kinds[i]; sim.ops.arg[i] = op_args[i]; }
	if (sim.sourced() && !c->raw_rows) {
		if (c->desc.d > vk_host::kSimSrcMaxD)
			return fail(VK_ERR_UNSUPPORTED, "span similarities beside the cosine: rows of at most " + std::to_string(vk_host::kSimSrcMaxD) + " features (the query is staged in 4 KiB of LDS)");
		if (c->rows_appended > 0 || c->finalized || c->is_view || c->shares_vectors)
			return fail(VK_ERR_STATE, "a span similarity beside the cosine is set before the first append: it reads the unmodified rows, and they are gone");
		VK_HIP(hipSetDevice(c->device));
		const int raw_tile_bytes = vk_host::span_sim_raw_tile_bytes(c->desc.d);
		const size_t bytes = (size_t)c->n_tiles * (size_t)raw_tile_bytes;
		auto rows = std::make_shared<vk_devbuf<uint8_t>>();
		if (int rc = rows->reserve(bytes, nullptr)) return rc;
		VK_HIP(hipMemsetAsync(*rows, 0, bytes, c->stream));   // (an error leaves the handle without the copy: `rows` frees it)
		VK_HIP(hipStreamSynchronize(c->stream));
		c->raw_rows = rows; c->raw_tile_bytes = raw_tile_bytes;
		c->device_bytes += (int64_t)bytes;   // counted by hand, as under vk_corpus_set_sim_source: the buffer may outlive this handle
	}
	c->span_sim = sim;
	return VK_OK;
}

// The combinator of a mixed handle (vk_sim_mix_host.h): host state, read when a query fills its tables.  Before the first
// append, as a source is: the operands' rows arrive beside the handle's own.
int vk_corpus_set_sim_mix(vk_corpus_t *c, int32_t kind, int32_t n_operands, const double *weights) {
	if (!c) return fail(VK_ERR_INVALID, "null argument");
	const char *why = "";
	if (vk_host::sim_mix_check(kind, n_operands, weights, &why) != VK_OK) return fail(VK_ERR_INVALID, std::string("vk_corpus_set_sim_mix: ") + why);
	if (c->desc.layout != VK_LAYOUT_STATIC)
		return fail(VK_ERR_UNSUPPORTED, "token similarity combinators run over VK_LAYOUT_STATIC only: this corpus is VK_LAYOUT_CONTEXTUAL");
	if (c->rows_appended > 0 || c->finalized || c->is_view || c->shares_vectors)
		return fail(VK_ERR_STATE, "a token similarity combinator is set before the first vk_corpus_append_vectors");
	for (const auto &op : c->operands)
		if (op.rows_appended > 0) return fail(VK_ERR_STATE, "a token similarity combinator is set before the first vk_corpus_append_operand_vectors");
	vk_host::sim_mix mix{};
	mix.kind = kind; mix.n = n_operands;
	for (int m = 0; m < n_operands; m++) mix.w[m] = kind == VK_SIMMIX_AVERAGE ? weights[m] : 0.0;
	c->sim_mix = mix;
	return VK_OK;
}

static int mix_operand_of(vk_corpus_t *c, int32_t i, const char *who) {
	if (!c) return fail(VK_ERR_INVALID, "null argument");
	if (!c->mixed()) return fail(VK_ERR_STATE, std::string(who) + ": the handle has no combinator (vk_corpus_set_sim_mix)");
	if (i < 1 || i >= c->sim_mix.n) return fail(VK_ERR_INVALID, std::string(who) + ": operand index must be 1 .. n_operands - 1 (operand 0 is the handle itself)");
	return VK_OK;
}

// An operand's width, source and chain; allocates its tiles as vk_corpus_create allocates the handle's, and -- under a source that is
// not the cosine -- the fp32 copy of the unmodified rows as vk_corpus_set_sim_source does
int vk_corpus_set_sim_operand(vk_corpus_t *c, int32_t i, int32_t d_i, int32_t src_kind, float src_arg, const int32_t *kinds, const float *args, int32_t n_ops) {
	if (int rc = mix_operand_of(c, i, "vk_corpus_set_sim_operand")) return rc;
	if (n_ops > 0 && (!kinds || !args)) return fail(VK_ERR_INVALID, "null argument");
	if (d_i < 1 || d_i > 8192) return fail(VK_ERR_INVALID, "embedding dimension out of range");
	if (vk_host::sim_src_check(src_kind, src_arg) != VK_OK)
		return fail(VK_ERR_INVALID, src_kind == VK_SIMSRC_PNORM ? "VK_SIMSRC_PNORM: p must be finite and > 0" : "unknown similarity source " + std::to_string(src_kind));
	int bad = -1;
	if (vk_host::sim_ops_check(kinds, args, n_ops, &bad) != VK_OK) {
		if (bad < 0) return fail(VK_ERR_INVALID, "n_ops must be 0 .. VK_MAX_SIM_OPS (8), got " + std::to_string(n_ops));
		return fail(VK_ERR_INVALID, "similarity operator " + std::to_string(bad) + ": unknown kind or an argument that is not finite");
	}
	if (src_kind != VK_SIMSRC_COSINE && d_i > vk_host::kSimSrcMaxD)
		return fail(VK_ERR_UNSUPPORTED, "similarity sources beside the cosine: rows of at most " + std::to_string(vk_host::kSimSrcMaxD) + " features (the table kernel keeps a query tile in LDS)");
	vk_corpus::sim_operand &op = c->operands[i - 1];
	vk_host::sim_ops chain{};
	chain.n = n_ops;
	for (int k = 0; k < n_ops; k++) { chain.kind[k] = kinds[k]; chain.arg[k] = args[k]; }
	// an operand that has its buffers: source and chain are host state, as vk_corpus_set_sim_source / vk_corpus_set_sim_ops are on a
	// handle that keeps the rows they read -- at any time, on this handle alone
	if (op.tiles && op.d == d_i && (src_kind == VK_SIMSRC_COSINE || op.raw_rows)) {
		op.src = vk_host::sim_src{src_kind, src_kind == VK_SIMSRC_PNORM ? src_arg : 0.0f};
		op.ops = chain;
		return VK_OK;
	}
	if (op.rows_appended > 0 || c->finalized || c->is_view || c->shares_vectors)
		return fail(VK_ERR_STATE, "an operand's width, and a source beside the cosine, are set before its first vk_corpus_append_operand_vectors: the unmodified rows are gone");
	VK_HIP(hipSetDevice(c->device));
	vk_corpus::sim_operand fresh;
	fresh.d = d_i; fresh.d_pad = (d_i + 15) / 16 * 16;
	if (c->prec) { fresh.nk32 = fresh.d_pad / 16; fresh.tail = 0; fresh.tile_bytes = fresh.d_pad * 64; }
	else { fresh.nk32 = (fresh.d_pad + 31) / 32; fresh.tail = (fresh.d_pad % 32) ? 1 : 0; fresh.tile_bytes = fresh.d_pad * 32; }
	fresh.src = vk_host::sim_src{src_kind, src_kind == VK_SIMSRC_PNORM ? src_arg : 0.0f};
	fresh.ops = chain;
	int64_t bytes_before = 0;
	if (op.tiles) bytes_before += (int64_t)op.tiles->capacity();
	if (op.raw_rows) bytes_before += (int64_t)op.raw_rows->capacity();
	const size_t tile_bytes_all = (size_t)c->n_tiles * (size_t)fresh.tile_bytes;
	fresh.tiles = std::make_shared<vk_devbuf<uint8_t>>();
	if (int rc = fresh.tiles->reserve(tile_bytes_all, nullptr)) return rc;
	VK_HIP(hipMemsetAsync(*fresh.tiles, 0, tile_bytes_all, c->stream));
	size_t raw_all = 0;
	if (src_kind != VK_SIMSRC_COSINE) {
		fresh.raw_tile_bytes = (d_i + 15) / 16 * 1024;
		raw_all = (size_t)c->n_tiles * (size_t)fresh.raw_tile_bytes;
		fresh.raw_rows = std::make_shared<vk_devbuf<uint8_t>>();
		if (int rc = fresh.raw_rows->reserve(raw_all, nullptr)) return rc;
		VK_HIP(hipMemsetAsync(*fresh.raw_rows, 0, raw_all, c->stream));
	}
	VK_HIP(hipStreamSynchronize(c->stream));   // (an error above leaves the operand as it was: `fresh` frees what it allocated)
	op = fresh;
	c->device_bytes += (int64_t)(tile_bytes_all + raw_all) - bytes_before;   // counted by hand, as raw_rows: the buffers may outlive this handle
	return VK_OK;
}

int vk_corpus_append_operand_vectors(vk_corpus_t *c, int32_t i, const void *rows, int64_t n_rows, int32_t dtype, int32_t normalize) {
	if (int rc = mix_operand_of(c, i, "vk_corpus_append_operand_vectors")) return rc;
	if (!rows && n_rows > 0) return fail(VK_ERR_INVALID, "null argument");
	if (c->finalized) return fail(VK_ERR_STATE, "corpus already finalized");
	if (dtype != VK_F32 && dtype != VK_BF16) return fail(VK_ERR_INVALID, "bad dtype");
	vk_corpus::sim_operand &op = c->operands[i - 1];
	if (!op.tiles) return fail(VK_ERR_STATE, "vk_corpus_append_operand_vectors before vk_corpus_set_sim_operand");
	if (n_rows < 0 || op.rows_appended + n_rows > c->rows_total) return fail(VK_ERR_INVALID, "more rows appended than declared");
	VK_HIP(hipSetDevice(c->device));
	const size_t row_bytes = (dtype == VK_F32 ? 4 : 2) * (size_t)op.d;
	if (int rc = c->d_stage.reserve((size_t)kStageBytes, &c->device_bytes)) return rc;
	const int64_t rows_per_chunk = std::max<int64_t>(1, kStageBytes / (int64_t)row_bytes);
	for (int64_t r = 0; r < n_rows; r += rows_per_chunk) {
		const int64_t nr = std::min(rows_per_chunk, n_rows - r);
		VK_HIP(hipMemcpyAsync(c->d_stage, (const uint8_t *)rows + (size_t)r * row_bytes, (size_t)nr * row_bytes, hipMemcpyHostToDevice, c->stream));
		VK_HIP(vk_launch_pack(c->d_stage, dtype == VK_BF16, nr, op.d, op.d_pad, op.rows_appended + r, *op.tiles, nullptr, normalize, c->prec, c->stream));
		if (op.raw_rows)
			VK_HIP(vk_launch_pack(c->d_stage, dtype == VK_BF16, nr, op.d, op.raw_tile_bytes / 64, op.rows_appended + r, *op.raw_rows, nullptr, 0, 1, c->stream));
		VK_HIP(hipStreamSynchronize(c->stream));
	}
	op.rows_appended += n_rows;
	return VK_OK;
}

int vk_corpus_set_query_operand(vk_corpus_t *c, int32_t i, const void *q_vectors, int32_t len_t, int32_t q_dtype, int32_t q_normalize) {
	if (int rc = mix_operand_of(c, i, "vk_corpus_set_query_operand")) return rc;
	if (!q_vectors) return fail(VK_ERR_INVALID, "q_vectors is null");
	if (q_dtype != VK_F32 && q_dtype != VK_BF16) return fail(VK_ERR_INVALID, "bad q_dtype");
	if (len_t < 1 || len_t > VK_MAX_LONG_QUERY_LEN) return fail(VK_ERR_INVALID, "len_t must be 1 .. VK_MAX_LONG_QUERY_LEN (512)");
	const vk_corpus::sim_operand &op = c->operands[i - 1];
	if (op.d < 1) return fail(VK_ERR_STATE, "vk_corpus_set_query_operand before vk_corpus_set_sim_operand");
	vk_corpus::mix_operand_bufs::rows rows;
	rows.len_t = len_t; rows.dtype = q_dtype; rows.normalize = q_normalize;
	const size_t bytes = (size_t)len_t * (size_t)op.d * (q_dtype == VK_F32 ? 4 : 2);
	rows.bytes.assign((const uint8_t *)q_vectors, (const uint8_t *)q_vectors + bytes);
	c->mixop[i - 1].pending.push_back(std::move(rows));
	return VK_OK;
}

// ---- the booster of a Saliency (vk_saliency_host.h, vk_saliency.hip).  Every entry point validates all of its arguments
// before it touches the handle, keeps what it uploads for the call in buffers of the call, and returns after the stream has drained.

// what every signal call asks of the handle and of the slot
static int signal_call_ok(const vk_corpus *c, int32_t slot, const char *who) {
	if (!c) return fail(VK_ERR_INVALID, "null argument");
	if (!c->finalized) return fail(VK_ERR_STATE, std::string(who) + ": corpus not finalized");
	if (c->span_sim.active()) return fail(VK_ERR_UNSUPPORTED, std::string(who) + ": a handle under a span similarity (vk_corpus_set_span_sim) has no boosters");
	if (slot < 0 || slot >= VK_MAX_SIGNALS) return fail(VK_ERR_INVALID, std::string(who) + ": slot must be 0 .. VK_MAX_SIGNALS - 1");
	return VK_OK;
}
// a buffer of d_signal that no slot names (there is one more buffer than slots)
static int free_signal_buffer(const vk_corpus *c) {
	for (int b = 0; b <= VK_MAX_SIGNALS; b++)
		if (std::find(std::begin(c->signal_buf), std::end(c->signal_buf), b) == std::end(c->signal_buf)) return b;
	return -1;
}
// the buffer a slot's new signal is written to: its own again, or a free one
static int signal_buffer_for(vk_corpus *c, int32_t slot, int *buf) {
	*buf = c->signal_buf[slot] >= 0 ? c->signal_buf[slot] : free_signal_buffer(c);
	return c->d_signal[*buf].reserve((size_t)c->desc.n_sentences, &c->device_bytes);
}
// runs `body` on the handle's device and leaves nothing in flight behind it, whatever it returns
static int signal_run(vk_corpus *c, const std::function<int()> &body) {
	VK_HIP(hipSetDevice(c->device));
	const int rc = body();
	const hipError_t drained = hipStreamSynchronize(c->stream);
	if (!rc && drained != hipSuccess) return fail(VK_ERR_HIP, std::string("a saliency kernel failed: ") + hipGetErrorString(drained));
	return rc;
}

int vk_signal_keywords(vk_corpus_t *c, int32_t slot, const int32_t *keyword_ids, int32_t n_keywords, int32_t max_count, const int32_t *token_ids,
	int32_t vocab_size) {
	if (int rc = signal_call_ok(c, slot, "vk_signal_keywords")) return rc;
	const bool is_static = c->desc.layout == VK_LAYOUT_STATIC;
	if (!is_static && !token_ids) return fail(VK_ERR_INVALID, "vk_signal_keywords: a VK_LAYOUT_CONTEXTUAL handle keeps no token ids: pass them for the call");
	const int64_t V = is_static ? c->desc.vocab_size : vocab_size;
	if (V < 1) return fail(VK_ERR_INVALID, "vk_signal_keywords: vocab_size must be >= 1");
	if (max_count < 1) return fail(VK_ERR_INVALID, "vk_signal_keywords: max_count must be >= 1");
	if (n_keywords < 0 || (n_keywords > 0 && !keyword_ids)) return fail(VK_ERR_INVALID, "vk_signal_keywords: bad keyword ids");
	std::vector<uint32_t> bitmap((size_t)vk_host::sal_bitmap_words(V), 0u);
	for (int32_t k = 0; k < n_keywords; k++) {
		if (keyword_ids[k] < 0 || keyword_ids[k] >= V) return fail(VK_ERR_INVALID, "vk_signal_keywords: a keyword id outside the vocabulary");
		vk_host::sal_bitmap_set(bitmap.data(), keyword_ids[k]);
	}
	const int64_t ns = c->desc.n_sentences, nt = c->desc.n_tokens;
	if (!c->entry_sent.empty()) (void)row_of_sentence(c, 0);   // builds sent_entry
	vk_devbuf<uint32_t> d_bitmap;
	vk_devbuf<int32_t> d_ids, d_rows;
	return signal_run(c, [&]() -> int {
		hipStream_t st = c->stream;
		int rc, buf = -1;
		if ((rc = d_bitmap.reserve(bitmap.size(), nullptr))) return rc;
		VK_HIP(hipMemcpyAsync(d_bitmap, bitmap.data(), bitmap.size() * 4, hipMemcpyHostToDevice, st));
		const int32_t *ids = c->d_tok_id;
		if (!is_static) {
			if ((rc = d_ids.reserve((size_t)nt + 64, nullptr))) return rc;
			if (nt > 0) VK_HIP(hipMemcpyAsync(d_ids, token_ids, (size_t)nt * 4, hipMemcpyHostToDevice, st));
			ids = d_ids;
		}
		const int32_t *rows = nullptr;
		if (!c->entry_sent.empty()) {
			if ((rc = d_rows.reserve((size_t)ns, nullptr))) return rc;
			VK_HIP(hipMemcpyAsync(d_rows, c->sent_entry.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st));
			rows = d_rows;
		}
		if ((rc = signal_buffer_for(c, slot, &buf))) return rc;
		VK_HIP(vk_launch_keyword_signal(ids, c->d_sent_start, c->d_sent_end, rows, ns, d_bitmap, V, max_count, c->d_signal[buf], st));
		VK_HIP(hipStreamSynchronize(st));
		c->signal_buf[slot] = buf;
		return VK_OK;
	});
}

int vk_signal_set(vk_corpus_t *c, int32_t slot, const float *values) {
	if (int rc = signal_call_ok(c, slot, "vk_signal_set")) return rc;
	if (!values && c->desc.n_sentences > 0) return fail(VK_ERR_INVALID, "vk_signal_set: values is null");
	return signal_run(c, [&]() -> int {
		int buf = -1;
		if (int rc = signal_buffer_for(c, slot, &buf)) return rc;
		if (c->desc.n_sentences > 0) VK_HIP(hipMemcpyAsync(c->d_signal[buf], values, (size_t)c->desc.n_sentences * 4, hipMemcpyHostToDevice, c->stream));
		VK_HIP(hipStreamSynchronize(c->stream));
		c->signal_buf[slot] = buf;
		return VK_OK;
	});
}

int vk_signal_filter(vk_corpus_t *c, int32_t slot, int32_t kind, int32_t width, const double *pulse, const int64_t *doc_off, int64_t n_docs) {
	if (int rc = signal_call_ok(c, slot, "vk_signal_filter")) return rc;
	if (kind != VK_SIGNAL_FILTER_MAX && kind != VK_SIGNAL_FILTER_CONV) return fail(VK_ERR_INVALID, "vk_signal_filter: unknown filter kind " + std::to_string(kind));
	if (width < 1 || width > vk_host::kSalMaxWidth) return fail(VK_ERR_INVALID, "vk_signal_filter: width must be 1 .. 4096");
	if (kind == VK_SIGNAL_FILTER_CONV && !pulse) return fail(VK_ERR_INVALID, "vk_signal_filter: a convolution needs its pulse");
	if (!doc_off) return fail(VK_ERR_INVALID, "vk_signal_filter: doc_off is null");
	const char *why = "";
	if (vk_host::sal_check_docs(doc_off, n_docs, c->desc.n_sentences, &why)) return fail(VK_ERR_INVALID, std::string("vk_signal_filter: ") + why);
	if (c->signal_buf[slot] < 0) return fail(VK_ERR_STATE, "vk_signal_filter: the slot holds no signal");
	vk_devbuf<int64_t> d_off;
	vk_devbuf<double> d_pulse;
	return signal_run(c, [&]() -> int {
		hipStream_t st = c->stream;
		int rc;
		if (c->desc.n_sentences == 0) return VK_OK;
		if ((rc = d_off.reserve((size_t)n_docs + 1, nullptr))) return rc;
		VK_HIP(hipMemcpyAsync(d_off, doc_off, ((size_t)n_docs + 1) * 8, hipMemcpyHostToDevice, st));
		if (kind == VK_SIGNAL_FILTER_CONV) {
			if ((rc = d_pulse.reserve((size_t)width, nullptr))) return rc;
			VK_HIP(hipMemcpyAsync(d_pulse, pulse, (size_t)width * 8, hipMemcpyHostToDevice, st));
		}
		const int to = free_signal_buffer(c);
		if ((rc = c->d_signal[to].reserve((size_t)c->desc.n_sentences, &c->device_bytes))) return rc;
		VK_HIP(vk_launch_signal_filter(c->d_signal[c->signal_buf[slot]], c->d_signal[to], d_off, n_docs, c->desc.n_sentences, kind, width,
			kind == VK_SIGNAL_FILTER_CONV ? (const double *)d_pulse : nullptr, st));
		VK_HIP(hipStreamSynchronize(st));
		c->signal_buf[slot] = to;   // (the buffer it leaves is the next filter's)
		return VK_OK;
	});
}

int vk_corpus_set_saliency(vk_corpus_t *c, const int32_t *slots, const double *weights, int32_t n, float *boost_out) {
	if (int rc = signal_call_ok(c, 0, "vk_corpus_set_saliency")) return rc;
	if (c->is_view) return fail(VK_ERR_STATE, "vk_corpus_set_saliency: the booster is set on the owning handle (its views share it)");
	if (n < 0 || n > VK_MAX_SIGNALS || (n > 0 && !slots) || !weights) return fail(VK_ERR_INVALID, "vk_corpus_set_saliency: 0 .. VK_MAX_SIGNALS slots and their weights");
	VkBoostAverageArgs a{};
	for (int32_t k = 0; k <= n; k++) {
		if (!(weights[k] >= 0.0) || !std::isfinite(weights[k])) return fail(VK_ERR_INVALID, "vk_corpus_set_saliency: weights must be finite and not negative");
		a.weights[k] = weights[k];
	}
	a.wsum = vk_host::sal_numpy_sum(weights, (int64_t)n + 1);
	if (!(a.wsum > 0.0)) return fail(VK_ERR_INVALID, "vk_corpus_set_saliency: the weights sum to 0");
	for (int32_t k = 0; k < n; k++) {
		if (slots[k] < 0 || slots[k] >= VK_MAX_SIGNALS) return fail(VK_ERR_INVALID, "vk_corpus_set_saliency: slot must be 0 .. VK_MAX_SIGNALS - 1");
		if (c->signal_buf[slots[k]] < 0) return fail(VK_ERR_STATE, "vk_corpus_set_saliency: slot " + std::to_string(slots[k]) + " holds no signal");
		a.signals[k] = c->d_signal[c->signal_buf[slots[k]]];
	}
	a.n_signals = n;
	const int64_t ns = c->desc.n_sentences, ne = c->n_entries;
	vk_resident_boost &res = *c->resident;
	vk_devbuf<int32_t> d_entry, d_bad;
	vk_devbuf<float> d_slices;
	std::vector<float> host((size_t)std::max<int64_t>(ns, 1), 1.0f);   // (never empty: its address names the resident booster)
	int32_t bad = 0;
	const int rc = signal_run(c, [&]() -> int {
		hipStream_t st = c->stream;
		int rc;
		if (!c->entry_sent.empty()) {
			if ((rc = d_entry.reserve((size_t)ne, nullptr))) return rc;
			VK_HIP(hipMemcpyAsync(d_entry, c->entry_sent.data(), (size_t)ne * 4, hipMemcpyHostToDevice, st));
			a.entry_sent = d_entry;
		}
		if ((rc = d_slices.reserve((size_t)ns, nullptr)) || (rc = d_bad.reserve(4, nullptr))) return rc;
		VK_HIP(hipMemsetAsync(d_bad, 0, 16, st));
		res.active = false;   // from here on the rows change: a failure leaves the corpus without a booster, not with half of one
		if ((rc = res.rows.reserve((size_t)ne + 8, nullptr))) return rc;
		a.n_entries = ne; a.rows = res.rows; a.slices = d_slices; a.bad = d_bad;
		VK_HIP(vk_launch_boost_average(&a, st));
		if (ns > 0) VK_HIP(hipMemcpyAsync(host.data(), d_slices, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
		VK_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
		VK_HIP(hipStreamSynchronize(st));
		return VK_OK;
	});
	const int64_t counted = (int64_t)(res.rows.capacity() * sizeof(float));
	c->device_bytes += counted - res.counted;
	res.counted = counted;
	if (rc) { res.host.clear(); return rc; }
	res.host.swap(host);
	res.nonneg = bad == 0;
	res.active = true;
	if (boost_out && ns > 0) memcpy(boost_out, res.host.data(), (size_t)ns * 4);
	for (int k = 0; k < VK_MAX_SIGNALS; k++) c->signal_buf[k] = -1;
	for (auto &b : c->d_signal) b.reset();
	return VK_OK;
}

int vk_corpus_clear_saliency(vk_corpus_t *c) {
	if (int rc = signal_call_ok(c, 0, "vk_corpus_clear_saliency")) return rc;
	if (c->is_view) return fail(VK_ERR_STATE, "vk_corpus_clear_saliency: the booster is cleared on the owning handle (its views share it)");
	VK_HIP(hipSetDevice(c->device));
	vk_resident_boost &res = *c->resident;
	res.active = false;
	res.nonneg = true;
	res.host.clear();
	res.rows.reset();
	c->device_bytes -= res.counted;
	res.counted = 0;
	return VK_OK;
}

// The filtered corpus: keep flags and their scan on the device, slice table re-indexed, token rows / ids / codes /
// magnitudes gathered.  A handle of its own (stream, workspaces); the static layout shares the vocabulary arrays.
int vk_corpus_filter(vk_corpus_t *src, uint64_t pos_mask, uint64_t tag_mask, vk_corpus_t **out) {
	if (!src || !out) return fail(VK_ERR_INVALID, "null argument");
	if (!src->finalized) return fail(VK_ERR_STATE, "corpus not finalized");
	// (a filtered span would be a slice without a row: no query on such a handle is span-shaped, and the copy of the unmodified rows
	// is not filtered)
	if (src->span_sim.active()) return fail(VK_ERR_UNSUPPORTED, "token filters on a handle under a span similarity (vk_corpus_set_span_sim): a span is one row");
	if (pos_mask && !src->d_pos) return fail(VK_ERR_STATE, "pos filter needs vk_corpus_set_token_pos");
	if (tag_mask && !src->d_tag) return fail(VK_ERR_STATE, "tag filter needs vk_corpus_set_token_tags");
	VK_HIP(hipSetDevice(src->device));
	hipStream_t st = src->stream;
	const int64_t n = src->desc.n_tokens, ne = src->n_entries, ns = src->desc.n_sentences;
	const bool is_static = src->desc.layout == VK_LAYOUT_STATIC;

	int32_t *keep = nullptr, *new_index = nullptr, *src_of = nullptr, *fs = nullptr, *fe = nullptr;
	void *temp = nullptr;
	vk_corpus *c = nullptr;
	int rc = VK_OK;
	auto body = [&]() -> int {
		VK_HIP(hipMalloc((void **)&keep, ((size_t)n + 1) * 4));
		VK_HIP(hipMalloc((void **)&new_index, ((size_t)n + 1) * 4));
		VK_HIP(hipMalloc((void **)&src_of, ((size_t)n + 1) * 4));
		VK_HIP(hipMalloc((void **)&fs, ((size_t)ne + 1) * 4));
		VK_HIP(hipMalloc((void **)&fe, ((size_t)ne + 1) * 4));
		size_t temp_bytes = 0;
		VK_HIP(vk_launch_filter_scan(nullptr, nullptr, 0, 0, n, keep, new_index, nullptr, &temp_bytes, st));
		VK_HIP(hipMalloc(&temp, temp_bytes ? temp_bytes : 16));
		VK_HIP(vk_launch_filter_scan(src->d_pos, src->d_tag, pos_mask, tag_mask, n, keep, new_index, temp, &temp_bytes, st));
		VK_HIP(vk_launch_filter_maps(keep, new_index, n, src_of, src->d_sent_start, src->d_sent_end, ne, fs, fe, st));
		int32_t n_kept32 = 0;
		std::vector<int32_t> hs((size_t)ne), he((size_t)ne);
		VK_HIP(hipMemcpyAsync(&n_kept32, new_index + n, 4, hipMemcpyDeviceToHost, st));
		if (ne > 0) {
			VK_HIP(hipMemcpyAsync(hs.data(), fs, (size_t)ne * 4, hipMemcpyDeviceToHost, st));
			VK_HIP(hipMemcpyAsync(he.data(), fe, (size_t)ne * 4, hipMemcpyDeviceToHost, st));
		}
		VK_HIP(hipStreamSynchronize(st));
		const int64_t n_kept = n_kept32;

		// slices of the filtered stream, per sentence (rows of the source's table that are padding carry no sentence)
		std::vector<int64_t> start((size_t)ns), end((size_t)ns);
		for (int64_t e = 0; e < ne; e++) {
			const int64_t sent = src->entry_sent.empty() ? e : src->entry_sent[(size_t)e];
			if (sent >= 0 && sent < ns) { start[(size_t)sent] = hs[(size_t)e]; end[(size_t)sent] = he[(size_t)e]; }
		}

		vk_corpus_desc desc = src->desc;
		desc.n_tokens = n_kept;
		if (is_static) {
			// token ids and slices are this handle's, the vocabulary (tiles, magnitudes) stays the source's
			c = new vk_corpus();
			c->desc = desc; c->device = src->device;
			c->shared = std::make_shared<vk_devblock>();
			c->shared->device = src->device;
			c->resident = std::make_shared<vk_resident_boost>();   // (a booster is per slice of ITS corpus: a filtered corpus starts without one)
			c->d_pad = src->d_pad; c->nk32 = src->nk32; c->tail = src->tail; c->tile_bytes = src->tile_bytes; c->prec = src->prec;
			c->rows_total = c->rows_appended = src->rows_total; c->n_tiles = src->n_tiles;
			c->d_tiles = src->d_tiles; c->d_mag = src->d_mag; c->shares_vectors = true;
			c->vectors_of = src->shares_vectors ? src->vectors_of : src->shared;   // the vocabulary stays alive with this handle
			c->sim_ops = src->sim_ops;   // the source's similarity
			c->sim_src = src->sim_src; c->raw_rows = src->raw_rows; c->raw_tile_bytes = src->raw_tile_bytes;   // ... and the unmodified rows it may read
			c->sim_mix = src->sim_mix;   // ... and its combinator with the operands' rows
			for (int m = 0; m < VK_MAX_SIM_OPERANDS - 1; m++) c->operands[m] = src->operands[m];
			if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return fail(VK_ERR_HIP, "hipStreamCreate failed");
			for (auto &e : c->ev) if (hipEventCreate(&e) != hipSuccess) return fail(VK_ERR_HIP, "hipEventCreate failed");
			int r;
			if ((r = alloc_shared(c, &c->d_tok_id, (size_t)n_kept + 64))) return r;
			if ((r = reserve_query_workspaces(c))) return r;
			VK_HIP(hipMemsetAsync(c->d_tok_id, 0, ((size_t)n_kept + 64) * 4, st));
			VK_HIP(vk_launch_filter_gather(src->d_tok_id, c->d_tok_id, 4, src_of, n_kept, st));
			c->have_ids = true;
		} else {
			int r = vk_corpus_create(&desc, &c);
			if (r) return r;
			c->sim_ops = src->sim_ops;   // the source's chain (vk_corpus_set_contextual_sim_ops)
			VK_HIP(hipStreamSynchronize(c->stream));   // the zero fill of the new tiles
			VK_HIP(vk_launch_filter_rows(src->d_tiles, c->d_tiles, src_of, n_kept, src->tile_bytes, st));
			if (src->d_mag && c->d_mag) VK_HIP(vk_launch_filter_gather(src->d_mag, c->d_mag, 4, src_of, n_kept, st));
			c->rows_appended = c->rows_total;
		}
		for (int which = 0; which < 2; which++) {
			int8_t *from = which ? src->d_tag : src->d_pos;
			int8_t **to = which ? &c->d_tag : &c->d_pos;
			if (!from) continue;
			int r = alloc_shared(c, to, (size_t)n_kept + 64);
			if (r) return r;
			VK_HIP(hipMemsetAsync(*to, 0, (size_t)n_kept + 64, st));
			VK_HIP(vk_launch_filter_gather(from, *to, 1, src_of, n_kept, st));
		}
		VK_HIP(hipStreamSynchronize(st));
		if (is_static) {
			c->h_tok = std::make_shared<std::vector<int32_t>>((size_t)n_kept);
			if (n_kept > 0) VK_HIP(hipMemcpy(c->h_tok->data(), c->d_tok_id, (size_t)n_kept * 4, hipMemcpyDeviceToHost));
		}
		if (c->d_tag) {
			c->h_tag = std::make_shared<std::vector<int8_t>>((size_t)n_kept);
			if (n_kept > 0) VK_HIP(hipMemcpy(c->h_tag->data(), c->d_tag, (size_t)n_kept, hipMemcpyDeviceToHost));
		}
		int r = set_slices_impl(c, start.data(), end.data(), ns, src->contiguous);
		if (r) return r;
		c->finalized = true;
		return VK_OK;
	};
	rc = body();
	for (void *p : {(void *)keep, (void *)new_index, (void *)src_of, (void *)fs, (void *)fe, temp}) if (p) (void)hipFree(p);
	if (rc) { if (c) vk_corpus_free(c); return rc; }
	*out = c;
	return VK_OK;
}

int vk_last_scores(vk_corpus_t *c, float *scores, int64_t n) {
	if (!c || !scores) return fail(VK_ERR_INVALID, "null argument");
	if (!c->have_scores) return fail(VK_ERR_STATE, "no query has run on this corpus");
	if (n != c->desc.n_sentences) return fail(VK_ERR_INVALID, "n differs from n_sentences");
	VK_HIP(hipSetDevice(c->device));
	if (c->bp.pruned) {
		// the last query scored its contenders only (bound pass): its exact pass over every slice now, once -- the query
		// tile, the gap tables and the boost are still in their workspaces
		VK_HIP(vk_launch_score(&c->bp.full, c->bp.full_grid, c->bp.full_smem, c->stream));
		VK_HIP(hipStreamSynchronize(c->stream));
		c->bp.pruned = false;
	}
	if (c->entry_sent.empty()) {
		VK_HIP(hipMemcpy(scores, c->d_scores, (size_t)n * 4, hipMemcpyDeviceToHost));
		return VK_OK;
	}
	std::vector<float> rows((size_t)c->n_entries);
	VK_HIP(hipMemcpy(rows.data(), c->d_scores, rows.size() * 4, hipMemcpyDeviceToHost));
	for (int64_t e = 0; e < c->n_entries; e++)
		if (c->entry_sent[(size_t)e] >= 0) scores[c->entry_sent[(size_t)e]] = rows[(size_t)e];
	return VK_OK;
}

// Internal (tests; not part of the ABI): the bounds of the last query's bound pass per slice (null: none wanted; n = n_sentences) and
// counters[7] -- the last query: bound pass ran, candidates of round 1 and of round 2, fell back to the full pass; since the handle
// was made: queries with a bound pass, fallbacks, candidates of round 2.
int vk_bound_pass_state(vk_corpus_t *c, float *bounds, int64_t n, int64_t *counters) {
	if (!c || !counters) return fail(VK_ERR_INVALID, "null argument");
	const int64_t v[7] = {c->bp.ran, c->bp.round1, c->bp.round2, c->bp.fell_back, c->bp.queries, c->bp.fallbacks, c->bp.survivors};
	memcpy(counters, v, sizeof v);
	if (!bounds) return VK_OK;
	if (!c->bp.ran) return fail(VK_ERR_STATE, "the last query ran no bound pass");
	if (n != c->desc.n_sentences) return fail(VK_ERR_INVALID, "n differs from n_sentences");
	VK_HIP(hipSetDevice(c->device));
	std::vector<float> rows((size_t)c->n_entries);
	VK_HIP(hipMemcpy(rows.data(), c->d_ub, rows.size() * 4, hipMemcpyDeviceToHost));
	for (int64_t e = 0; e < c->n_entries; e++) {
		const int64_t sent = c->entry_sent.empty() ? e : (int64_t)c->entry_sent[(size_t)e];
		if (sent >= 0) bounds[sent] = rows[(size_t)e];
	}
	return VK_OK;
}

// Internal (tests; not part of the ABI): the format of the handle's shadow -- 0 none, 8 int8 (MODE 7), 6 E2M3 (MODE 8, or MODE 9 where
// vk_bound_pass_shadow reports tiles of 3,712 bytes) -- which is
// the format of every bound pass vk_bound_pass_state reports on
int vk_bound_pass_bits(vk_corpus_t *c, int64_t *bits) {
	if (!c || !bits) return fail(VK_ERR_INVALID, "null argument");
	*bits = c->shadow ? c->shadow_format.bits : 0;
	return VK_OK;
}

// Internal (tests; not part of the ABI): K where the last query's bound pass ran a flat-tailed form (general gaps under a slice-gap
// table flat beyond K entries), else 0
int vk_bound_pass_tail(vk_corpus_t *c, int32_t *k) {
	if (!c || !k) return fail(VK_ERR_INVALID, "null argument");
	*k = c->bp.ran ? (int32_t)c->bp.tail_k : 0;
	return VK_OK;
}

// Internal (tests; not part of the ABI): 1 where the last query's bound pass ran vk_score_local_kernel (the compact 6-bit shadow, general
// gaps under the flat tail, local alignment, VK_BOUND_DP not `generic`: DESIGN 11.12), else 0
int vk_bound_pass_dp(vk_corpus_t *c, int32_t *out) {
	if (!c || !out) return fail(VK_ERR_INVALID, "null argument");
	*out = c->bp.ran ? (int32_t)c->bp.fast_dp : 0;
	return VK_OK;
}

// Internal (tests; not part of the ABI): the handle's shadow as the device holds it.  format[5]: bits (0: no shadow, the rest zero
// then), K-steps per tile, live quarters of the last K-step, bytes per tile, tiles (the zero tile behind the corpus included);
// nx[2]: the corpus-wide constants N and X.  out (null: none wanted): the bytes of tiles tile0 .. tile0 + n - 1.
int vk_bound_pass_shadow(vk_corpus_t *c, int64_t *format, float *nx, int64_t tile0, int64_t n, uint8_t *out) {
	if (!c || !format || !nx) return fail(VK_ERR_INVALID, "null argument");
	const vk_host::shadow_format &sf = c->shadow_format;
	const int64_t f[5] = {sf.bits, sf.steps, sf.live, sf.tile_bytes(), c->n_tiles};
	memset(format, 0, sizeof f);
	nx[0] = nx[1] = 0.0f;
	if (!c->shadow) return out ? fail(VK_ERR_STATE, "the corpus has no shadow") : VK_OK;
	memcpy(format, f, sizeof f);
	nx[0] = c->shadow_n; nx[1] = c->shadow_x;
	if (!out) return VK_OK;
	if (tile0 < 0 || n < 0 || tile0 > c->n_tiles || n > c->n_tiles - tile0) return fail(VK_ERR_INVALID, "tiles out of range");
	VK_HIP(hipSetDevice(c->device));
	VK_HIP(hipStreamSynchronize(c->stream));
	if (n > 0) VK_HIP(hipMemcpy(out, c->shadow + tile0 * sf.tile_bytes(), (size_t)n * sf.tile_bytes(), hipMemcpyDeviceToHost));
	return VK_OK;
}

// Internal (tests; not part of the ABI): which route the last vk_query_batch on this handle took and in which form -- state[VK_BS_COUNT]
// in the order of vk_batch_state_index (all zero: no batch yet)
int vk_batch_state(vk_corpus_t *c, int64_t *state) {
	if (!c || !state) return fail(VK_ERR_INVALID, "null argument");
	memcpy(state, c->batch_state, sizeof c->batch_state);
	return VK_OK;
}

// Internal (tests; not part of the ABI): queries per LDS fill of the span pass over tiles of tile_bytes (vk_span_batch_host.h; 0: none)
int32_t vk_span_batch_fill_queries(int32_t tile_bytes) { return vk_host::span_batch_fill_queries(tile_bytes); }

// Internal (tests; not part of the ABI): the route of the last vk_query on this handle -- state[VK_QR_COUNT] in the order of
// vk_query_route_index (all zero: no query yet)
int vk_query_route(vk_corpus_t *c, int64_t *state) {
	if (!c || !state) return fail(VK_ERR_INVALID, "null argument");
	memcpy(state, c->query_route, sizeof c->query_route);
	return VK_OK;
}

// Internal (tests): one v_mfma_i32_16x16x64_i8 on 16 x 64 int8 query rows and 16 x 64 int8 token rows (host, row-major), packed as
// the shadow packs its blocks: out[16 j + i] = q[j] . x[i]
int vk_i8_tile_probe(const int8_t *q, const int8_t *x, int32_t *out) {
	if (!q || !x || !out) return fail(VK_ERR_INVALID, "null argument");
	vk_devbuf<uint8_t> buf;
	if (int rc = buf.reserve(4096, nullptr)) return rc;
	uint8_t *d = buf;
	VK_HIP(hipMemcpy(d, q, 1024, hipMemcpyHostToDevice));
	VK_HIP(hipMemcpy(d + 1024, x, 1024, hipMemcpyHostToDevice));
	VK_HIP(vk_launch_i8_probe((const int8_t *)d, (const int8_t *)d + 1024, (int32_t *)(d + 2048), nullptr));
	VK_HIP(hipDeviceSynchronize());
	VK_HIP(hipMemcpy(out, d + 2048, 1024, hipMemcpyDeviceToHost));
	return VK_OK;
}

// Internal (tests): one shadow tile of nk64 K-steps (5 or 12) through the bound kernel's own product (dot_tile_i8, vk_common.hip.h) with
// `live` quarters of the last block fetched.  q, x: 16 rows x 64 nk64 int8 each (host, row-major), packed as the shadow packs its
// blocks: out[16 j + i] = q[j] . x[i] over the features the kernel reads
int vk_i8_bound_tile_probe(const int8_t *q, const int8_t *x, int32_t nk64, int32_t live, int32_t *out) {
	if (!q || !x || !out) return fail(VK_ERR_INVALID, "null argument");
	if ((nk64 != 5 && nk64 != 12) || live < 1 || live > 4) return fail(VK_ERR_INVALID, "nk64 is 5 or 12, live 1 .. 4");
	const size_t tb = (size_t)nk64 * 1024;
	vk_devbuf<uint8_t> buf;
	if (int rc = buf.reserve(2 * tb + 1024, nullptr)) return rc;
	uint8_t *d = buf;
	std::vector<uint8_t> pk(2 * tb);
	for (int side = 0; side < 2; side++)
		for (int i = 0; i < 16; i++)
			vk_host::i8_put_row(pk.data() + side * tb, i, (const uint8_t *)(side ? x : q) + (size_t)i * nk64 * 64, nk64 * 64);
	VK_HIP(hipMemcpy(d, pk.data(), 2 * tb, hipMemcpyHostToDevice));
	VK_HIP(vk_launch_i8_bound_probe(d, d + tb, nk64, live, (int32_t *)(d + 2 * tb), nullptr));
	VK_HIP(hipDeviceSynchronize());
	VK_HIP(hipMemcpy(out, d + 2 * tb, 1024, hipMemcpyDeviceToHost));
	return VK_OK;
}

// Internal (tests): one tile through the 6-bit bound kernel's own product (dot_tile_fp6, vk_common.hip.h).  q, x: 16 rows x 384 E2M3
// codes each (host, row-major, one code per byte); the query tile is packed whole, the token tile with `live6` quarters of its last
// K-step as the shadow packs it (vk_host::fp6_put_row) -- and the query's codes at features >= 256 + 32 live6 stay in its tile:
// out[16 j + i] = q[j] . x[i] in grid values over the features the kernel reads
int vk_fp6_bound_tile_probe(const uint8_t *q, const uint8_t *x, int32_t live6, float *out) {
	if (!q || !x || !out) return fail(VK_ERR_INVALID, "null argument");
	if (live6 < 1 || live6 > 4) return fail(VK_ERR_INVALID, "live6 is 1 .. 4");
	const size_t xoff = VK_DEV_FP6_QTILE_BYTES, ooff = xoff + 5120;
	vk_devbuf<uint8_t> buf;
	if (int rc = buf.reserve(ooff + 1024, nullptr)) return rc;
	uint8_t *d = buf;
	std::vector<uint8_t> pk(ooff, 0);
	for (int i = 0; i < 16; i++) {
		vk_host::fp6_put_row(pk.data(), 4, i, q + (size_t)i * 384, 384);
		vk_host::fp6_put_row(pk.data() + xoff, live6, i, x + (size_t)i * 384, 256 + 32 * live6);
	}
	static_assert(VK_DEV_FP6_QTILE_BYTES % 128 == 0 && VK_DEV_FP6_TILE_BYTES(4) <= 5120, "the probe's buffer");
	VK_HIP(hipMemcpy(d, pk.data(), ooff, hipMemcpyHostToDevice));
	VK_HIP(vk_launch_fp6_bound_probe(d, d + xoff, live6, (float *)(d + ooff), nullptr));
	VK_HIP(hipDeviceSynchronize());
	VK_HIP(hipMemcpy(out, d + ooff, 1024, hipMemcpyDeviceToHost));
	return VK_OK;
}

// Internal (tests): the same through MODE 9's loads (dot_tile_fp6<true>).  The token tile is packed compact (vk_host::fp6c_put_row:
// x's codes at features >= d are left out, d <= 304) and every byte of the buffer behind the tile's 3,712 is `fill`: a lane that read
// past the tile would carry it into the product
int vk_fp6c_bound_tile_probe(const uint8_t *q, const uint8_t *x, int32_t d, int32_t fill, float *out) {
	if (!q || !x || !out) return fail(VK_ERR_INVALID, "null argument");
	if (d < 0 || d > 304) return fail(VK_ERR_INVALID, "d is 0 .. 304");
	const size_t xoff = VK_DEV_FP6_QTILE_BYTES, ooff = xoff + 5120;
	vk_devbuf<uint8_t> buf;
	if (int rc = buf.reserve(ooff + 1024, nullptr)) return rc;
	uint8_t *dv = buf;
	std::vector<uint8_t> pk(ooff, 0);
	for (int i = 0; i < 16; i++) {
		vk_host::fp6_put_row(pk.data(), 4, i, q + (size_t)i * 384, 384);
		vk_host::fp6c_put_row(pk.data() + xoff, i, x + (size_t)i * 384, d);
	}
	memset(pk.data() + xoff + VK_DEV_FP6C_TILE_BYTES, fill, 5120 - VK_DEV_FP6C_TILE_BYTES);
	VK_HIP(hipMemcpy(dv, pk.data(), ooff, hipMemcpyHostToDevice));
	VK_HIP(vk_launch_fp6c_bound_probe(dv, dv + xoff, (float *)(dv + ooff), nullptr));
	VK_HIP(hipDeviceSynchronize());
	VK_HIP(hipMemcpy(out, dv + ooff, 1024, hipMemcpyDeviceToHost));
	return VK_OK;
}

int vk_last_timings(const vk_corpus_t *c, vk_timings *t) {
	if (!c || !t) return fail(VK_ERR_INVALID, "null argument");
	*t = c->last;
	return VK_OK;
}

} // extern "C"
