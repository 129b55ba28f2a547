// vk_internal.h -- shared by the host-side units of the C-ABI (vk_corpus.cpp, vk_query.cpp, vk_batch.cpp):
// error reporting, small conversions, the corpus handle.  Internal; the public interface is include/vectorian_hip.h.
#ifndef VK_INTERNAL_H
#define VK_INTERNAL_H

#include "../../include/vectorian_hip.h"
#include "vk_device.h"
#include "vk_devbuf.h"
#include "vk_guard.h"
#include "vk_result_host.h"
#include "vk_bound_host.h"
#include "vk_route_host.h"
#include "vk_span_batch_host.h"
#include "vk_span_sim_host.h"
#include "vk_sim_ops_host.h"
#include "vk_saliency_host.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

std::string &vk_error_slot();   // the calling thread's last error message (vk_corpus.cpp)

namespace {

int fail(int code, const std::string &msg) {
	vk_error_slot() = msg;
	return code;
}

#define VK_HIP(call) \
	do { \
		hipError_t e_ = (call); \
		if (e_ != hipSuccess) { \
			char buf_[512]; \
			snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
			return fail(VK_ERR_HIP, buf_); \
		} \
	} while (0)

uint16_t f32_to_bf16(float x) {
	uint32_t u;
	memcpy(&u, &x, 4);
	if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
	u += 0x7fffu + ((u >> 16) & 1u);
	return (uint16_t)(u >> 16);
}

float bf16_to_f32(uint16_t b) {
	uint32_t u = ((uint32_t)b) << 16;
	float f;
	memcpy(&f, &u, 4);
	return f;
}

using vk_host::gap_cost;

constexpr int kTopkChunk = 2048;
constexpr int kGapTable = 640;   // entries of the gap tables sent to the device (> VK_MAX_SENT_LEN)
constexpr int64_t kStageBytes = 64ll << 20;
// The 8-bit bound pass.  VK_BOUND_PASS, read at finalize and per query: "off" no shadow and no bound pass, "force" both
// whatever the corpus size, anything else the default -- from kBoundPassMinSentences slices on.  1,000,000 is the one size at which
// the path has been measured against the exact pass (1.8 x); smaller corpora pay the shadow's + 54 % bytes, one more
// host synchronisation and about ten small launches per query for a gain nobody has measured, so they stay on the exact pass
// unless the caller asks (force).  Lower it only from a sweep of sizes recorded under profiles/.
constexpr int64_t kBoundPassMinSentences = 1000000;
constexpr int64_t kBoundRound2Floor = 1024; // round 2 rescores up to max(n / 16, this) slices; more: the full exact pass instead
inline int bound_pass_mode() {
	const char *e = getenv("VK_BOUND_PASS");
	return !e ? 0 : !strcmp(e, "off") ? -1 : !strcmp(e, "force") ? 1 : 0;
}
// VK_BOUND_BITS, read at finalize: which shadow a corpus of 289 .. 304 features gets -- "8" the int8 one, "6" the E2M3 one in
// 3,968-byte tiles, "6c" the E2M3 one in compact 3,712-byte tiles.
// Unset: 8 under VK_BOUND_PASS=force (the sizes below a million slices have been measured with 8 only, and the tests of the 8-bit
// pass run under force), 6c where the pass is switched on by size (profiles/bound_fp6_ab.json: - 8.9 % per query at 1 M slices for
// six bits, profiles/bound_compact_ab.json: a further - 4.6 % for the compact tiles).
// 753 .. 768 features: always 8.  A corpus carries one shadow.  The value is the bits_wanted of vk_host::shadow_format_of.
inline int bound_bits_wanted(int mode) {
	const char *e = getenv("VK_BOUND_BITS");
	if (e && !strcmp(e, "6c")) return vk_host::bits6_compact;
	if (e && !strcmp(e, "6")) return 6;
	if (e && !strcmp(e, "8")) return 8;
	return mode > 0 ? 8 : vk_host::bits6_compact;
}
// VK_BOUND_TAIL, read per query: whether the bound pass of a query with general gaps scores under the flat-tailed slice-gap table
// (vk_host::bound_tail_choice, by the same rule: the default is on where the pass is switched on by size)
inline bool bound_tail_wanted(int mode) { return vk_host::bound_tail_choice(getenv("VK_BOUND_TAIL"), mode); }

} // namespace

// Device arrays that several handles read -- a corpus, its views (vk_corpus_view), the filtered corpora of a static layout
// (vk_corpus_filter shares the vocabulary vectors): owned by a refcounted block, freed when the LAST handle that names them is
// freed.  The order in which a caller (or a garbage collector) frees the handles of one corpus therefore cannot matter; the reference
// keeps its results alive the same way (shared_ptr graph, vectorian/core/cpp/result_set.h:17-30).
struct vk_devblock {
	int device = 0;
	std::mutex mu;
	std::vector<void *> ptrs;
	void add(void *p) { std::lock_guard<std::mutex> g(mu); ptrs.push_back(p); }
	void release(void *p);   // free one array now (the slice table is re-created when the slices are set again before finalize)
	~vk_devblock();
};

// The ring of the handles on one corpus (vk_corpus::peer) is read by every query of every handle and written by vk_corpus_view /
// vk_corpus_free, from whichever threads the caller uses: one mutex around insert, unlink and the peer's turn-taking event.
std::mutex &vk_ring_mutex();

// What a view takes over from its source (vk_corpus_view assigns this part in one statement): the description of the resident corpus,
// the aliases of the arrays several handles read and their owners, the host mirrors.  Nothing a handle has for itself belongs here --
// no workspace, event, stream, lazily built layout or ring link.
// The resident booster of a corpus (vk_corpus_set_saliency): one block that the owning handle and its views hold together --
// what the owner sets or clears, the views see.  `rows`: the booster per row of the slice table, as upload_boost lays a caller's array
// out (padding rows: 1); `host`: per slice, what the winners' restated scores read; `nonneg`: every boost >= 0 and none NaN, computed
// where the booster was (the bound pass's precondition).  Counted in the owner's device_bytes by hand, as raw_rows is.
struct vk_resident_boost {
	bool active = false, nonneg = true;
	vk_devbuf<float> rows;
	std::vector<float> host;
	int64_t counted = 0;
};

struct vk_corpus_shape {
	vk_corpus_desc desc{};
	int device = 0;
	int d_pad = 0, nk32 = 0, tail = 0, tile_bytes = 0;
	int prec = 0;                // vk_precision: 1 = fp32 tiles (nk32 then counts blocks of 16 features, tail = 0)
	int64_t rows_total = 0, rows_appended = 0, n_tiles = 0;
	uint8_t *d_tiles = nullptr;
	float *d_mag = nullptr;
	int32_t *d_tok_id = nullptr;
	int8_t *d_pos = nullptr;   // POS code per token (tag-weighted queries, token filters)
	int8_t *d_tag = nullptr;   // tag code per token (token filters)
	int32_t *d_sent_start = nullptr, *d_sent_end = nullptr;
	// host mirrors, shared by the views of a corpus: rows of the slice table (as on the device, padding included), token ids and tag
	// codes of the static layout -- what restating a transport winner on the host needs (vk_transport_host.h)
	std::shared_ptr<std::vector<int32_t>> h_start, h_end, h_tok;
	std::shared_ptr<std::vector<int8_t>> h_tag;
	bool contiguous = false;   // slices are the CSR partition of the token stream
	bool overlapping = false;  // some token belongs to more than one slice (sliding windows)
	bool have_ids = false, have_sent = false;
	int max_len = 0, max_group_tiles = 0, max_group_tokens = 0;
	int max_pair_tiles = 0;    // tiles spanned by two consecutive rows of the slice table (vk_score32_kernel)
	int max_short_pair_tiles = 0;   // ... leaving out the groups that hold a long slice
	// slice table on the device: n_entries >= n_sentences rows.  Slices longer than VK_FAST_SENT_LEN sit alone in
	// their group of 4 (padded with empty rows) and are scored by a second launch over d_long_groups.
	int64_t n_entries = 0;
	std::vector<int32_t> entry_sent;   // [n_entries] sentence of a row, -1 = padding; empty when the table is the identity
	int32_t *d_long_groups = nullptr;
	int n_long_groups = 0, max_short_len = 0, long_group_tiles = 0, long_group_tokens = 0;   // the long pass: slices of 65 .. VK_MAX_SENT_LEN tokens
	int max_long_len = 0;      // ... the longest of them
	std::shared_ptr<std::vector<int32_t>> h_apart;   // rows of the slice table of every group that holds a slice of more than 64 tokens
	std::shared_ptr<std::vector<int32_t>> h_xlong;   // rows of the slice table of slices beyond VK_MAX_SENT_LEN (whole documents)
	int uniform_len = 0;       // > 0: every sentence has exactly this many tokens
	bool shares_vectors = false; // a filtered corpus of the static layout: vocabulary tiles and magnitudes belong to its source
	// who owns the arrays several handles read (d_tiles, d_mag, d_tok_id, d_pos, d_tag, d_sent_start, d_sent_end, d_long_groups):
	// `shared` the block this handle allocates into (a view: its source's), `vectors_of` the block of the source of a filtered
	// static corpus (its vocabulary tiles and magnitudes).  The raw pointers above are aliases into these blocks.
	std::shared_ptr<vk_devblock> shared, vectors_of;
	// the shadow of the token rows (null: none), in `shared` like the tiles, its format (vk_bound_host.h), and the
	// corpus-wide constants of the bound -- shadow_n >= every |s_x xq|, shadow_x >= every |x|
	const uint8_t *shadow = nullptr;
	vk_host::shadow_format shadow_format;
	float shadow_n = 0.0f, shadow_x = 0.0f;
	// the operator chain on the cosine (static layout: vk_corpus_set_sim_ops; contextual: vk_corpus_set_contextual_sim_ops): a
	// view and a filtered corpus start with their source's, after that each handle is set on its own
	vk_host::sim_ops sim_ops{};
	// the source the chain runs on (vk_corpus_set_sim_source; vk_sim_src_host.h), inherited the same way, and -- under a source that
	// is not the cosine -- the second, fp32 copy of the UNMODIFIED rows in the fp32 tile layout: n_tiles tiles of raw_tile_bytes.  An
	// owning buffer that the handles of one vocabulary hold together (views and filtered corpora copy the pointer): it goes with the
	// last of them.  Counted in the device_bytes of the handle that made it, by hand (a buffer's own count would outlive that handle)
	vk_host::sim_src sim_src{};
	std::shared_ptr<vk_devbuf<uint8_t>> raw_rows;
	int raw_tile_bytes = 0;
	// the combinator of a mixed handle (vk_corpus_set_sim_mix; vk_sim_mix_host.h; kind VK_SIMMIX_NONE: none) and its operands 1 ..
	// sim_mix.n - 1 at operands[0 ..] -- operand 0 is the handle itself.  Inherited like source and chain; the rows are owning buffers
	// held together like raw_rows
	vk_host::sim_mix sim_mix{};
	struct sim_operand {
		int d = 0, d_pad = 0, nk32 = 0, tail = 0, tile_bytes = 0;   // the operand's own width in the handle's precision (as the fields above)
		int64_t rows_appended = 0;
		vk_host::sim_src src{};
		vk_host::sim_ops ops{};
		std::shared_ptr<vk_devbuf<uint8_t>> tiles;      // unit rows as tiles, n_tiles of tile_bytes (the zero tile included)
		std::shared_ptr<vk_devbuf<uint8_t>> raw_rows;   // under a source that is not the cosine: the unmodified rows, fp32 tiles of raw_tile_bytes
		int raw_tile_bytes = 0;
	} operands[VK_MAX_SIM_OPERANDS - 1];
	// the span similarity of a VK_LAYOUT_CONTEXTUAL handle of one-row slices (vk_corpus_set_span_sim; vk_span_sim_host.h), in
	// fields of its own: nothing keyed on sim_ops.n > 0 or table_is_canonical() engages for such a handle -- the scoring pass's float IS
	// the result.  Under a source that is not the cosine the handle keeps the unmodified rows in raw_rows, as a static handle does.
	// Views inherit it with the shape.
	vk_host::span_sim span_sim{};
	// the resident booster (made with the handle; a view's is its source's, a filtered corpus has its own, empty one)
	std::shared_ptr<vk_resident_boost> resident;
	// the booster a query without one of its own runs under: the host copy of the resident one, or null.  The query paths see it as
	// the query's boost -- every rule that reads q->boost holds as it stands -- and know it by its address (boost_is_resident)
	const float *resident_boost() const { return resident && resident->active ? resident->host.data() : nullptr; }
	bool boost_is_resident(const float *boost) const { return boost != nullptr && boost == resident_boost(); }
	bool mixed() const { return sim_mix.kind != VK_SIMMIX_NONE; }
	// what the kernels' sim_src says: not the cosine -- read the table's cell -- under a source of the handle's or a combinator
	int dev_sim_src() const { return mixed() ? VK_DEV_SIMSRC_MIXED : sim_src.kind; }
	bool table_is_canonical() const { return dev_sim_src() != VK_SIMSRC_COSINE; }
};

// vk_corpus::batch_state by index (the internal export vk_batch_state hands the array out in this order; the tests name the
// entries in the same order).  Route: 1 query by query, 2 the shared pass, 3 the GEMM pass, 4 the span pass (vk_span_batch_host.h; it
// states n_qtiles and uniform_len).
enum vk_batch_state_index {
	VK_BS_ROUTE,
	VK_BS_QB_MAX, VK_BS_LT, VK_BS_GAP_MODE,                                                     // the shared pass
	VK_BS_STAT, VK_BS_STAT_UNIFORM32, VK_BS_UNIFORM16, VK_BS_B32, VK_BS_R32, VK_BS_GRAN,        // the GEMM pass
	VK_BS_WIDE32, VK_BS_DENSE, VK_BS_QPT, VK_BS_N_QTILES, VK_BS_UNIFORM_LEN, VK_BS_LATE_MASK,
	VK_BS_COUNT
};

// vk_corpus::query_route by index (the internal export vk_query_route hands the array out in this order; the tests name the entries
// in the same order): the route of the last vk_query on the handle as vk_host::route_query decided it (the enums of vk_route_host.h;
// all -1: a query of more than VK_MAX_QUERY_LEN tokens, which vk_longq_host.cpp serves).  VK_QR_PLAN is what ran: PLAN_FUSED where a
// query row that is not finite or a negative boost kept a query off the bound pass it was routed to.
enum vk_query_route_index {
	VK_QR_PLAN, VK_QR_GAP_MODE, VK_QR_WIDE_GAP_MODE, VK_QR_SCORE32_GAP_MODE, VK_QR_WAVE_TILES,
	VK_QR_PASS_SHORT, VK_QR_PASS_MID, VK_QR_PASS_XLONG, VK_QR_LIST, VK_QR_RING_ROWS, VK_QR_FLOW, VK_QR_OSTRIDE, VK_QR_RAW, VK_QR_SPAN_SKIP_RAW,
	VK_QR_COUNT
};

// The handle: the shape above and what is this handle's alone.  Every workspace is a vk_devbuf (vk_devbuf.h): sized by reserve() where
// it is needed, counted in device_bytes while it lives, freed with the handle.
struct vk_corpus : vk_corpus_shape {
	hipStream_t stream = nullptr;
	bool finalized = false;
	std::vector<int32_t> sent_entry;   // the inverse of entry_sent (row of a sentence), built when vk_query_desc.only_slices first needs it
	int64_t device_bytes = 0;    // bytes of device memory this handle has allocated and not freed (declared before the buffers that count into it)
	vk_devbuf<uint8_t> d_bq; vk_devbuf<int32_t> d_bqlen; vk_devbuf<float> d_bscores; vk_devbuf<uint64_t> d_bkeys[2];
	vk_devbuf<float> d_braw;   // aligner scores of a batch of alignment queries
	vk_devbuf<float> d_bspan;  // the score matrix [queries x spans] of a batch of one-token queries (vk_span_batch_kernel): this route's alone
	// workspaces
	vk_devbuf<uint8_t> d_stage;
	vk_devbuf<uint8_t> d_qtile;
	vk_devbuf<float> d_ws, d_wt;   // d_ws: at least kGapTable floats (grown by a query over a corpus with longer slices)
	vk_devbuf<int32_t> d_qids;
	vk_devbuf<float> d_table;
	vk_devbuf<float> d_qraw;      // under a source that is not the cosine: the query's unmodified rows, per tile [16 x d] and 16 sums of |q_k|
	// a mixed handle (vk_corpus_set_sim_mix), per operand 1 ..: its tables of the running query (sized as d_table is), its query
	// tiles and -- under a source -- its query's unmodified rows; and the rows vk_corpus_set_query_operand has left for the next
	// queries, in the order of the calls (vk_query reads entry q_operand_at: 0, or the query's place in a batch run query by query)
	struct mix_operand_bufs {
		vk_devbuf<float> table, qraw;
		vk_devbuf<uint8_t> qtile;
		struct rows { std::vector<uint8_t> bytes; int32_t len_t = 0, dtype = 0, normalize = 0; };
		std::vector<rows> pending;
	} mixop[VK_MAX_SIM_OPERANDS - 1];
	int q_operand_at = 0;
	bool in_batch = false;        // vk_query_batch is running its queries one by one: it clears the pending rows, not vk_query
	void drop_query_operands() { for (auto &m : mixop) m.pending.clear(); q_operand_at = 0; }
	vk_devbuf<float> d_scores, d_raw, d_boost;
	// the booster of a query on the device, per row of the slice table: the resident one, or the query's own in d_boost (upload_boost)
	const float *dev_boost(const float *boost) const { return !boost ? nullptr : boost_is_resident(boost) ? (const float *)resident->rows : (const float *)d_boost; }
	// the signal slots of a Saliency being compiled (vk_signal_*): slot k lives in d_signal[signal_buf[k]] (-1: empty); a filter writes
	// into a free buffer and the slot moves there.  Freed by vk_corpus_set_saliency
	vk_devbuf<float> d_signal[VK_MAX_SIGNALS + 1];
	int signal_buf[VK_MAX_SIGNALS] = {-1, -1, -1, -1, -1, -1, -1, -1};
	vk_devbuf<uint64_t> d_keys[2];
	vk_devbuf<float> d_out_raw, d_out_sim;   // the winners' outputs: at least VK_MAX_MATCHES of them (grown by a query that asks for more matches)
	vk_devbuf<int16_t> d_out_map;
	vk_devbuf<float> d_wrd_raw, d_wrd_val;   // exact transports: one value per candidate
	vk_devbuf<uint32_t> d_counter;
	vk_devbuf<float> d_rows_out, d_plan_out;   // transport flows of the winners
	vk_devbuf<uint8_t> d_bqt; vk_devbuf<uint64_t> d_bcand; vk_devbuf<int32_t> d_bcandq; vk_devbuf<float> d_brows;   // similarity rows of a batch's winners
	vk_devbuf<float, true> h_brows;   // pinned host staging of the similarity rows of a batch's winners
	vk_devbuf<uint32_t> d_qbits;   // tag-weighted vocabulary transports over the static layout: bitmap of the query's token ids
	vk_devbuf<uint8_t> d_wrdl_scratch;   // exact transport, queries of 17..64 tokens over long slices: per-workgroup state
	vk_devbuf<uint8_t> d_wide_scratch;   // vk_wide_kernel, global-state form: per-workgroup state of a slice
	vk_devbuf<int32_t> d_apart_order; int32_t n_apart_order = -1;   // ... over the slices of more than 64 tokens (general gaps: the one-wave-per-slice pass is their fastest kernel)
	vk_devbuf<int32_t> d_xlong_order; int32_t n_xlong_order = -1;   // the same list over the slices beyond VK_MAX_SENT_LEN only (queries of at most 16 tokens: the other slices keep their fused kernels)
	vk_devbuf<int32_t> d_wide_order; int32_t n_wide_order = -1;   // ... its work list: the non-empty rows of the slice table, longest first
	int rows_w = 0;              // columns per similarity row they are sized for (16, 32, 48 or 64)
	// batched GEMM over a ragged corpus (vk_query_batch): a padded copy of the sentences, one bucket per padded length
	// 16 / 32 / 48 / 64 tokens, built on the first such batch (this handle's; about 1.2 x the corpus for lengths 8..64)
	struct batch_bucket { vk_devbuf<uint8_t> tiles; vk_devbuf<int32_t> len, id; int64_t n = 0; };
	batch_bucket bl[4];
	bool bl_built = false;
	int64_t bl_empty = 0;        // slices without tokens (in no bucket: their scores stay -inf)
	// batched relaxed WMD over the static layout (vk_rwmd_static32_kernel): the rows of the slice table by length bucket (1..32 /
	// 33..64 tokens; null lists when every slice has exactly 32 tokens), the batch's similarity table and its diagonal cells
	// the bound pass (vk_query.cpp score_bounded): the query's 8-bit tile, the bound of every row, the groups its rounds rescore
	vk_devbuf<uint8_t> d_qtile8; vk_devbuf<float> d_ub; vk_devbuf<int32_t> d_bound_groups; vk_devbuf<uint64_t> d_bound_keys;
	struct bound_state {
		bool pruned = false;          // d_scores holds the contenders' scores only: vk_last_scores runs `full` first
		VkScoreParams full{}; int full_grid = 0; size_t full_smem = 0;   // the exact pass of the last query (its workspaces stay until the next)
		int64_t ran = 0, round1 = 0, round2 = 0, fell_back = 0;           // the last query: bound pass ran, candidates of the rounds, full pass after all
		int64_t tail_k = 0;                                                // ... under a slice-gap table flat beyond this many entries (0: the caller's table)
		int64_t fast_dp = 0;                                               // ... on vk_score_local_kernel (vk_score_m9f.hip)
		int64_t queries = 0, fallbacks = 0, survivors = 0;                // since the handle was made
		vk_host::bound_backoff backoff;                                    // default mode: when the handle stops trying (vk_bound_host.h)
	} bp;
	vk_devbuf<int32_t> d_sb_id[2]; int64_t sb_n[2] = {0, 0}; bool sb_built = false; int64_t sb_empty = 0;
	vk_devbuf<uint16_t> d_btable;
	vk_devbuf<int64_t> d_bfix;
	vk_devbuf<uint32_t> d_blive;  // ... under an operator chain: per query tile of the batch, the rows that hold a token
	vk_devbuf<int32_t> d_bqids;   // token ids of a batch's queries, 16 per query (the winners' rows: sim[id(t_j)][j] = 1)
	vk_devbuf<uint64_t> d_sort[2]; vk_devbuf<uint8_t> d_sort_temp;   // result sets beyond VK_MAX_MATCHES: all keys, sorted
	// route and form of the last vk_query_batch on this handle (vk_batch_state in vk_corpus.cpp, for the tests; host integers only),
	// addressed by VK_BS_*: the route, then the shared pass's three, then the GEMM pass's twelve
	int64_t batch_state[VK_BS_COUNT] = {};
	int64_t query_route[VK_QR_COUNT] = {};   // ... of the last vk_query (vk_query_route), addressed by VK_QR_*
	hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // 0 start, 5 before / 1 after the wait for the peer's kernel, 2 scored (the peer's turn), 3 selected, 4 done; 6: the batched GEMM has ended (its turn ends after the selection)
	vk_timings last{};
	bool have_scores = false;
	bool is_view = false;        // shares the corpus arrays of another handle (vk_corpus_view)
	// queries of 65 .. VK_MAX_LONG_QUERY_LEN tokens (vk_longq_host.cpp): query tiles, small per-query arrays (floats / ints), the static
	// layout's tables (one per 16 query tokens), scratch of the scoring pass and of the tracebacks, the winners' outputs
	struct longq_bufs {
		vk_devbuf<uint8_t> qt;
		vk_devbuf<float> fl;
		vk_devbuf<int32_t> il;
		vk_devbuf<float> table;
		vk_devbuf<uint8_t> scratch, fscratch;
		vk_devbuf<uint8_t> bscratch;                     // scratch of the block form's scoring pass (slices of 65 .. VK_MAX_SENT_LEN tokens)
		vk_devbuf<int32_t> order; int32_t n_order = -1;   // ... its work list: those rows of the slice table, longest first (-1: not built)
		vk_devbuf<float> raw, sim;
		vk_devbuf<int16_t> map;
	} lq;
	vk_corpus *peer = nullptr;   // ring of the handles on one corpus: a handle's scoring kernel starts after its peer's (under vk_ring_mutex)
	std::atomic<bool> ev2_recorded{false};   // (device-side wait on ev[2]), so that scoring kernels run back to back, never queued inside each other
};

namespace {

// an array the views of this corpus read too: owned by the handle's refcounted block
template <typename T> int alloc_shared(vk_corpus *c, T **p, size_t n) {
	VK_HIP(hipMalloc((void **)p, n ? n * sizeof(T) : 16));
	c->device_bytes += (int64_t)(n * sizeof(T));
	c->shared->add((void *)*p);
	return VK_OK;
}

} // namespace

// units
// this handle's scoring kernel starts when its peer's has finished: a device-side wait on the peer's event, taken under the
// ring's mutex so that the peer cannot be unlinked and destroyed in between (vk_corpus.cpp)
int vk_wait_peer_turn(vk_corpus *c, hipStream_t st);
int vk_validate_query(const vk_corpus *c, const vk_query_desc *q, const vk_topk_out *out);
int vk_longq_query(vk_corpus *c, const vk_query_desc *q, vk_topk_out *out, vk_host_keep &keep);   // vk_longq_host.cpp
// bound_tile: with a shadow, the query's tile in the shadow's format and the cells' constants behind it (left empty when a row is not finite)
void vk_pack_query(const vk_corpus *c, const vk_query_desc *q, std::vector<uint8_t> &tile, float *mags, std::vector<uint8_t> *bound_tile = nullptr);
// ... the query tiles alone, for rows of any width (an operand of a mixed handle has its own): tile_bytes per tile of d features
void vk_pack_query_rows(int d, int tile_bytes, int prec, const void *q_vectors, int q_dtype, int q_normalize, int len_t, std::vector<uint8_t> &tile, float *mags);

// ---- steps the query paths share (vk_query.cpp, vk_longq_host.cpp, vk_batch.cpp); the rules without a device are in vk_result_host.h
namespace {

// The corpus fields every kernel parameter struct has ...
template <typename P> void corpus_fields(P &p, const vk_corpus *c) {
	p.tiles = c->d_tiles; p.sent_start = c->d_sent_start; p.sent_end = c->d_sent_end;
	p.nk32 = c->nk32; p.tail = c->tail; p.tile_bytes = c->tile_bytes;
}
// the handle's operator chain into the structs of the kernels that restate cells of the static layout (the others have no such field)
// (beside it the kind of the handle's source: not the cosine, and those kernels read the table's cells instead)
// (VkScoreParams has the chain alone -- a contextual handle's, DESIGN 19: no source to go with it)
template <typename P> auto sim_ops_field(P &p, const vk_corpus *c, int) -> decltype((void)p.sim_ops, (void)p.sim_src) { p.sim_ops = c->sim_ops; p.sim_src = c->dev_sim_src(); }
template <typename P> auto sim_ops_field(P &p, const vk_corpus *c, long) -> decltype((void)p.sim_ops) { p.sim_ops = c->sim_ops; }
template <typename P> void sim_ops_field(P &, const vk_corpus *, ...) {}
// ... and those of the structs that serve both layouts and both precisions (d_tok_id is null unless the layout is static)
template <typename P> void corpus_fields_ids(P &p, const vk_corpus *c) {
	corpus_fields(p, c);
	sim_ops_field(p, c, 0);
	p.tok_id = c->d_tok_id; p.prec = c->prec;
	p.layout = c->desc.layout == VK_LAYOUT_STATIC ? VK_DEV_LAYOUT_STATIC : VK_DEV_LAYOUT_CONTEXTUAL;
}
// the recurrence's constants (vk_host::gap_form, or another parameter struct) into a parameter struct; gap_mode stays with the caller
template <typename P, typename G> void gap_fields(P &p, const G &g) {
	p.gs = g.gs; p.gt = g.gt; p.a_s = g.a_s; p.a_t = g.a_t; p.open_s = g.open_s; p.open_t = g.open_t;
}

// The tag-weighted modifier's fields of a kernel parameter struct whose tw / tpos arrays hold `cols` query columns, and the reference
// score's total either way: the sum of the query's tag weights (reference_score with max_similarity_for_t = t_pos_weights,
// slice/static.h:280-286), its length without them
inline float ref_total_of(const vk_query_desc *q) {
	if (!q->tag_weights) return (float)q->len_t;
	float total = 0.0f;
	for (int j = 0; j < q->len_t; j++) total += q->tag_weights[j];
	return total;
}
template <typename P> void tag_weight_fields(P &p, const vk_corpus *c, const vk_query_desc *q, int cols) {
	const bool tagged = q->tag_weights != nullptr;
	for (int j = 0; j < cols; j++) {
		p.tw[j] = (tagged && j < q->len_t) ? q->tag_weights[j] : 0.0f;
		p.tpos[j] = (tagged && j < q->len_t) ? (int32_t)q->q_pos[j] : -1;
	}
	p.ref_total = ref_total_of(q);
	if (!tagged) return;
	p.pos_s = c->d_pos; p.tw_keep = 1.0f - q->pos_mismatch_penalty; p.tw_threshold = q->similarity_threshold;
}

// c->last from the events of a query: 0 start, 5 before / 1 after the wait for the peer, `scored` the scoring pass has ended (2; the
// batched GEMM: 6), 3 selected, 4 done.  flow: whether the path has a traceback stage of its own between 3 and 4.
void state_timings(vk_corpus *c, bool flow, int scored = 2) {
	float ms = 0;
	vk_timings t{};
	if (hipEventElapsedTime(&ms, c->ev[0], c->ev[5]) == hipSuccess) t.prepare_ms = ms;
	if (hipEventElapsedTime(&ms, c->ev[5], c->ev[1]) == hipSuccess) t.queue_ms = ms;
	if (hipEventElapsedTime(&ms, c->ev[1], c->ev[scored]) == hipSuccess) t.score_ms = ms;   // (a pruned query: the bound pass; its rounds count below)
	if (hipEventElapsedTime(&ms, c->ev[scored], c->ev[3]) == hipSuccess) t.topk_ms = ms;
	if (flow && hipEventElapsedTime(&ms, c->ev[3], c->ev[4]) == hipSuccess) t.flow_ms = ms;
	if (hipEventElapsedTime(&ms, c->ev[0], c->ev[4]) == hipSuccess) t.total_ms = ms - t.queue_ms;
	c->last = t;
}

// The kk best of d_scores above `floor` as keys, best first, in *d_sel (one of d_keys[0 / 1]).
// Wave-streaming selection (kk <= 64): n -> ceil(n / 4096) * kk keys -> ... -> kk keys
int select_waves(vk_corpus *c, float floor, int kk, hipStream_t st, const uint64_t **d_sel) {
	int64_t nw = 0;
	int cur = 0;
	VK_HIP(vk_launch_topk_wave(c->d_scores, nullptr, c->n_entries, floor, kk, 4096, c->d_keys[0], &nw, st));
	while (nw > 1) {
		const int64_t nkeys = nw * kk;
		const int64_t per_wave = nkeys <= 16384 ? nkeys : 4096;
		VK_HIP(vk_launch_topk_wave(nullptr, c->d_keys[cur], nkeys, 0.0f, kk, per_wave, c->d_keys[1 - cur], &nw, st));
		cur = 1 - cur;
	}
	*d_sel = c->d_keys[cur];
	return VK_OK;
}
// Block selection (kk <= VK_MAX_MATCHES): each block sorts 2,048 keys and keeps its kk best, until one block is left
int select_blocks(vk_corpus *c, float floor, int kk, hipStream_t st, const uint64_t **d_sel, const float *scores = nullptr) {
	int nb = 0, cur = 0;
	VK_HIP(vk_launch_topk_scores(scores ? scores : (const float *)c->d_scores, c->n_entries, floor, kk, c->d_keys[0], &nb, st));
	while (nb > 1) {
		VK_HIP(vk_launch_topk_keys(c->d_keys[cur], (int64_t)nb * kk, kk, c->d_keys[1 - cur], &nb, st));
		cur = 1 - cur;
	}
	*d_sel = c->d_keys[cur];
	return VK_OK;
}

// the caller's boost per slice as d_boost per row of the slice table (padding rows: 1)
// (nonneg: also answers whether every slice's boost is >= 0 -- the bound pass needs it; one more pass over the caller's array, vectorised)
// (the resident booster is on the device already, and its answer with it)
int upload_boost(vk_corpus *c, const float *boost, vk_host_keep &keep, hipStream_t st, bool *nonneg = nullptr) {
	const int64_t n = c->n_entries;
	if (c->boost_is_resident(boost)) {
		if (nonneg) *nonneg = c->resident->nonneg;
		return VK_OK;
	}
	if (nonneg) {
		float least = 0.0f;
		bool nan = false;
		for (int64_t s = 0; s < c->desc.n_sentences; s++) { least = std::min(least, boost[s]); nan = nan || boost[s] != boost[s]; }
		*nonneg = !(least < 0.0f) && !nan;
	}
	if (int rc = c->d_boost.reserve((size_t)n + 8, &c->device_bytes)) return rc;
	if (!c->entry_sent.empty()) {
		std::vector<float> &rows = keep.vec<float>((size_t)n);
		for (int64_t e = 0; e < n; e++) rows[(size_t)e] = c->entry_sent[(size_t)e] >= 0 ? boost[c->entry_sent[(size_t)e]] : 1.0f;
		boost = rows.data();
	}
	VK_HIP(hipMemcpyAsync(c->d_boost, boost, (size_t)n * 4, hipMemcpyHostToDevice, st));
	return VK_OK;
}

// Under a source that is not the cosine: the query's rows as the caller gives them (bf16 widened exactly; q_normalize is the cosine
// tile's alone) for the table kernel -- per 16 query tokens [16 x d] floats and the 16 sums of |q_k| (vk_host::sim_src_abs_sum) -- into
// d_qraw, and the arguments of vk_launch_table for tile t
constexpr size_t vk_source_tile_floats(int d) { return 16 * (size_t)d + 16; }
int upload_source_rows(vk_corpus *c, int d, const void *q_vectors, int q_dtype, int len_t, vk_devbuf<float> &dst, vk_host_keep &keep, hipStream_t st) {
	const int nq = (len_t + 15) / 16;
	const size_t per = vk_source_tile_floats(d);
	std::vector<float> &rows = keep.vec<float>(per * (size_t)nq);
	std::fill(rows.begin(), rows.end(), 0.0f);
	for (int i = 0; i < len_t; i++) {
		float *row = rows.data() + (size_t)(i >> 4) * per + (size_t)(i & 15) * d;
		for (int k = 0; k < d; k++)
			row[k] = q_dtype == VK_F32 ? ((const float *)q_vectors)[(size_t)i * d + k] : bf16_to_f32(((const uint16_t *)q_vectors)[(size_t)i * d + k]);
		rows[(size_t)(i >> 4) * per + 16 * (size_t)d + (size_t)(i & 15)] = vk_host::sim_src_abs_sum(row, d);
	}
	if (int rc = dst.reserve(rows.size(), &c->device_bytes)) return rc;
	VK_HIP(hipMemcpyAsync(dst, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, st));
	return VK_OK;
}
int upload_source_query(vk_corpus *c, const vk_query_desc *q, vk_host_keep &keep, hipStream_t st) {
	return upload_source_rows(c, c->desc.d, q->q_vectors, q->q_dtype, q->len_t, c->d_qraw, keep, st);
}
VkSimSrcArgs source_table_args_of(const vk_host::sim_src &src, const vk_devbuf<uint8_t> *raw_rows, int raw_tile_bytes, int d, const float *qraw, int t) {
	VkSimSrcArgs a{};
	a.src = src; a.raw_tiles = raw_rows ? (const uint8_t *)*raw_rows : nullptr; a.raw_tile_bytes = raw_tile_bytes; a.d = d;
	a.q_rows = qraw + (size_t)t * vk_source_tile_floats(d);
	a.q_abs_sums = a.q_rows + 16 * (size_t)d;
	return a;
}
VkSimSrcArgs source_table_args(const vk_corpus *c, int t) {
	return source_table_args_of(c->sim_src, c->raw_rows.get(), c->raw_tile_bytes, c->desc.d, (const float *)c->d_qraw, t);
}

// The per-query tables of the static layout, one [V_pad x 16] table per 16 query tokens at `table` (table_stride floats apart), from
// the query tiles at d_qtile and the 16 token ids per tile at d_qids (null: none): the cosine (or the handle's source), the chain,
// sim[id(t_j)][j] = 1, the clip (metric/static.cpp:9-78).  The traceback kernels restate their cells themselves -- or, where the
// table's cell is the canonical cell (a source that is not the cosine, a combinator), read them from these tables: then a query that
// only states listed slices (`only`) needs them too.
// A mixed handle: every operand's table -- a cosine operand's in the canonical arithmetic, operand 0's in place -- from
// the rows vk_corpus_set_query_operand left (vk_validate_query has seen them), then their combination into `table`.
int fill_query_tables(vk_corpus *c, const vk_query_desc *q, const uint8_t *d_qtile, const int32_t *d_qids, float *table, int64_t table_stride,
	bool only, vk_host_keep &keep, hipStream_t st) {
	const bool sourced = c->sim_src.kind != VK_SIMSRC_COSINE, mixed = c->mixed();
	if (only && !sourced && !mixed) return VK_OK;
	const int nq = (q->len_t + 15) / 16, V = c->desc.vocab_size, n_tiles = (int32_t)c->n_tiles;
	int rc;
	if (sourced && (rc = upload_source_query(c, q, keep, st))) return rc;
	for (int m = 1; mixed && m < c->sim_mix.n; m++) {
		const vk_corpus::sim_operand &op = c->operands[m - 1];
		vk_corpus::mix_operand_bufs &b = c->mixop[m - 1];
		const vk_corpus::mix_operand_bufs::rows &rows = b.pending[(size_t)c->q_operand_at];
		if ((rc = b.table.reserve((size_t)nq * (size_t)table_stride, &c->device_bytes))) return rc;
		std::vector<uint8_t> &tile = keep.vec<uint8_t>();
		float mags[VK_MAX_LONG_QUERY_LEN];
		vk_pack_query_rows(op.d, op.tile_bytes, c->prec, rows.bytes.data(), rows.dtype, rows.normalize, q->len_t, tile, mags);
		if ((rc = b.qtile.reserve(tile.size(), &c->device_bytes))) return rc;
		VK_HIP(hipMemcpyAsync(b.qtile, tile.data(), tile.size(), hipMemcpyHostToDevice, st));
		if (op.src.kind != VK_SIMSRC_COSINE && (rc = upload_source_rows(c, op.d, rows.bytes.data(), rows.dtype, q->len_t, b.qraw, keep, st))) return rc;
	}
	for (int t = 0; t < nq; t++) {
		const int cols = std::min(16, q->len_t - t * 16);
		const int32_t *ids = d_qids ? d_qids + t * 16 : nullptr;
		float *tab = table + (size_t)t * table_stride;
		const VkSimSrcArgs sa = source_table_args(c, t);
		if (mixed && !sourced)
			VK_HIP(vk_launch_canon_table(c->d_tiles, d_qtile + (size_t)t * c->tile_bytes, n_tiles, c->nk32, c->tail, c->tile_bytes, c->desc.d, tab, ids, cols, V, c->prec, &c->sim_ops, st));
		else
			VK_HIP(vk_launch_table(c->d_tiles, d_qtile + (size_t)t * c->tile_bytes, n_tiles, c->nk32, c->tail, c->tile_bytes, tab, ids, cols, V, c->prec, &c->sim_ops,
				sourced ? &sa : nullptr, st));
		if (!mixed) continue;
		VkMixArgs mix{};
		mix.in[0] = tab; mix.out = tab; mix.n_cells = table_stride; mix.mix = c->sim_mix;
		for (int m = 1; m < c->sim_mix.n; m++) {
			const vk_corpus::sim_operand &op = c->operands[m - 1];
			vk_corpus::mix_operand_bufs &b = c->mixop[m - 1];
			float *otab = b.table + (size_t)t * table_stride;
			const uint8_t *oq = b.qtile + (size_t)t * op.tile_bytes;
			if (op.src.kind != VK_SIMSRC_COSINE) {
				const VkSimSrcArgs osa = source_table_args_of(op.src, op.raw_rows.get(), op.raw_tile_bytes, op.d, (const float *)b.qraw, t);
				VK_HIP(vk_launch_table(*op.tiles, oq, n_tiles, op.nk32, op.tail, op.tile_bytes, otab, ids, cols, V, c->prec, &op.ops, &osa, st));
			} else
				VK_HIP(vk_launch_canon_table(*op.tiles, oq, n_tiles, op.nk32, op.tail, op.tile_bytes, op.d, otab, ids, cols, V, c->prec, &op.ops, st));
			mix.in[m] = otab;
		}
		VK_HIP(vk_launch_table_mix(&mix, st));
	}
	return VK_OK;
}

// the slice of a row of the slice table as the writer of a result set takes it (vk_host::selected): null where rows are slices
inline const int32_t *slice_of_row(const vk_corpus *c) { return c->entry_sent.empty() ? nullptr : c->entry_sent.data(); }
// row of the slice table of a slice (long slices sit in padded groups); the inverse of entry_sent is built when first needed
int64_t row_of_sentence(vk_corpus *c, int64_t s) {
	if (c->entry_sent.empty()) return s;
	if (c->sent_entry.empty()) {
		c->sent_entry.assign((size_t)c->desc.n_sentences, -1);
		for (int64_t e = 0; e < c->n_entries; e++) if (c->entry_sent[(size_t)e] >= 0) c->sent_entry[(size_t)c->entry_sent[(size_t)e]] = (int32_t)e;
	}
	return (int64_t)c->sent_entry[(size_t)s];
}

// ---- what vk_query.cpp and vk_longq_host.cpp both do around a selection (one copy; each caller keeps its own copies and syncs)
// `ord` (rows of the slice table) longest slice first, rows of one length in the order given: a work list of a one-wave-per-slice pass
inline void rows_longest_first(const vk_corpus *c, std::vector<int32_t> &ord) {
	std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
		return (*c->h_end)[(size_t)a] - (*c->h_start)[(size_t)a] > (*c->h_end)[(size_t)b] - (*c->h_start)[(size_t)b]; });
}
// q->only_slices as keys of rows of the slice table (long slices sit in padded groups: rows != slices) in d_keys[0], in the caller's
// order.  sync: the stream is synchronised before the return; else the caller's next synchronisation covers the copy (the keys live
// in the keep).  *h_keys: the keys on the host.
int upload_listed_keys(vk_corpus *c, const vk_query_desc *q, vk_host_keep &keep, hipStream_t st, bool sync, const uint64_t **h_keys = nullptr) {
	std::vector<uint64_t> &hk = keep.vec<uint64_t>((size_t)q->n_only);
	for (int i = 0; i < q->n_only; i++) hk[(size_t)i] = vk_host::key_of_row(row_of_sentence(c, q->only_slices[i]));
	VK_HIP(hipMemcpyAsync(c->d_keys[0], hk.data(), hk.size() * 8, hipMemcpyHostToDevice, st));
	if (sync) VK_HIP(hipStreamSynchronize(st));
	if (h_keys) *h_keys = hk.data();
	return VK_OK;
}
// The host ends of a selection's copies: `cap` keys and aligner scores and, with tracebacks, cap x stride mappings and edge
// similarities -- taken from the keep once (candidate rounds fetch into the same ones round after round) -- and `sel`, the view of
// them that the writer of a result set takes
struct selected_host {
	std::vector<uint64_t> &keys;
	std::vector<float> &raw, &sim;
	std::vector<int16_t> &map;
	vk_host::selected sel;
	selected_host(vk_host_keep &keep, const vk_corpus *c, int cap, int stride, bool traced)
		: keys(keep.vec<uint64_t>((size_t)cap)), raw(keep.vec<float>((size_t)cap)), sim(keep.vec<float>(traced ? (size_t)cap * stride : 0)),
		  map(keep.vec<int16_t>(traced ? (size_t)cap * stride : 0)) {
		sel.keys = keys.data(); sel.cap = cap; sel.slice_of_row = slice_of_row(c);
		if (traced) { sel.raw = raw.data(); sel.map = map.data(); sel.sim = sim.data(); sel.stride = stride; }
	}
};
// The selected keys at d_keys back on the host and, where tracebacks ran, their outputs at d_raw / d_map / d_sim (rows of h's stride)
// with them; the stream synchronised: h.sel then states the selection
int fetch_selected(const uint64_t *d_keys, const float *d_raw, const int16_t *d_map, const float *d_sim, selected_host &h, hipStream_t st) {
	VK_HIP(hipMemcpyAsync(h.keys.data(), d_keys, h.keys.size() * 8, hipMemcpyDeviceToHost, st));
	if (h.sel.raw) {
		VK_HIP(hipMemcpyAsync(h.raw.data(), d_raw, h.raw.size() * 4, hipMemcpyDeviceToHost, st));
		VK_HIP(hipMemcpyAsync(h.map.data(), d_map, h.map.size() * 2, hipMemcpyDeviceToHost, st));
		VK_HIP(hipMemcpyAsync(h.sim.data(), d_sim, h.sim.size() * 4, hipMemcpyDeviceToHost, st));
	}
	VK_HIP(hipStreamSynchronize(st));
	return VK_OK;
}
// The aligner scores of the first `count` selected rows from the scoring pass's array d_raw into h.raw: more than `singles` of them,
// the whole array in one copy, gathered here; else one float each.  The stream is synchronised.
int gather_raw(vk_corpus *c, const vk_host::selected &sel, int count, int singles, selected_host &h, vk_host_keep &keep, hipStream_t st) {
	const bool whole = count > singles;
	std::vector<float> &all_raw = keep.vec<float>(whole ? (size_t)c->n_entries : 0);
	if (whole) VK_HIP(hipMemcpyAsync(all_raw.data(), c->d_raw, (size_t)c->n_entries * 4, hipMemcpyDeviceToHost, st));
	else for (int i = 0; i < count; i++) VK_HIP(hipMemcpyAsync(&h.raw[(size_t)i], c->d_raw + sel.row(i), 4, hipMemcpyDeviceToHost, st));
	VK_HIP(hipStreamSynchronize(st));
	for (int i = 0; whole && i < count; i++) h.raw[(size_t)i] = all_raw[(size_t)sel.row(i)];
	return VK_OK;
}

// the exact solver over the `count` candidates at w.keys: slices of at most 64 tokens, then (long_too) those of 65 .. 512 tokens
int launch_wrd_exact_both(vk_corpus *c, VkWrdParams &w, int count, float *scores_to_mark, bool long_too, hipStream_t st) {
	VK_HIP(vk_launch_wrd_exact(&w, count, scores_to_mark, st));
	if (long_too) {
		if (w.nq > 1)
			if (int rc = c->d_wrdl_scratch.reserve((size_t)vk_wrd_long_blocks() * vk_wrd_long_scratch_bytes(), &c->device_bytes)) return rc;
		w.scratch = c->d_wrdl_scratch; w.scratch_stride = (int64_t)vk_wrd_long_scratch_bytes();
		VK_HIP(vk_launch_wrd_exact_long(&w, count, st));
	}
	return VK_OK;
}

} // namespace

#endif
