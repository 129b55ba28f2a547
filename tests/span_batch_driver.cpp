// Driver of tests/test_span_batch_host.py: the carve-up of the batched span pass (vectorian_amd/csrc/vk_span_batch_host.h) over a table
// of (tile_bytes, spans, queries) -- every query in exactly one chunk of the score matrix and one LDS fill, LDS within the budget, the
// matrix within its cap, 32-bit cell indices only where they hold -- and the qualification's truth table, one flipped condition at a
// time.  `fill <tile_bytes>` prints the queries per LDS fill.
#include "vk_span_batch_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace vk_host;

static long long violations = 0;
static void violated(const char *what, int tile_bytes, long long n, long long B) {
	if (violations++ < 20) printf("VIOLATED %s: tile_bytes %d n %lld B %lld\n", what, tile_bytes, n, B);
}

int main(int argc, char **argv) {
	if (argc > 2 && !strcmp(argv[1], "fill")) {
		printf("%d\n", span_batch_fill_queries(atoi(argv[2])));
		return 0;
	}
	const int bf16_d[] = {5, 200, 289, 304, 305, 384, 753, 769, 1024}, f32_d[] = {5, 289, 304, 305, 1024};
	std::vector<int> tile_bytes;
	for (const int d : bf16_d) tile_bytes.push_back((d + 15) / 16 * 16 * 32);
	for (const int d : f32_d) tile_bytes.push_back((d + 15) / 16 * 16 * 64);
	const long long ns[] = {1, 15, 16, 17, 3001, 100000, 1ll << 20, 1ll << 24, (1ll << 24) + 1, (1ll << 27) - 1, 1ll << 27};
	const long long Bs[] = {2, 15, 16, 17, 40, 128, 129, 256, 257, 1000, 5000};
	long long points = 0;
	for (const int tb : tile_bytes)
		for (const long long n : ns)
			for (const long long B : Bs) {
				points++;
#define CHECK(cond, what) do { if (!(cond)) violated(what, tb, n, B); } while (0)
				// ---- LDS: a 16-query tile fits at every width up to 1,024 features in both precisions; every form within the budget
				const int fill = span_batch_fill_tiles(tb);
				CHECK(fill >= 1 && fill <= kSpanBatchMaxFillTiles, "no query tile fits");
				CHECK(span_batch_lds_bytes(tb, fill) <= kSpanBatchLdsBudget && kSpanBatchLdsBudget * kSpanBatchBlocksPerCu <= kSpanBatchLdsPerCu, "LDS beyond the budget");
				for (const int t : kSpanBatchFillSet)
					if (t > fill) CHECK(span_batch_lds_bytes(tb, t) > kSpanBatchLdsBudget, "a larger fill of the set fits");
				for (int t = 1; t <= fill; t++) {
					const int form = span_batch_form_tiles(t);
					CHECK(form >= t && form <= fill && span_batch_lds_bytes(tb, form) <= kSpanBatchLdsBudget, "form of a launch");
				}
				// ---- the matrix: the largest multiple of 16 rows within the cap; a corpus where 16 rows exceed it does not qualify
				const long long n_pad = span_batch_n_pad(n), chunk = span_batch_chunk(n);
				CHECK(n_pad >= n && n_pad % 16 == 0 && n_pad < n + 16, "row of the matrix");
				span_batch_corpus c;
				c.finalized = c.contextual = c.contiguous = true; c.uniform_len = 1; c.tile_bytes = tb; c.n = n;
				CHECK(chunk % 16 == 0 && chunk >= 0, "chunk");
				CHECK((size_t)(chunk + 16) * (size_t)n_pad * 4 > kSpanBatchMatrixCap, "a larger chunk fits the cap");
				CHECK(span_batch_corpus_ok(c) == (chunk >= 16), "a corpus qualifies iff 16 rows fit the cap");
				if (chunk < 16) continue;
				CHECK(span_batch_matrix_floats(n, chunk) * 4 <= kSpanBatchMatrixCap, "matrix beyond the cap");
				CHECK(span_batch_index_fits_u32(n, chunk), "a cell's index leaves 32 bits");
				CHECK(!span_batch_index_fits_u32((1ll << 31), 4), "the 32-bit rule admits 2^33 cells");
				// ---- every query in exactly one chunk and one fill: the loops of vk_batch.cpp and of the kernel's grid restated
				std::vector<int> seen((size_t)B, 0);
				const long long per = chunk < (B + 15) / 16 * 16 ? chunk : (B + 15) / 16 * 16;
				for (long long base = 0; base < B; base += per) {
					const long long nq = per < B - base ? per : B - base, n_qtiles = (nq + 15) / 16;
					const long long ft = fill < n_qtiles ? fill : n_qtiles, fills = (n_qtiles + ft - 1) / ft;
					CHECK(span_batch_matrix_floats(n, nq) * 4 <= kSpanBatchMatrixCap, "a chunk's matrix beyond the cap");
					for (long long y = 0; y < fills; y++) {
						const long long t1 = (y + 1) * ft < n_qtiles ? (y + 1) * ft : n_qtiles;
						CHECK(span_batch_lds_bytes(tb, span_batch_form_tiles((int)ft)) <= kSpanBatchLdsBudget, "a fill beyond the budget");
						for (long long row = y * ft * 16; row < t1 * 16 && row < nq; row++) seen[(size_t)(base + row)]++;
					}
				}
				for (long long i = 0; i < B; i++) CHECK(seen[(size_t)i] == 1, "a query in no fill, or in two");
				for (const int cus : {1, 256, 304}) {
					const int g = span_batch_grid(n, cus);
					CHECK(g >= 1 && g <= cus * kSpanBatchBlocksPerCu, "grid");
				}
#undef CHECK
			}
	// ---- the truth table: the batch that qualifies, then one condition flipped at a time
	long long table = 0;
#define EXPECT(cond, what) do { table++; if (!(cond)) { violations++; printf("VIOLATED truth table: %s\n", what); } } while (0)
	span_batch_corpus c;
	c.finalized = c.contextual = c.contiguous = true; c.uniform_len = 1; c.tile_bytes = 304 * 32; c.n = 3001;
	EXPECT(span_batch_corpus_ok(c), "the corpus that qualifies");
	{ span_batch_corpus x = c; x.finalized = false; EXPECT(!span_batch_corpus_ok(x), "not finalized"); }
	{ span_batch_corpus x = c; x.contextual = false; EXPECT(!span_batch_corpus_ok(x), "static layout"); }
	{ span_batch_corpus x = c; x.contiguous = false; EXPECT(!span_batch_corpus_ok(x), "not contiguous"); }
	{ span_batch_corpus x = c; x.uniform_len = 0; EXPECT(!span_batch_corpus_ok(x), "ragged"); }
	{ span_batch_corpus x = c; x.uniform_len = 2; EXPECT(!span_batch_corpus_ok(x), "two-token slices"); }
	{ span_batch_corpus x = c; x.n_long_groups = 1; EXPECT(!span_batch_corpus_ok(x), "long groups"); }
	{ span_batch_corpus x = c; x.has_entry_sent = true; EXPECT(!span_batch_corpus_ok(x), "entry_sent"); }
	{ span_batch_corpus x = c; x.sourced = true; EXPECT(!span_batch_corpus_ok(x), "a source that is not the cosine"); }
	{ span_batch_corpus x = c; x.chained = true; EXPECT(!span_batch_corpus_ok(x), "an operator chain"); }
	{ span_batch_corpus x = c; x.n = 0; EXPECT(!span_batch_corpus_ok(x), "no spans"); }
	{ span_batch_corpus x = c; x.tile_bytes = (int)kSpanBatchLdsBudget + 512; EXPECT(!span_batch_corpus_ok(x), "a query tile beyond the LDS"); }
	{ span_batch_corpus x = c; EXPECT(!span_batch_corpus_ok(x, 15 * 3008 * 4) && span_batch_corpus_ok(x, 16 * 3008 * 4), "16 rows against the cap"); }
	span_batch_query q;
	q.len_t = 1; q.align = q.local = true; q.max_matches = 10; q.min_score = 0.25f;
	EXPECT(span_batch_query_ok(q, q), "the query that qualifies");
	{ span_batch_query x = q; x.len_t = 2; EXPECT(!span_batch_query_ok(x, q), "two tokens"); }
	{ span_batch_query x = q; x.align = false; EXPECT(!span_batch_query_ok(x, q), "no alignment"); }
	{ span_batch_query x = q; x.local = false; EXPECT(!span_batch_query_ok(x, q), "not local"); }
	{ span_batch_query x = q; x.tagged = true; EXPECT(!span_batch_query_ok(x, q), "tag weights"); }
	{ span_batch_query x = q; x.submatch = true; EXPECT(!span_batch_query_ok(x, q), "submatch weight"); }
	{ span_batch_query x = q; x.boost = true; EXPECT(!span_batch_query_ok(x, q), "booster"); }
	{ span_batch_query x = q; x.want_flow = true; EXPECT(!span_batch_query_ok(x, q), "want_flow"); }
	{ span_batch_query x = q; x.only = true; EXPECT(!span_batch_query_ok(x, q), "only_slices"); }
	{ span_batch_query x = q; x.max_matches = 11; EXPECT(!span_batch_query_ok(x, q), "another max_matches"); }
	{ span_batch_query x = q; x.min_score = 0.5f; EXPECT(!span_batch_query_ok(x, q), "another min_score"); }
	{ span_batch_query x = q; x.min_score = -0.25f; EXPECT(!span_batch_query_ok(x, q), "min_score of the other sign"); }
#undef EXPECT
	printf("points %lld table %lld violations %lld\n", points, table, violations);
	return violations ? 1 : 0;
}
