"""-m gpu: batches of one-token queries over a corpus of one-token slices (the span-embedding index) on the span pass of
vk_query_batch (vk_span_batch_kernel), through the C-ABI shim.  The contract of vk_query_batch is "n calls of vk_query":
every result set of a batch is compared with vk_query alone on the same handle -- n, the slices and the bits of the scores, with ==.
The route comes from vk_batch_state (an internal export of the library): 4 is the span pass.

Corpus: 3,001 spans (no multiple of 16, nor of a wave's run of tiles), rows from width_cases (tail-heavy: a lost or doubled tail
feature moves every cosine), rows 100 and 2,900 copies of row 7 (exact ties).  Widths: the edges of width_cases at which a form of
the new kernel or of vk_span_kernel changes."""

import ctypes as C
import inspect
import re

import numpy as np
import pytest

import width_cases as wc

pytestmark = pytest.mark.gpu

N = 3001
BF16 = (5, 200, 289, 304, 305, 384, 753, 769, 1024)
F32 = (5, 289, 304, 305, 1024)
SPAN_ROUTE, ROUTE, N_QTILES, UNIFORM_LEN = 4, 0, 13, 14    # vk_batch_state_index
SPAN = dict(q_normalize=True, gap_s=0.0, gap_t=0.0, want_flow=False)   # HipSpanEncoderIndex's own options

WORLDS = {}   # (precision, d) -> (handle, rows)
for _d in BF16 + F32:
	assert _d in wc.BF16_WIDTHS or _d in wc.F32_WIDTHS, _d


@pytest.fixture(scope="module", autouse=True)
def worlds():
	yield
	for c, _ in WORLDS.values():
		c.close()
	WORLDS.clear()


def rows_of(d, n=N):
	rng = np.random.default_rng(4000 + d)
	G = wc.tail_heavy(wc.with_common_direction(rng.standard_normal((n, d)), rng))
	G[100] = G[2900] = G[7]
	return G


def handle(hip, precision, d, rows=None, off=None):
	rows = rows_of(d) if rows is None else rows
	off = np.arange(len(rows) + 1, dtype=np.int64) if off is None else off
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=len(rows), n_sentences=len(off) - 1, precision=precision)
	c.append_vectors(rows, normalize=True)
	c.set_sentences(off)
	c.finalize()
	return c


def world(hip, precision, d):
	if (precision, d) not in WORLDS:
		rows = rows_of(d)
		WORLDS[(precision, d)] = (handle(hip, precision, d, rows), rows)
	return WORLDS[(precision, d)]


def queries_of(rows, B):
	"""B one-vector queries: of every 40, 17 noisy copies of corpus rows (the tied rows 7 / 100 / 2,900 among them), 20 random ones,
	the same one twice, a zero vector.  The first B of a longer list are the list for B."""
	d = rows.shape[1]
	rng = np.random.default_rng(77 * d + 1)
	out = []
	while len(out) < B:
		at = [7, 100, 2900, 0, N - 1, N - 2] + [int(i) for i in rng.integers(0, N, size=11)]
		out += list(wc.noisy_copy(rows[at], rng))
		out += list(wc.tail_heavy(rng.standard_normal((20, d))))
		out += [out[-1].copy(), out[-1].copy(), np.zeros(d, np.float32)]
	return [np.ascontiguousarray(q[None, :], dtype=np.float32) for q in out[:B]]


def batch_state(hip, c):
	lib = hip.lib()
	lib.vk_batch_state.restype = C.c_int
	lib.vk_batch_state.argtypes = [C.c_void_p, C.c_void_p]
	st = np.zeros(16, dtype=np.int64)
	with c.lock:
		hip._check(lib.vk_batch_state(c._h, st.ctypes.data))
	return st


def run_batch(hip, c, qs, options):
	"""vk_query_batch with a descriptor of its own per query (options: one dict for all, or one per query)"""
	per = options if isinstance(options, (list, tuple)) else [options] * len(qs)
	keep, outs = [], []
	descs = (hip._QueryDesc * len(qs))()
	sos = (hip._TopkOut * len(qs))()
	for i, (q, opt) in enumerate(zip(qs, per)):
		descs[i], len_t = c._desc(q, keep, **opt)
		outs.append(hip.TopK(max(1, descs[i].max_matches), len_t))
		sos[i] = outs[-1]._struct()
	with c.lock:
		hip._check(hip.lib().vk_query_batch(c._h, descs, len(qs), sos))
	for t, so in zip(outs, sos):
		t.n = so.n_out
	return outs


def assert_same(got, ref, what):
	assert got.n == ref.n, (what, got.n, ref.n)
	assert (got.sentence[:got.n] == ref.sentence[:ref.n]).all(), (what, got.sentence[:8], ref.sentence[:8])
	assert (got.score[:got.n].view(np.uint32) == ref.score[:ref.n].view(np.uint32)).all(), (what, got.score[:8], ref.score[:8])
	assert (got.raw_score[:got.n].view(np.uint32) == ref.raw_score[:ref.n].view(np.uint32)).all(), (what, "raw_score")


def assert_batch_is_queries(hip, c, qs, options, route, what, singles=None):
	outs = run_batch(hip, c, qs, options)
	st = batch_state(hip, c)
	if route == SPAN_ROUTE:
		assert st[ROUTE] == SPAN_ROUTE and st[N_QTILES] == (len(qs) + 15) // 16 and st[UNIFORM_LEN] == 1, (what, st)
	else:
		assert st[ROUTE] != SPAN_ROUTE and st[ROUTE] != 0, (what, st)
	per = options if isinstance(options, (list, tuple)) else [options] * len(qs)
	for i, (q, opt) in enumerate(zip(qs, per)):
		ref = singles[i] if singles is not None else c.query(q, **opt)
		assert_same(outs[i], ref, (what, "query", i))
	return outs


@pytest.mark.parametrize("precision,d", [("bf16", d) for d in BF16] + [("f32", d) for d in F32])
def test_every_cell_of_a_batch_is_the_single_querys(hip, precision, d):
	"""max_matches = n, min_score = -1: every span of every query is in the result set, so every cell of the score matrix is compared"""
	c, rows = world(hip, precision, d)
	qs = queries_of(rows, 40)
	outs = assert_batch_is_queries(hip, c, qs, dict(SPAN, max_matches=N, min_score=-1.0), SPAN_ROUTE, (precision, d))
	assert all(t.n == N for t in outs)
	# the planted ties: rows 7, 100 and 2,900 carry one score under every query, and rank by slice index descending
	for t in outs[:3]:
		at = {int(s): j for j, s in enumerate(t.sentence[:t.n])}
		assert t.score[at[7]] == t.score[at[100]] == t.score[at[2900]] and at[2900] < at[100] < at[7]


@pytest.mark.parametrize("min_score", (0.0, 0.3))
@pytest.mark.parametrize("k", (1, 10, 64, 65, 100, 1500))
def test_selection_paths(hip, k, min_score):
	"""k <= 64: the wave selection over the whole matrix; 65 .. 1,024: the block selection row by row; beyond: every key of a row sorted"""
	c, rows = world(hip, "bf16", 304)
	assert_batch_is_queries(hip, c, queries_of(rows, 40), dict(SPAN, max_matches=k, min_score=min_score), SPAN_ROUTE, (k, min_score))


def fill_queries(hip, precision, d):
	lib = hip.lib()
	lib.vk_span_batch_fill_queries.restype = C.c_int32
	lib.vk_span_batch_fill_queries.argtypes = [C.c_int32]
	return lib.vk_span_batch_fill_queries(wc.d_pad(d) * (64 if precision == "f32" else 32))


def test_batch_sizes_and_lds_fills(hip):
	"""around one query tile (15, 16, 17), around four (64, 65), into a third LDS fill of 304-d queries (257), and one query more than
	an LDS fill at 304 and at 1,024 features"""
	for d, sizes in ((304, [2, 15, 16, 17, 64, 65, 257, fill_queries(hip, "bf16", 304) + 1]), (1024, [fill_queries(hip, "bf16", 1024) + 1])):
		assert fill_queries(hip, "bf16", d) >= 16 and fill_queries(hip, "f32", d) >= 16
		c, rows = world(hip, "bf16", d)
		opt = dict(SPAN, max_matches=10, min_score=0.0)
		qs = queries_of(rows, max(sizes))
		singles = [c.query(q, **opt) for q in qs]
		for B in sizes:
			assert_batch_is_queries(hip, c, qs[:B], opt, SPAN_ROUTE, (d, B), singles=singles)


def test_a_batch_over_three_chunks_of_the_matrix(hip, monkeypatch):
	c, rows = world(hip, "bf16", 304)
	monkeypatch.setenv("VK_SPAN_BATCH_CAP", str(16 * 3008 * 4 + 100))   # room for 16 rows of 3,008 floats: 40 queries take 16 + 16 + 8
	for k in (10, 100):
		assert_batch_is_queries(hip, c, queries_of(rows, 40), dict(SPAN, max_matches=k, min_score=0.0), SPAN_ROUTE, ("chunks", k))
	monkeypatch.setenv("VK_SPAN_BATCH_CAP", str(15 * 3008 * 4))   # not even 16 rows: the batch does not qualify (384-d: query by query)
	c, rows = world(hip, "bf16", 384)
	assert_batch_is_queries(hip, c, queries_of(rows, 4), dict(SPAN, max_matches=10, min_score=0.0), 1, "cap below 16 rows")


def test_what_does_not_qualify_answers_as_before(hip, monkeypatch):
	c, rows = world(hip, "bf16", 384)
	qs = queries_of(rows, 6)
	opt = dict(SPAN, max_matches=10, min_score=0.0)
	assert_batch_is_queries(hip, c, qs, opt, SPAN_ROUTE, "the same batch qualifies")
	two = np.ascontiguousarray(np.concatenate((qs[1], qs[2])))
	assert_batch_is_queries(hip, c, [qs[0], two] + qs[2:], opt, 1, "one query of two tokens")
	assert_batch_is_queries(hip, c, qs, [opt] * 5 + [dict(opt, min_score=0.25)], 1, "differing min_score")
	assert_batch_is_queries(hip, c, qs, [opt] * 5 + [dict(opt, max_matches=11)], 1, "differing max_matches")
	assert_batch_is_queries(hip, c, qs, dict(opt, want_flow=True), 1, "want_flow")
	boost = np.linspace(0.5, 1.5, N).astype(np.float32)
	assert_batch_is_queries(hip, c, qs, dict(opt, boost=boost), 1, "a booster")
	assert_batch_is_queries(hip, c, qs, dict(opt, locality=hip.Locality.GLOBAL), 1, "global alignment")
	monkeypatch.setenv("VK_SPAN_BATCH", "off")
	assert_batch_is_queries(hip, c, qs, opt, 1, "VK_SPAN_BATCH=off")
	monkeypatch.delenv("VK_SPAN_BATCH")
	# a corpus with one slice of two tokens
	off = np.concatenate((np.arange(50), np.arange(51, N + 2))).astype(np.int64)
	ragged = handle(hip, "bf16", 384, rows=rows_of(384, N + 1), off=off)
	try:
		assert_batch_is_queries(hip, ragged, qs, opt, 1, "one two-token slice")
	finally:
		ragged.close()


@pytest.mark.parametrize("d", (384, 768))
def test_find_many_is_find_per_text(hip, d):
	"""through the package: HipSpanEncoderIndex.find_many against find, text by text, and against numpy's cosine at the tolerance
	test_span_embedding_index_on_hip holds one query to"""
	import test_gpu_index
	from test_host_api import Document, Session
	from vectorian_amd.sim import EmbeddedSpanSim, SpanEmbedding
	atol = float(re.search(r"atol=([0-9.e-]+)", inspect.getsource(test_gpu_index.test_span_embedding_index_on_hip)).group(1))
	rng = np.random.default_rng(9 + d)
	n = 3000
	vectors = rng.standard_normal((n, d)).astype(np.float32)
	docs = [Document([[f"s{i}"] for i in range(1000)]) for _ in range(3)]
	session = Session(docs, embeddings=[])
	texts = [f"text {i}" for i in range(40)]
	of_text = {t: vectors[int(rng.integers(0, n))] + 0.1 * rng.standard_normal(d).astype(np.float32) for t in texts}
	emb = SpanEmbedding("enc", d, lambda ts: np.stack([of_text[t] for t in ts]))
	index = session.partition("sentence").index(EmbeddedSpanSim(emb), vectors=vectors)
	try:
		done = []
		many = index.find_many(texts, n=5, progress=done.append)
		assert batch_state(hip, index._corpus)[ROUTE] == SPAN_ROUTE and done == [1.0]
		assert len(many) == len(texts)
		key = lambda r: [(docs.index(m.prepared_doc), m.slice_id, m.score) for m in r]
		for t, r in zip(texts, many):
			assert key(r) == key(index.find(t, n=5)), t
			cos = (vectors @ of_text[t]) / (np.linalg.norm(vectors, axis=1) * np.linalg.norm(of_text[t]))
			order = np.argsort(-cos)[:5]
			got = [di * 1000 + sid for di, sid, _ in key(r)]
			# the planted span first; behind it unrelated spans whose cosines lie closer together than the rounding of bf16 rows, so
			# their order is held to the tolerance, not to numpy's: each score is its own span's cosine, and the five are the five largest
			assert got[0] == int(order[0]) and len(set(got)) == 5
			np.testing.assert_allclose([m.score for m in r], cos[got], atol=atol)
			np.testing.assert_allclose([m.score for m in r], cos[order], atol=atol)
	finally:
		index.close()


def test_the_matrix_belongs_to_its_handle(hip):
	rows = rows_of(304)
	c = handle(hip, "bf16", 304, rows)
	qs = queries_of(rows, 40)
	opt = dict(SPAN, max_matches=10, min_score=0.0)
	before = c.device_bytes
	singles = [c.query(q, **opt) for q in qs]
	assert_batch_is_queries(hip, c, qs, opt, SPAN_ROUTE, "first handle", singles=singles)
	grown = c.device_bytes
	assert grown - before >= 48 * 3008 * 4      # the matrix of 40 queries, rounded up to whole query tiles
	v = c.view()
	v_before = v.device_bytes
	assert_batch_is_queries(hip, v, qs, opt, SPAN_ROUTE, "a view", singles=singles)
	assert v.device_bytes - v_before >= 48 * 3008 * 4 and c.device_bytes == grown   # the view grew a matrix of its own
	v.close()
	assert c.device_bytes == grown
	assert_batch_is_queries(hip, c, qs, opt, SPAN_ROUTE, "after the view is closed", singles=singles)
	c.close()
	# a handle closed right after a batch, and a view that outlives its source
	c = handle(hip, "bf16", 304, rows)
	v = c.view()
	run_batch(hip, c, qs, opt)
	c.close()
	assert_batch_is_queries(hip, v, qs[:17], opt, SPAN_ROUTE, "the view of a closed handle")
	v.close()
