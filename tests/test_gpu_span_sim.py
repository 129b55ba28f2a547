"""-m gpu: the span index under a VectorSim that is not the bare cosine (vk_corpus_set_span_sim), through the C-ABI shim and
through HipSpanEncoderIndex.

Expected values: vector_sim_cases.source_matrix(spans, q[None], source)[:, 0] (the numpy restatement of vk_sim_src_host.h), then
sim_ops_cases.apply_numpy(ops, .) (vectorian_amd/kernel.py in float32), then admission score > max(min_score, 0), then the order of a
result set: keys (orderable(score) << 32) | row, descending.  Scores are compared as view(uint32) with == for p = 1, p = 2 and the
sqrt-cosine under exactly rounded operators (Bias, Scale, Threshold, DistanceToSimilarity).  Under powf / expf (p = 3, p = 0.5,
Power, RadialBasis) DESIGN 12's rule applies: 2e-5 relative, the returned ids checked as a set wherever two expected scores are
closer than that.  Every test asserts that its result set is not empty: n == min(k, #expected above the floor) > 0.

Corpus rows: width_cases' tail-heavy rows of three magnitudes, as test_gpu_span_batch.py builds them; among them a zero row (5), a
row equal to the query (3: distance exactly 0), a row of NaN (9) and three identical rows (7, 100, 2,900: exact ties, ordered by
row)."""

import ctypes as C

import numpy as np
import pytest

import pool_cases as pc
import sim_ops_cases as sc
import vector_sim_cases as vc
import width_cases as wc
from vectorian_amd.kernel import Bias, DistanceToSimilarity, Power, RadialBasis, Scale, Threshold
from vectorian_amd.sim import (AggregatedSpanEmbedding, CosineSim, EmbeddedSpanSim, ImprovedSqrtCosineSim, ModifiedVectorSim, PNormDistance,
	SpanEmbedding)

pytestmark = pytest.mark.gpu

WIDTHS = (2, 5, 15, 16, 17, 31, 33, 64, 67, 300, 768, 1024)
COUNTS = (1, 16, 17, 3001)
N = 3001
TOL = 2e-5
PNORM, SQRT_COS = 1, 2   # core.VK_SIMSRC_*
SOURCES = {"p1": (PNORM, np.float32(1)), "p2": (PNORM, np.float32(2)), "p3": (PNORM, np.float32(3)), "p0.5": (PNORM, np.float32(0.5)),
	"sqrt-cos": (SQRT_COS, np.float32(0))}
EXACT_SOURCES = ("p1", "p2", "sqrt-cos")
SPAN = dict(q_normalize=True, gap_s=0.0, gap_t=0.0, want_flow=False)   # HipSpanEncoderIndex's own options
ZERO, EQUAL, NAN, TIES = 5, 3, 9, (7, 100, 2900)


def rows_of(d, n=N, seed=0, magnitudes=True):
	"""(rows, query): the query is row EQUAL's copy where the corpus has such a row, else a noisy copy of row 0"""
	rng = np.random.default_rng(9000 + 31 * d + seed)
	G = wc.tail_heavy(wc.with_common_direction(rng.standard_normal((max(n, 4), d)), rng))
	if magnitudes:
		G = G * rng.choice([1e-3, 1.0, 1e3], size=(max(n, 4), 1))
	G = np.ascontiguousarray(G[:n], dtype=np.float32)
	q = wc.noisy_copy(G[:1], rng)[0] if n <= EQUAL else G[EQUAL].copy()
	if n > ZERO:
		G[ZERO] = 0
	if n > NAN:
		G[NAN] = np.nan
	if n > TIES[-1]:
		G[TIES[1]] = G[TIES[2]] = G[TIES[0]]
	return G, np.ascontiguousarray(q, dtype=np.float32)


def handle(hip, rows, source=None, ops=(), precision="bf16", chunks=None, span_sim=True):
	"""a span corpus: one row per slice.  chunks: rows per append call (the rest in a last call)"""
	n, d = rows.shape
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=n, n_sentences=n, precision=precision)
	if span_sim:
		c.set_span_sim(source, sc.pairs(ops))
	at = 0
	for m in list(chunks or ()) + [n]:
		m = min(m, n - at)
		if m > 0:
			c.append_vectors(rows[at:at + m], normalize=True)
		at += m
	c.set_sentences(np.arange(n + 1, dtype=np.int64))
	c.finalize()
	return c


def orderable(scores):
	b = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
	return np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xffffffff), b | np.uint64(0x80000000))


def values_of(rows, q, source, ops):
	"""the score of every span, float32 [n]"""
	with np.errstate(all="ignore"):
		v = vc.source_matrix(rows, q[None, :], source)[:, 0]
		return sc.apply_numpy(ops, v) if len(ops) else v


def expected_set(values, k, min_score):
	floor = np.float32(max(min_score, 0.0))
	with np.errstate(invalid="ignore"):
		rows = np.nonzero(values > floor)[0]
	keys = (orderable(values[rows]) << np.uint64(32)) | rows.astype(np.uint64)
	order = np.argsort(keys)[::-1][:k]
	return rows[order], values[rows[order]]


def assert_exact(top, values, k, min_score, what):
	ids, scores = expected_set(values, k, min_score)
	assert len(ids) > 0, (what, "an empty expectation proves nothing")
	assert top.n == len(ids), (what, top.n, len(ids))
	assert (top.sentence[:top.n] == ids).all(), (what, top.sentence[:8], ids[:8])
	assert (top.score[:top.n].view(np.uint32) == scores.view(np.uint32)).all(), (what, top.score[:8], scores[:8])
	assert (top.raw_score[:top.n].view(np.uint32) == scores.view(np.uint32)).all(), (what, "raw_score")


def assert_close(top, values, k, min_score, what):
	"""under powf / expf: every returned score within TOL of its span's expected value, descending; as many results as the floor
	admits to within TOL; every span whose expected value beats the last returned one by more than TOL is returned"""
	floor = max(min_score, 0.0)
	with np.errstate(invalid="ignore"):
		n_lo, n_hi = int((values > floor * (1 + TOL) + 1e-30).sum()), int((values > floor * (1 - TOL)).sum())
	assert n_lo > 0, (what, "an empty expectation proves nothing")
	assert min(k, n_lo) <= top.n <= min(k, n_hi), (what, top.n, n_lo, n_hi)
	ids, got = top.sentence[:top.n], top.score[:top.n]
	assert len(set(ids.tolist())) == top.n and np.isfinite(values[ids]).all(), what
	assert (np.abs(got - values[ids]) <= TOL * np.abs(values[ids])).all(), (what, got[:8], values[ids][:8])
	assert (got[:-1] >= got[1:]).all() and (got > floor).all(), what
	if top.n == k:
		with np.errstate(invalid="ignore"):
			must = set(np.nonzero(values > got[-1] * (1 + 2 * TOL))[0].tolist())
		assert must <= set(ids.tolist()), (what, sorted(must - set(ids.tolist()))[:8])
	assert (top.raw_score[:top.n].view(np.uint32) == got.view(np.uint32)).all(), (what, "raw_score")


def check(top, values, k, min_score, exact, what):
	(assert_exact if exact else assert_close)(top, values, k, min_score, what)


def is_exact(source_name, ops):
	return source_name in EXACT_SOURCES and all(type(op) in (Bias, Scale, Threshold, DistanceToSimilarity) for op in ops)


@pytest.mark.parametrize("d", WIDTHS)
def test_every_form_at_every_width_and_span_count(hip, d):
	"""1, 16, 17 and 3,001 spans; the handle keeps its copy of the rows and changes among the sources, as DESIGN 13's static handles do"""
	for n in COUNTS:
		rows, q = rows_of(d, n)
		c = handle(hip, rows, SOURCES["p2"])
		try:
			for name, source in SOURCES.items():
				c.set_span_sim(source, [])
				values = values_of(rows, q, source, [])
				for k, floor in ((10, 0.0), (N, 0.0)):
					check(c.query(q[None, :], max_matches=k, min_score=floor, **SPAN), values, k, floor, name in EXACT_SOURCES, (d, n, name, k))
				if n == N:
					# a bare distance ranks the farthest span first; the row equal to the query (distance exactly 0), the NaN row and,
					# under the sqrt-cosine, the zero row (0 by nan_to_num) are no matches; the tied rows come back in the order of a result set
					top = c.query(q[None, :], max_matches=N, min_score=0.0, **SPAN)
					got = top.sentence[:top.n].tolist()
					assert NAN not in got and (EQUAL not in got) == (source[0] == PNORM) and (ZERO in got) == (source[0] == PNORM), (d, name)
					at = {s: j for j, s in enumerate(got)}
					assert (TIES[0] in at) == bool(values[TIES[0]] > 0) and (source[0] != PNORM or TIES[0] in at), (d, name)
					if TIES[0] in at:
						assert top.score[at[7]] == top.score[at[100]] == top.score[at[2900]] and at[2900] < at[100] < at[7], (d, name)
		finally:
			c.close()


@pytest.mark.parametrize("chain", ("i", "ii", "iii", "iv", "v", "vi"))
def test_the_six_chains_every_k_and_two_floors(hip, chain):
	"""scales and widths from the median value (vector_sim_cases.chain with E = the span vectors); k across the forms of the
	selection (64, 1,024); floors 0 and the median expected score"""
	d = 67
	rows, q = rows_of(d, N, seed=1)
	finite = np.ascontiguousarray(np.delete(rows, NAN, axis=0))
	sim, ops = vc.chain(chain, finite, q[None, :])
	source = vc.source_of(sim)
	name = next(k for k, v in SOURCES.items() if v[0] == source[0] and float(v[1]) == float(source[1]))
	values = values_of(rows, q, source, ops)
	if ops and type(ops[-1]) in (DistanceToSimilarity, RadialBasis):
		assert float(((values > 0) & (values < 1)).mean()) >= 1 / 3, chain
	c = handle(hip, rows, source, ops)
	try:
		median = float(np.median(values[np.isfinite(values) & (values > 0)]))
		for floor in (0.0, median):
			for k in (1, 10, 64, 65, 1024, 1500):
				check(c.query(q[None, :], max_matches=k, min_score=floor, **SPAN), values, k, floor, is_exact(name, ops), (chain, k, floor))
		# a negative min_score admits nothing more: negative values and NaN are never matches
		check(c.query(q[None, :], max_matches=N, min_score=-1.0, **SPAN), values, N, 0.0, is_exact(name, ops), (chain, "min_score -1"))
	finally:
		c.close()


def test_power_and_radial_basis_on_exact_sources(hip):
	rows, q = rows_of(300, N, seed=2)
	m = float(np.nanmedian(values_of(rows, q, SOURCES["p2"], [])))
	for name, ops in (("p2", [Scale(1 / (2 * m)), DistanceToSimilarity(), Power(2.5)]), ("p1", [Scale(1 / (40 * m)), RadialBasis(1.5)]),
			("sqrt-cos", [Bias(0.1), Power(0.5)])):
		values = values_of(rows, q, SOURCES[name], ops)
		c = handle(hip, rows, SOURCES[name], ops)
		try:
			for k in (10, 1500):
				check(c.query(q[None, :], max_matches=k, min_score=0.0, **SPAN), values, k, 0.0, False, (name, k))
		finally:
			c.close()


def test_one_tile_more_than_a_sweep_of_the_grid(hip):
	"""d = 5: the count at which the grid-stride wraps, from the header's grid (an internal export) on this device"""
	lib = hip.lib()
	lib.vk_span_sim_launch_grid.restype = C.c_int32
	lib.vk_span_sim_launch_grid.argtypes = [C.c_int64]
	grid = lib.vk_span_sim_launch_grid(1 << 30)
	assert grid >= 3 and lib.vk_span_sim_launch_grid(1) == 1
	sweep = grid * 4 * 4   # tiles: four waves per workgroup, runs of four tiles
	n = (sweep + 1) * 16 - 3
	assert lib.vk_span_sim_launch_grid(n) == grid
	rng = np.random.default_rng(55)
	rows = (rng.standard_normal((n, 5)) * rng.choice([1e-3, 1.0, 1e3], size=(n, 1))).astype(np.float32)
	q = rows[n - 2].copy()
	c = handle(hip, rows, SOURCES["p1"])
	try:
		for name in EXACT_SOURCES:
			c.set_span_sim(SOURCES[name], [])
			values = values_of(rows, q, SOURCES[name], [])
			assert_exact(c.query(q[None, :], max_matches=1500, min_score=0.0, **SPAN), values, 1500, 0.0, name)
			# every span's score: the tiles of the wrapped run and the partly filled last tile among them
			c.query(q[None, :], max_matches=1, min_score=0.0, **SPAN)
			assert (c.last_scores().view(np.uint32) == values.view(np.uint32)).all(), name
	finally:
		c.close()


def test_rows_appended_in_three_calls_and_as_bf16(hip):
	"""5, 16 and the rest: the raw copy's offsets are no multiples of 16; bf16 rows are widened exactly"""
	for d in (33, 300):
		rows, q = rows_of(d, N, seed=3)
		bits = (rows.view(np.uint32) >> 16).astype(np.uint16)
		wide = pc.widen(bits)
		for given, unmodified in ((rows, rows), (bits, wide)):
			c = handle(hip, given, SOURCES["p2"], chunks=(5, 16))
			try:
				for name in EXACT_SOURCES:
					c.set_span_sim(SOURCES[name], [Scale(0.5)])
					values = values_of(unmodified, q, SOURCES[name], [Scale(0.5)])
					assert_exact(c.query(q[None, :], max_matches=N, min_score=0.0, **SPAN), values, N, 0.0, (d, given.dtype, name))
				# ... and a bf16 query
				qb = (q.view(np.uint32) >> 16).astype(np.uint16)
				values = values_of(unmodified, pc.widen(qb), SOURCES["sqrt-cos"], [Scale(0.5)])
				assert_exact(c.query(qb[None, :], max_matches=N, min_score=0.0, **SPAN), values, N, 0.0, (d, given.dtype, "bf16 query"))
			finally:
				c.close()


@pytest.mark.parametrize("precision,d", [("bf16", 300), ("bf16", 305), ("bf16", 768), ("f32", 300)])
def test_the_cosine_under_a_chain_is_the_plain_handles_unclipped_sum(hip, precision, d):
	"""the same vectors on a plain handle, queried with q and with -q.  A plain clipped score for q strictly inside (0, 1) IS the
	unclipped sum u: the chained handle returns apply_numpy(ops, u) bit for bit.  For the spans of negative cosine u is taken as minus
	the plain score for -q.  On the fp32 matrix pipe negating the query negates every partial sum exactly and those are held bit for
	bit too; the bf16 pipe (v_mfma_f32_16x16x32_bf16) does NOT round symmetrically -- measured on an MI355X: of 3,001 spans the
	unclipped sums for q and -q differ in 238 .. 976, by at most 1.3e-6 relative -- so negative cosines under bf16 are held within
	1e-5, the tolerance of tests/test_gpu_f32_precision.py.  Every span's score is read (vk_last_scores), and the result sets are
	held against those scores with ==."""
	rng = np.random.default_rng(70 + d)
	rows = np.ascontiguousarray(wc.tail_heavy(wc.with_common_direction(rng.standard_normal((N, d)), rng)), dtype=np.float32)
	rows[100] = rows[2900] = rows[7]
	q = np.ascontiguousarray(wc.noisy_copy(rows[7:8], rng), dtype=np.float32)   # (rows 7, 100 and 2,900 tie at the top)
	plain = handle(hip, rows, precision=precision, span_sim=False)
	try:
		u = np.full(N, np.nan, np.float32)
		positive = np.zeros(N, bool)
		for sign in (1.0, -1.0):
			top = plain.query(np.float32(sign) * q, max_matches=N, min_score=-1.0, **SPAN)
			assert top.n == N
			s, ids = top.score[:N], top.sentence[:N]
			inside = (s > 0) & (s < 1)
			u[ids[inside]] = np.float32(sign) * s[inside]
			if sign > 0:
				positive[ids[inside]] = True
	finally:
		plain.close()
	known = np.isfinite(u)
	assert known.all(), int((~known).sum())
	assert (u < 0).mean() >= 1 / 3 and (u > 0).mean() >= 1 / 3
	exact = positive if precision == "bf16" else known

	def held(c, ops, k, floor, what):
		want = sc.apply_numpy(ops, u)
		top = c.query(q, max_matches=k, min_score=floor, **SPAN)
		got = c.last_scores()
		assert (got[exact].view(np.uint32) == want[exact].view(np.uint32)).all(), (what, int((got[exact].view(np.uint32) != want[exact].view(np.uint32)).sum()))
		assert (np.abs(got[~exact] - want[~exact]) <= 1e-5).all(), (what, float(np.abs(got[~exact] - want[~exact]).max(initial=0)))
		assert_exact(top, got, k, floor, what)        # the result set: the kernel's own floats, admitted and ordered
		return top

	for ops in ([Bias(1), Scale(0.5)], [Threshold(0.3)]):
		c = handle(hip, rows, None, ops, precision=precision)
		try:
			top = held(c, ops, N, 0.0, (precision, d, type(ops[0]).__name__))
			assert top.n == (N if len(ops) == 2 else int((u > np.float32(0.3)).sum()))
			held(c, ops, 10, 0.4, (precision, d, "k 10"))
			# the chain may change at any time, before or after finalize: no copy is needed
			c.set_span_sim(None, sc.pairs([Scale(-1.0)]))
			assert held(c, [Scale(-1.0)], N, 0.0, (precision, d, "negated")).n == int((~positive).sum())
		finally:
			c.close()


def test_the_cosine_handle_is_untouched(hip):
	"""a span handle that never calls set_span_sim and one that sets (cosine, no operators): today's scores, nothing allocated"""
	rows, q = rows_of(300, N, seed=4)
	rows = np.nan_to_num(rows)
	never = handle(hip, rows, span_sim=False)
	bare = handle(hip, rows, None, [])
	try:
		assert never.device_bytes == bare.device_bytes
		for k, floor in ((10, 0.0), (1500, 0.2), (N, -1.0)):
			a, b = never.query(q[None, :], max_matches=k, min_score=floor, **SPAN), bare.query(q[None, :], max_matches=k, min_score=floor, **SPAN)
			assert a.n == b.n > 0 and (a.sentence[:a.n] == b.sentence[:b.n]).all()
			assert (a.score[:a.n].view(np.uint32) == b.score[:b.n].view(np.uint32)).all()
			assert ((a.score[:a.n] >= 0) & (a.score[:a.n] <= 1)).all()
		# back from a chain to the bare cosine: the clipped scores again
		bare.set_span_sim(None, sc.pairs([Bias(1)]))
		assert bare.query(q[None, :], max_matches=N, min_score=0.0, **SPAN).score[:10].max() > 1
		bare.set_span_sim(None, [])
		a, b = never.query(q[None, :], max_matches=N, min_score=0.0, **SPAN), bare.query(q[None, :], max_matches=N, min_score=0.0, **SPAN)
		assert a.n == b.n > 0 and (a.score[:a.n].view(np.uint32) == b.score[:b.n].view(np.uint32)).all() and (a.sentence[:a.n] == b.sentence[:b.n]).all()
	finally:
		never.close()
		bare.close()


def test_pooled_spans_at_the_corpus_level_keep_their_nan_rows(hip):
	"""vk_corpus_append_pooled fills the copy from its fp32 aggregates: an empty span's row of NaN stays NaN and is never returned"""
	d = 65
	case = pc.rows_case(d)
	start, end = case["start"], case["end"]
	n = len(start)
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=n, n_sentences=n)
	try:
		c.set_span_sim(SOURCES["p2"], [])
		pooled = c.append_pooled(case["rows"], start, end, np.mean, normalize=True, want_pooled=True)
		c.set_sentences(np.arange(n + 1, dtype=np.int64))
		c.finalize()
		empty = np.nonzero(end == start)[0]
		assert len(empty) == 1 and np.isnan(pooled[empty[0]]).all()
		q = np.ascontiguousarray(pooled[int(np.nonzero(np.isfinite(pooled).all(axis=1))[0][0])] + np.float32(0.25))
		for name in EXACT_SOURCES:
			c.set_span_sim(SOURCES[name], [])
			values = values_of(pooled, q, SOURCES[name], [])
			top = c.query(q[None, :], max_matches=n, min_score=0.0, **SPAN)
			assert_exact(top, values, n, 0.0, name)
			assert empty[0] not in top.sentence[:top.n].tolist()
	finally:
		c.close()


@pytest.mark.parametrize("embedding", ["static", "contextual"])
def test_a_pooled_index_is_the_index_over_the_numpy_aggregates(hip, embedding):
	session, embeddings, texts = pc.toy_session()
	part = session.partition("sentence", 3, 2)
	emb = AggregatedSpanEmbedding(embeddings[embedding], np.mean)
	vectors = pc.reference_span_vectors(session, part, emb)
	qv = emb.encode(texts[:1])
	s = 1 / (2 * float(np.nanmedian(values_of(vectors, qv[0], SOURCES["p2"], []))))
	sim = ModifiedVectorSim(PNormDistance(2), Scale(s), DistanceToSimilarity())
	key = lambda result: [(session.documents.index(m.prepared_doc), m.slice_id, np.float32(m.score).view(np.uint32)) for m in result]
	pooled = part.index(emb.to_sentence_sim(sim))
	given = part.index(emb.to_sentence_sim(sim), vectors=vectors)
	try:
		values = values_of(vectors, qv[0], SOURCES["p2"], [Scale(s), DistanceToSimilarity()])
		assert float(((values > 0) & (values < 1)).mean()) >= 1 / 3
		for text in texts:
			a, b = pooled.find(text, n=8), given.find(text, n=8)
			assert len(a) >= 1 and key(a) == key(b), text
		ids, scores = expected_set(values, 8, 0.0)
		first = pooled.find(texts[0], n=8)
		assert len(first) == 8 and [np.float32(m.score).view(np.uint32) for m in first] == scores.view(np.uint32).tolist()
		# find_many is find, bit for bit
		many = pooled.find_many(texts, n=8)
		assert [key(r) for r in many] == [key(pooled.find(t, n=8)) for t in texts]
	finally:
		pooled.close()
		given.close()


def batch_state(hip, c):
	lib = hip.lib()
	lib.vk_batch_state.restype = C.c_int
	lib.vk_batch_state.argtypes = [C.c_void_p, C.c_void_p]
	st = np.zeros(16, dtype=np.int64)
	with c.lock:
		hip._check(lib.vk_batch_state(c._h, st.ctypes.data))
	return st


def test_batches_views_and_lifetime(hip):
	d = 300
	rows, q = rows_of(d, N, seed=5, magnitudes=False)   # (one scale: every query of the batch has spans within the chain's reach)
	rng = np.random.default_rng(8)
	qs = [np.ascontiguousarray(x[None, :]) for x in wc.noisy_copy(rows[rng.integers(10, N, size=257)], rng)]
	ops = [Scale(1 / (2 * float(np.nanmedian(values_of(rows, q, SOURCES["p2"], []))))), DistanceToSimilarity()]
	plain = handle(hip, rows, span_sim=False)
	chained = handle(hip, rows, None, [Bias(1), Scale(0.5)])
	c = handle(hip, rows, SOURCES["p2"], ops)
	view = None
	try:
		# device_bytes: at least the copy for a source (ceil(d / 16) KiB per 16 spans), nothing for a chain on the cosine
		assert chained.device_bytes == plain.device_bytes
		assert c.device_bytes - plain.device_bytes >= (N + 15) // 16 * ((d + 15) // 16) * 1024
		for handle_, label in ((c, "source"), (chained, "cosine chain")):
			singles = [handle_.query(x, max_matches=10, min_score=0.0, **SPAN) for x in qs]
			assert all(t.n == 10 for t in singles)
			for B in (2, 16, 257):
				outs = handle_.query_batch(qs[:B], max_matches=10, min_score=0.0, **SPAN)
				st = batch_state(hip, handle_)
				assert st[0] == 1, (label, B, st)   # query by query: not the span pass (4), not the shared pass (2)
				for i, (a, b) in enumerate(zip(outs, singles)):
					assert a.n == b.n and (a.sentence[:a.n] == b.sentence[:b.n]).all(), (label, B, i)
					assert (a.score[:a.n].view(np.uint32) == b.score[:b.n].view(np.uint32)).all(), (label, B, i)
		# a view answers as its owner, also after the owner is gone
		values = values_of(rows, q, SOURCES["p2"], ops)
		view = c.view()
		assert_exact(view.query(q[None, :], max_matches=100, min_score=0.0, **SPAN), values, 100, 0.0, "view")
		c.close()
		assert_exact(view.query(q[None, :], max_matches=100, min_score=0.3, **SPAN), values, 100, 0.3, "view, owner closed")
		# ... and may change among sources and chains: it shares the copy
		view.set_span_sim(SOURCES["p1"], [])
		assert_exact(view.query(q[None, :], max_matches=100, min_score=0.0, **SPAN), values_of(rows, q, SOURCES["p1"], []), 100, 0.0, "view, p = 1")
	finally:
		for h in (plain, chained, c, view):
			if h is not None:
				h.close()


def test_find_many_is_find(hip):
	from test_host_api import Document, Session
	rng = np.random.default_rng(21)
	n, d = 90, 24
	vectors = rng.standard_normal((n, d)).astype(np.float32)
	docs = [Document([[f"s{i}"] for i in range(30)]) for _ in range(3)]
	session = Session(docs, embeddings=[])
	texts = [f"text {i}" for i in range(40)]
	target = {t: vectors[int(rng.integers(0, n))] + 0.05 * rng.standard_normal(d).astype(np.float32) for t in texts}
	emb = SpanEmbedding("enc", d, lambda ts: np.stack([target[t] for t in ts]))
	for sim in (ModifiedVectorSim(PNormDistance(2), RadialBasis(0.02)), ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5)), ImprovedSqrtCosineSim()):
		index = session.partition("sentence").index(EmbeddedSpanSim(emb, sim), vectors=vectors)
		try:
			key = lambda r: [(docs.index(m.prepared_doc), m.slice_id, np.float32(m.score).view(np.uint32)) for m in r]
			many = index.find_many(texts, n=5, min_score=0.05)
			assert all(len(r) >= 1 for r in many)
			assert [key(r) for r in many] == [key(index.find(t, n=5, min_score=0.05)) for t in texts]
		finally:
			index.close()


def refused(hip, status, words, call):
	with pytest.raises(hip.VkError) as e:
		call()
	assert e.value.status == status and all(w in str(e.value) for w in words), (status, words, str(e.value))


def test_refusals_leave_the_handle_as_it_was(hip):
	d = 33
	rows, q = rows_of(d, 40, seed=6)
	values = values_of(rows, q, SOURCES["p2"], [])
	# set after the first append; on a finalized handle without the copy; on a view; a fresh append succeeds afterwards
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=40, n_sentences=40)
	c.append_vectors(rows[:8], normalize=True)
	refused(hip, hip.VK_ERR_STATE, ("before the first append",), lambda: c.set_span_sim(SOURCES["p2"], []))
	c.append_vectors(rows[8:], normalize=True)
	c.set_sentences(np.arange(41, dtype=np.int64))
	c.finalize()
	refused(hip, hip.VK_ERR_STATE, ("before the first append",), lambda: c.set_span_sim(SOURCES["sqrt-cos"], []))
	v = c.view()
	refused(hip, hip.VK_ERR_STATE, ("before the first append",), lambda: v.set_span_sim(SOURCES["p1"], []))
	assert c.query(q[None, :], max_matches=5, min_score=-1.0, **SPAN).n == 5 and v.query(q[None, :], max_matches=5, min_score=-1.0, **SPAN).n == 5
	v.close()
	c.close()
	# d = 1,025
	wide = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=1025, n_tokens=4, n_sentences=4)
	refused(hip, hip.VK_ERR_UNSUPPORTED, ("1024",), lambda: wide.set_span_sim(SOURCES["p2"], []))
	wide.set_span_sim(None, sc.pairs([Bias(1)]))   # a chain on the cosine needs no copy
	wide.close()
	# a span-sim call on a static handle
	static = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=d, n_tokens=8, n_sentences=2, vocab_size=4)
	refused(hip, hip.VK_ERR_UNSUPPORTED, ("VK_LAYOUT_STATIC",), lambda: static.set_span_sim(SOURCES["p2"], []))
	refused(hip, hip.VK_ERR_UNSUPPORTED, ("VK_LAYOUT_STATIC",), lambda: static.set_span_sim(None, sc.pairs([Bias(1)])))
	static.close()
	# ... and the static entry points keep refusing contextual handles
	c = handle(hip, rows, SOURCES["p2"])
	try:
		refused(hip, hip.VK_ERR_UNSUPPORTED, ("CONTEXTUAL",), lambda: c.set_sim_source(*SOURCES["p2"]))
		refused(hip, hip.VK_ERR_UNSUPPORTED, ("CONTEXTUAL",), lambda: c.set_sim_ops(sc.pairs([Bias(1)])))
		# bad kind, p, operator; nine operators
		for source, ops in (((7, 0.0), []), ((PNORM, 0.0), []), ((PNORM, float("inf")), []), ((PNORM, float("nan")), []), ((PNORM, -1.0), []),
				(SOURCES["p1"], [(9, 1.0)]), (SOURCES["p1"], [(-1, 1.0)]), (SOURCES["p1"], [(0, float("nan"))]), (None, [(0, 0.1)] * 9)):
			refused(hip, hip.VK_ERR_INVALID, (), lambda: c.set_span_sim(source, ops))
		ok = dict(SPAN, max_matches=5, min_score=0.0)
		assert_exact(c.query(q[None, :], **ok), values, 5, 0.0, "after the refused settings")
		# queries that are not span-shaped, each named
		two = np.ascontiguousarray(np.stack([q, q]))
		for words, call in (
				(("more than one token",), lambda: c.query(two, **ok)),
				(("want_flow",), lambda: c.query(q[None, :], **dict(ok, want_flow=True))),
				(("booster",), lambda: c.query(q[None, :], boost=np.ones(40, np.float32), **ok)),
				(("only_slices",), lambda: c.query(q[None, :], only_slices=[1, 2], **dict(ok, want_flow=True))),
				(("VK_ALG_RWMD",), lambda: c.query(q[None, :], algorithm=hip.VK_ALG_RWMD, **ok)),
				(("global alignment",), lambda: c.query(q[None, :], locality=hip.Locality.GLOBAL, **ok)),
				(("submatch",), lambda: c.query(q[None, :], submatch_weight=0.5, **ok)),
				(("more than one token",), lambda: c.query_batch([q[None, :], two], **ok))):
			refused(hip, hip.VK_ERR_UNSUPPORTED, ("span similarity",) + words, call)
			assert_exact(c.query(q[None, :], **ok), values, 5, 0.0, words)
		refused(hip, hip.VK_ERR_UNSUPPORTED, ("span similarity",), lambda: c.filtered(1, 0))
		assert_exact(c.query(q[None, :], **ok), values, 5, 0.0, "after a refused filter")
	finally:
		c.close()
