"""-m gpu: span vectors pooled from token rows on the device (vk_corpus_append_pooled, vk_pool_spans_kernel).
The aggregates the call hands back (pooled_out) are held against numpy's own agg(v, axis=0) on the span's float32 rows -- the mean
bit for bit, minimum and maximum value for value, NaN in the same cells -- for every width and span length of pool_cases.py, rows as
they are and gathered through token ids, fp32 and bf16, from host and from device memory.  A corpus built by append_pooled answers
vk_query and vk_query_batch as one built by append_vectors from numpy's aggregates does, with ==; an AggregatedSpanEmbedding index
returns the matches of a span index given the reference's loop as vectors=; every refusal leaves the handle usable.
Everything is generated from seeds: nothing outside the repository is read."""

import numpy as np
import pytest

import pool_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
	import torch
	return torch


def on_device(torch, rows):
	t = torch.from_numpy(rows.view(np.int16) if rows.dtype == np.uint16 else rows).to(torch.device("cuda", 0))
	torch.cuda.synchronize()
	return t


@pytest.mark.parametrize("kind", ["rows", "gather"])
@pytest.mark.parametrize("d", pc.WIDTHS)
def test_pooled_out_is_numpys_aggregate(hip, torch, d, kind):
	make = pc.rows_case if kind == "rows" else pc.gather_case
	n = len(make(d)["start"])
	with hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=12 * n, n_sentences=12 * n) as c:
		for bf16 in (False, True):
			case = make(d, bf16=bf16)
			rows, want = np.array(case["rows"]), pc.expected(case)
			dev = on_device(torch, rows)
			for mem in ("host", "device"):
				for agg in ("mean", "min", "max"):
					if mem == "host":
						got = c.append_pooled(rows, case["start"], case["end"], agg, ids=case["ids"], want_pooled=True)
					else:
						got = c.append_pooled_device(dev.data_ptr(), rows.shape[0], hip.VK_BF16 if bf16 else hip.VK_F32, case["start"], case["end"],
							pc.AGGS[agg], ids=case["ids"], want_pooled=True)
					pc.assert_pooled(got, want[agg], agg, (d, kind, "bf16" if bf16 else "f32", mem))
			del dev


def test_rows_off_the_16_byte_boundary_take_the_element_form(hip, torch):
	"""device rows whose base is not a multiple of 16 bytes: the launcher must not read them in 16-byte pieces"""
	d = 300
	case = pc.rows_case(d)
	rows = np.array(case["rows"])
	flat = on_device(torch, np.concatenate((np.zeros(1, np.float32), rows.ravel())))   # the rows start 4 bytes into the allocation
	n = len(case["start"])
	with hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=n, n_sentences=n) as c:
		got = c.append_pooled_device(flat.data_ptr() + 4, rows.shape[0], hip.VK_F32, case["start"], case["end"], "mean", want_pooled=True)
	pc.assert_pooled(got, pc.expected(case)["mean"], "mean", "unaligned")


def test_spans_without_tokens_need_no_rows(hip):
	d = 12
	none = np.zeros(3, np.int64)
	with hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=6, n_sentences=6) as c:
		for got in (c.append_pooled(np.zeros((0, d), np.float32), none, none, "mean", want_pooled=True),
				c.append_pooled_device(0, 0, hip.VK_F32, none, none, "max", want_pooled=True)):
			assert got.shape == (3, d) and np.isnan(got).all()


def span_corpus(hip, d, n):
	return hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=n, n_sentences=n)


def finish(c, n):
	c.set_sentences(np.arange(n + 1, dtype=np.int64))
	c.finalize()


@pytest.mark.parametrize("agg", ["mean", "min", "max"])
@pytest.mark.parametrize("d", [300, 768])
def test_a_pooled_corpus_answers_as_one_appended_from_numpy(hip, d, agg):
	"""300 spans, 20 queries: the same result sets from vk_query and from vk_query_batch, ids and scores with =="""
	rng = np.random.default_rng(d + len(agg))
	n, gather = 300, d == 300
	lens = rng.integers(1, 41, size=n)
	lens[150] = 0                                       # an empty span: a row of NaN, packed as a zero row by both
	start = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
	end = start + lens
	start[10:20] = np.maximum(start[10:20] - 7, 0)      # some overlap their neighbours
	total = int(end[-1])
	if gather:
		rows = rng.standard_normal((500, d)).astype(np.float32)
		rows[3] = 0
		ids = rng.integers(0, 500, size=total).astype(np.int32)
		tokens = rows[ids]
	else:
		rows, ids = rng.standard_normal((total, d)).astype(np.float32), None
		tokens = rows
	want = np.full((n, d), np.nan, np.float32)
	for i in range(n):
		if end[i] > start[i]:
			want[i] = pc.AGGS[agg](tokens[start[i]:end[i]], axis=0)
	queries = [np.ascontiguousarray(want[i:i + 1] + 0.1 * rng.standard_normal((1, d)).astype(np.float32)) for i in rng.integers(0, 150, size=20)]
	options = dict(q_normalize=True, gap_s=0.0, gap_t=0.0, want_flow=False, max_matches=10, min_score=0.05)
	with span_corpus(hip, d, n) as pooled, span_corpus(hip, d, n) as plain:
		got = pooled.append_pooled(rows, start, end, agg, ids=ids, normalize=True, want_pooled=True)
		pc.assert_pooled(got, want, agg, (d, agg))
		plain.append_vectors(want, normalize=True)
		finish(pooled, n)
		finish(plain, n)
		results = []
		for c in (pooled, plain):
			single = [c.query(q, **options) for q in queries]
			batch = c.query_batch(queries, **options)
			results.append([(t.n, t.sentence[:t.n].tolist(), t.score[:t.n].tolist()) for t in single + list(batch)])
		assert all(r[0] >= 1 for r in results[0])
		assert results[0] == results[1]
		assert results[0][:20] == results[0][20:]       # the batch is 20 calls of vk_query


@pytest.mark.parametrize("embedding", ["static", "contextual"])
@pytest.mark.parametrize("partition", [("sentence", 1, None), ("sentence", 3, 2), ("document", 1, None)])
def test_an_aggregated_index_finds_what_the_reference_loop_finds(hip, partition, embedding):
	"""index.find and index.find_many of an AggregatedSpanEmbedding index against a span index given vectors= -- the reference's loop,
	one numpy call per span on the host -- match for match, for mean, min and max"""
	from vectorian_amd.sim import AggregatedSpanEmbedding
	session, embeddings, texts = pc.toy_session()
	part = session.partition(*partition)
	key = lambda result: [(session.documents.index(m.prepared_doc), m.slice_id, m.score) for m in result]
	for agg in (np.mean, np.min, np.max):
		emb = AggregatedSpanEmbedding(embeddings[embedding], agg)
		vectors = pc.reference_span_vectors(session, part, emb)
		with_device = part.index(emb.to_sentence_sim())
		with_vectors = part.index(emb.to_sentence_sim(), vectors=vectors)
		try:
			assert with_device._corpus.n_sentences == len(vectors) >= 40
			found = 0
			for text in texts:
				a, b = with_device.find(text, n=5, min_score=0.01), with_vectors.find(text, n=5, min_score=0.01)
				assert key(a) == key(b), (partition, embedding, agg, text)
				found += len(a)
			assert found >= len(texts)
			many_a, many_b = with_device.find_many(texts, n=5, min_score=0.01), with_vectors.find_many(texts, n=5, min_score=0.01)
			assert [key(r) for r in many_a] == [key(r) for r in many_b]
			assert [key(r) for r in many_a] == [key(with_device.find(t, n=5, min_score=0.01)) for t in texts]
		finally:
			with_device.close()
			with_vectors.close()


def test_every_refusal_leaves_the_handle_usable(hip):
	d, n = 8, 6
	rng = np.random.default_rng(5)
	rows = rng.standard_normal((20, d)).astype(np.float32)
	ids = rng.integers(0, 20, size=30).astype(np.int32)
	one = (np.array([0], np.int64), np.array([4], np.int64))
	appended = 0

	def refused(c, status, call):
		with pytest.raises(hip.VkError) as e:
			call()
		assert e.value.status == status, (e.value.status, str(e.value))

	with span_corpus(hip, d, n) as c:
		def usable():
			nonlocal appended
			got = c.append_pooled(rows, *one, "max", want_pooled=True)
			assert np.array_equal(got[0], rows[0:4].max(axis=0))
			appended += 1
		lib = hip.lib()
		st, en = hip._np_ptr(one[0]), hip._np_ptr(one[1])
		# null arguments
		refused(c, hip.VK_ERR_INVALID, lambda: hip._check(lib.vk_corpus_append_pooled(c._h, None, 20, hip.VK_F32, hip.VK_MEM_HOST, None, 0, st, en, 1, 0, 1, None)))
		refused(c, hip.VK_ERR_INVALID, lambda: hip._check(lib.vk_corpus_append_pooled(c._h, hip._np_ptr(rows), 20, hip.VK_F32, hip.VK_MEM_HOST, None, 0, None, en, 1, 0, 1, None)))
		refused(c, hip.VK_ERR_INVALID, lambda: hip._check(lib.vk_corpus_append_pooled(None, hip._np_ptr(rows), 20, hip.VK_F32, hip.VK_MEM_HOST, None, 0, st, en, 1, 0, 1, None)))
		usable()
		refused(c, hip.VK_ERR_INVALID, lambda: c.append_pooled(rows, *one, 3))                                 # unknown agg
		usable()
		refused(c, hip.VK_ERR_INVALID, lambda: c.append_pooled(rows, [5], [4], "mean"))                        # start > end
		refused(c, hip.VK_ERR_INVALID, lambda: c.append_pooled(rows, [0], [21], "mean"))                       # outside the rows
		refused(c, hip.VK_ERR_INVALID, lambda: c.append_pooled(rows, [-1], [2], "mean"))
		refused(c, hip.VK_ERR_INVALID, lambda: c.append_pooled(rows, [0], [31], "mean", ids=ids))              # outside the ids
		usable()
		bad = ids.copy()
		bad[17] = 20
		refused(c, hip.VK_ERR_INVALID, lambda: c.append_pooled(rows, [0], [30], "mean", ids=bad))              # an id outside [0, n_rows)
		bad[17] = -1
		refused(c, hip.VK_ERR_INVALID, lambda: c.append_pooled(rows, [0], [30], "mean", ids=bad))
		refused(c, hip.VK_ERR_INVALID, lambda: c.append_pooled(rows, [0] * 4, [3] * 4, "mean"))                # more rows than declared (3 + 4 > 6)
		usable()
		# a span of more than 2^24 tokens: (float)n is not exact
		long_ids = np.zeros((1 << 24) + 1, np.int32)
		refused(c, hip.VK_ERR_UNSUPPORTED, lambda: c.append_pooled(rows, [0], [len(long_ids)], "mean", ids=long_ids))
		usable()
		assert appended == 5
		got = c.append_pooled(rows, [0], [30], "min", ids=ids, want_pooled=True)                                # the sixth row
		assert np.array_equal(got[0], rows[ids].min(axis=0))
		finish(c, n)
		refused(c, hip.VK_ERR_STATE, lambda: c.append_pooled(rows, *one, "mean"))                               # finalized
		view = c.view()
		try:
			refused(view, hip.VK_ERR_STATE, lambda: view.append_pooled(rows, *one, "mean"))                     # a view
		finally:
			view.close()
		top = c.query(rows[0:4].max(axis=0)[None, :], q_normalize=True, gap_s=0.0, gap_t=0.0, want_flow=False, max_matches=3)
		assert top.n == 3 and top.sentence[0] in range(5) and top.score[0] > 0.99   # (rows 0 .. 4 are the same aggregate)
	# a static handle, with and without a similarity source
	for source in (None, (hip.VK_SIMSRC_PNORM, 2.0)):
		with hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=d, n_tokens=30, n_sentences=3, vocab_size=20) as s:
			if source:
				s.set_sim_source(*source)
			refused(s, hip.VK_ERR_UNSUPPORTED, lambda: s.append_pooled(rows, *one, "mean"))
			s.append_vectors(rows, normalize=True)                                                              # ... and goes on as before
			s.set_token_ids(ids)
			s.set_sentences(np.array([0, 10, 20, 30], np.int64))
			s.finalize()
