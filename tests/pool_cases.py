"""The inputs of the pooled-span tests (test_pool_host.py on the host, test_gpu_pooled_spans.py on the device) and what numpy makes of
them: AggregatedTokenImpl's own call, agg(v, axis=0) on the float32 rows of a span.  A case is generated from its width
alone and its expectation is computed once."""

import functools

import numpy as np

WIDTHS = (2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 768, 1025)
LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 33, 64, 65, 513)
AGGS = dict(mean=np.mean, min=np.min, max=np.max)
VOCAB = 50       # rows of the gathered cases: far fewer than tokens, so ids repeat
ZERO_ROW = 7     # ... one of them the zero row of an out-of-vocabulary word


def _values(rng, shape):
	"""three magnitudes side by side, so that the order of a sum shows in its last bits"""
	return (rng.standard_normal(shape) * rng.choice([1e-3, 1.0, 1e3], size=shape)).astype(np.float32)


def _spans(rng):
	"""one span of every length, end to end, in an order that puts the empty one in the middle; then two windows that overlap them"""
	order = [n for n in rng.permutation([n for n in LENGTHS if n])]
	order.insert(len(order) // 2, 0)
	start = np.concatenate(([0], np.cumsum(order)[:-1])).astype(np.int64)
	end = start + np.asarray(order, dtype=np.int64)
	total = int(end[-1])
	start = np.concatenate((start, [10, 20])).astype(np.int64)
	end = np.concatenate((end, [43, 53])).astype(np.int64)
	return start, end, total


def widen(bits):
	return (bits.astype(np.uint32) << 16).view(np.float32)


@functools.lru_cache(maxsize=None)
def _rows_case(d, bf16):
	rng = np.random.default_rng(1600 + d)
	start, end, total = _spans(rng)
	rows = _values(rng, (total, d))
	# one NaN component, inside the 33-token span
	i = int(np.nonzero(end - start == 33)[0][0])
	rows[int(start[i]) + 5, d // 2] = np.nan
	if bf16:
		rows = (rows.view(np.uint32) >> 16).astype(np.uint16)
	for a in (rows, start, end):
		a.setflags(write=False)
	return dict(name="rows", rows=rows, ids=None, start=start, end=end)


def rows_case(d, bf16=False):
	"""span i is rows[start[i] .. end[i])"""
	return _rows_case(d, bool(bf16))


@functools.lru_cache(maxsize=None)
def _gather_case(d, bf16):
	rng = np.random.default_rng(2600 + d)
	start, end, total = _spans(rng)
	rows = _values(rng, (VOCAB, d))
	rows[ZERO_ROW] = 0
	rows[11, d // 2] = np.nan
	ids = rng.integers(0, VOCAB, size=total).astype(np.int32)
	ids[ids == 11] = 12
	i = int(np.nonzero(end - start == 33)[0][0])
	ids[int(start[i]) + 5] = 11                       # the NaN once, in the 33-token span
	ids[int(start[i]) + 6] = ZERO_ROW
	i = int(np.nonzero(end - start == 2)[0][0])
	ids[int(start[i]):int(end[i])] = ZERO_ROW         # a span of out-of-vocabulary words only
	if bf16:
		rows = (rows.view(np.uint32) >> 16).astype(np.uint16)
	for a in (rows, ids, start, end):
		a.setflags(write=False)
	return dict(name="gather", rows=rows, ids=ids, start=start, end=end)


def gather_case(d, bf16=False):
	"""span i is rows[ids[start[i] .. end[i])]: repeated ids, the zero row, one NaN component"""
	return _gather_case(d, bool(bf16))


_expected = {}


def expected(case):
	"""{agg name: [n_spans x d] float32}: numpy's aggregate of every span's rows, a row of NaN for a span without tokens"""
	key = id(case["rows"])
	if key not in _expected:
		rows = case["rows"] if case["rows"].dtype == np.float32 else widen(case["rows"])
		out = {name: np.full((len(case["start"]), rows.shape[1]), np.nan, dtype=np.float32) for name in AGGS}
		with np.errstate(all="ignore"):
			for i, (a, b) in enumerate(zip(case["start"], case["end"])):
				v = rows[a:b] if case["ids"] is None else rows[case["ids"][a:b]]
				if v.shape[0] > 0:
					for name, agg in AGGS.items():
						out[name][i, :] = agg(v, axis=0)
		for o in out.values():
			o.setflags(write=False)
		_expected[key] = (case, out)   # (the case is kept: its id stays its own)
	return _expected[key][1]


def assert_pooled(got, want, agg, what=None):
	"""NaN in the same cells; elsewhere the mean bit for bit, the extrema value for value"""
	got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
	assert got.shape == want.shape, (what, agg, got.shape, want.shape)
	nan = np.isnan(want)
	assert np.array_equal(np.isnan(got), nan), (what, agg, "NaN cells differ", np.argwhere(np.isnan(got) != nan)[:5])
	if agg == "mean":
		same = (got.view(np.uint32) == want.view(np.uint32)) | nan
	else:
		same = (got == want) | nan
	assert same.all(), (what, agg, int((~same).sum()), np.argwhere(~same)[:5], got[~same][:5], want[~same][:5])


def sequential_mean(v):
	"""the header's MEAN in numpy: a row-by-row fp32 sum, divided once"""
	acc = v[0].astype(np.float32).copy()
	for row in v[1:]:
		acc = acc + row
	return acc / np.float32(len(v))


def pairwise_mean(v):
	def tree(x):
		return x[0] if len(x) == 1 else tree(x[:len(x) // 2]) + tree(x[len(x) // 2:])
	return tree(v) / np.float32(len(v))


# ---- the operator surface: a session of small documents under a static and a contextual embedding

STATIC_D, CONTEXTUAL_D = 52, 30


@functools.lru_cache(maxsize=None)
def toy_session(n_docs=40, seed=16):
	"""(session, {"static": embedding, "contextual": embedding}, query texts): documents of 2 .. 6 sentences of 1 .. 9 words; the word
	"unseen" is outside the static embedding (a zero row)"""
	from vectorian_amd.corpus import Document
	from vectorian_amd.embedding import ContextualEmbedding, StaticEmbedding
	from vectorian_amd.session import Session
	rng = np.random.default_rng(seed)
	words = [f"w{i}" for i in range(60)]
	static = StaticEmbedding("toy-static", words, _values(rng, (len(words), STATIC_D)))
	table = {}

	def contextual_rows(tokens):
		"""a vector per occurrence: the word's own plus its position's"""
		out = np.zeros((len(tokens), CONTEXTUAL_D), np.float32)
		for i, t in enumerate(tokens):
			if t not in table:
				table[t] = np.random.default_rng(1000 + len(table)).standard_normal(CONTEXTUAL_D).astype(np.float32)
			out[i] = table[t] + np.float32(0.05) * np.float32(i % 7)
		return out
	contextual = ContextualEmbedding("toy-contextual", CONTEXTUAL_D, contextual_rows)
	docs = []
	for _ in range(n_docs):
		sentences = [[str(w) for w in rng.choice(words + ["unseen"], size=int(rng.integers(1, 10)))] for _ in range(int(rng.integers(2, 7)))]
		tokens = [t for s in sentences for t in s]
		docs.append(Document(sentences, contextual_embeddings={"toy-contextual": contextual_rows(tokens)}))
	session = Session(docs, embeddings=[static, contextual])
	texts = [" ".join(docs[i]._sentences[j % len(docs[i]._sentences)]) for i, j in ((0, 0), (7, 1), (13, 2), (21, 0), (39, 1))] + ["w3 unseen w9 w9"]
	return session, dict(static=static, contextual=contextual), texts


def window_ranges(doc, partition):
	"""(slice id, first token, end token) of every window of a document: Spans::iterate, as the indexes enumerate them"""
	st, en = doc.spans[partition.level]["start"], doc.spans[partition.level]["end"]
	n = len(st)
	return [(sid, int(st[sid]), int(en[min(sid + partition.window_size - 1, n - 1)])) for sid in range(0, n, partition.window_step)]


def reference_span_vectors(session, partition, embedding):
	"""the reference's loop (AggregatedTokenImpl.encode): one numpy call per span, on the host; a span without tokens stays NaN"""
	emb = embedding.token_embedding
	out = []
	for doc in session.documents:
		for _, a, b in window_ranges(doc, partition):
			v = emb.encode_tokens(doc.tokens[a:b]).unmodified if emb.is_static else doc.contextual_vectors(emb.name)[a:b]
			out.append(embedding.agg(v, axis=0) if v.shape[0] > 0 else np.full(emb.dimension, np.nan, np.float32))
	return np.asarray(out, dtype=np.float32).reshape(len(out), emb.dimension)
