"""-m gpu: the booster of a Saliency compiled and kept on the device (vk_signal_*, vk_corpus_set_saliency), through the C-ABI
shim and through Session.

The compiled booster against the restatement in numpy / scipy (tests/saliency_cases.py): keyword signals over slices of 0, 1, 31, 32,
33, 63, 64, 65, 200 and 600 tokens and over windows of 3 sentences by 2, static and contextual handles, vocabularies of 37, 524,288
(the largest whose bitmap is staged in LDS) and 600,000 words (read from global memory); every filter case of the host tier; two
filtered signals and a custom one averaged.  Signals and boosts compare with ==, except behind a convolution: there within one float32
ulp, as on the host tier (numpy does not specify the order of its sum) -- and the boost behind it within one ulp too: at strength <= 0.5
a boost lies in [0.5, 1], where one ulp is 2^-24; a convolved signal below 1 that is off by its last place moves the float64 average by
less than w_k / sum(w) * 2^-24 < one ulp of the boost, which the one rounding to float32 turns into at most one.

Results under the resident booster against the same handle's results with that array passed per query: ids, scores, aligner scores,
mappings and edge similarities bit for bit, on every route that honours a boost."""

import ctypes as C

import numpy as np
import pytest

import bound_cases as bc
import saliency_cases as sc
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

V = 37
N_FILTER = 96   # slices of the handle the filter cases run on


# ---- corpora

def mixed_slices():
	"""the slices of the `mixed` corpora and the documents they belong to: document 0 the lengths that matter to the keyword kernel (a
	slice of at most 64 tokens is one trip of a wave, a longer one loops) and to the slice table (a slice of more than 64 tokens sits
	alone in a padded group of rows); documents 1 and 3 windows of 3 sentences by 2 over sentences of 1 .. 12 tokens -- neighbouring
	windows share a sentence; document 2 has no slices"""
	rng = np.random.default_rng(5)
	start, end, docs, at = [], [], [0], 0
	for n in (0, 1, 31, 32, 33, 63, 64, 65, 200, 600):
		start.append(at), end.append(at + n)
		at += n
	docs.append(len(start))
	for n_sent in (11, 0, 8):
		lens = rng.integers(1, 13, n_sent)
		sent_off = at + np.concatenate(([0], np.cumsum(lens)))
		for i in range(0, n_sent, 2):
			j = min(i + 2, n_sent - 1)
			start.append(int(sent_off[i])), end.append(int(sent_off[j + 1]))
		at = int(sent_off[-1])
		docs.append(len(start))
	return np.array(start, np.int64), np.array(end, np.int64), np.array(docs, np.int64), at


def static_handle(hip, ids, start, end, vocab=V, d=16, seed=3):
	rows = np.random.default_rng(seed).standard_normal((vocab, d)).astype(np.float32)
	c = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=d, n_tokens=len(ids), n_sentences=len(start), vocab_size=vocab, keep_magnitudes=True)
	c.append_vectors(rows, normalize=True)
	c.set_token_ids(ids)
	c.set_slices(start, end)
	c.finalize()
	return c


def contextual_handle(hip, X, off=None, slices=None, keep_magnitudes=True):
	n = len(off) - 1 if off is not None else len(slices[0])
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=X.shape[1], n_tokens=X.shape[0], n_sentences=n, keep_magnitudes=keep_magnitudes)
	c.append_vectors(synth.to_bf16_bits(synth.normalize_rows(X)), normalize=False)
	if off is not None:
		c.set_sentences(off)
	else:
		c.set_slices(*slices)
	c.finalize()
	return c


def read_signal(c, slot):
	"""a slot's signal: the average under weights (0, 1) is the signal itself -- (0 * 1 + 1 * s) / 1 in float64, rounded back"""
	return c.set_saliency([slot], [0.0, 1.0])


@pytest.fixture(scope="module")
def mixed(hip):
	start, end, docs, n_tokens = mixed_slices()
	rng = np.random.default_rng(11)
	ids = rng.integers(0, 31, n_tokens).astype(np.int32)   # words 31 .. 36 are in the vocabulary and in no document
	stat = static_handle(hip, ids, start, end)
	# the contextual handle: the same slices, its ids given per call -- a tenth of the tokens without an id, two beyond the vocabulary
	cids = ids.copy()
	cids[rng.random(n_tokens) < 0.1] = -1
	cids[[3, 700]] = V, 2 ** 31 - 1
	ctx = contextual_handle(hip, rng.standard_normal((n_tokens, 16)).astype(np.float32), slices=(start, end))
	yield dict(start=start, end=end, docs=docs, ids=ids, cids=cids, stat=stat, ctx=ctx)
	stat.close()
	ctx.close()


KEYWORDS = np.array([2, 7, 7, 19, 30, 33, 36], dtype=np.int32)   # one twice, two that no token has


# ---- the compiled booster against the restatement

@pytest.mark.parametrize("max_count", [1, 3])
def test_keyword_signals_are_the_restatements(hip, mixed, max_count):
	m = mixed
	assert (m["end"] - m["start"])[:10].tolist() == [0, 1, 31, 32, 33, 63, 64, 65, 200, 600]
	assert (m["start"][11:-1] < m["end"][10:-2]).any()   # windows overlap
	for c, ids, token_ids in ((m["stat"], m["ids"], None), (m["ctx"], m["cids"], m["cids"])):
		c.signal_keywords(0, KEYWORDS, max_count=max_count, token_ids=token_ids, vocab_size=V)
		got = read_signal(c, 0)
		want = sc.keyword_signal(ids, m["start"], m["end"], KEYWORDS, max_count)
		assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
		assert got[0] == 0.0 and got[9] == 1.0 and (max_count == 1 or len(np.unique(got)) == 4)
		c.clear_saliency()
	# no keyword at all: a signal of zeros
	m["stat"].signal_keywords(1, np.zeros(0, np.int32))
	assert not read_signal(m["stat"], 1).any()
	m["stat"].clear_saliency()


@pytest.mark.parametrize("vocab", [524288, 600000])
def test_keyword_signals_over_a_large_vocabulary(hip, vocab):
	"""524,288 words: the bitmap fills the 64 KiB a workgroup stages; 600,000: it stays in global memory.  Ids up to the last word"""
	rng = np.random.default_rng(vocab)
	off = np.concatenate(([0], np.cumsum(rng.integers(0, 70, 700)))).astype(np.int64)
	ids = rng.integers(0, vocab, int(off[-1])).astype(np.int32)
	ids[::7] = rng.integers(vocab - 64, vocab, len(ids[::7]))
	kw = np.unique(np.concatenate((rng.choice(ids, 300), [vocab - 1, vocab - 33, 0, 31, 32]))).astype(np.int32)
	c = static_handle(hip, ids, off[:-1], off[1:], vocab=vocab)
	try:
		c.signal_keywords(0, kw, max_count=3)
		got = read_signal(c, 0)
		want = sc.keyword_signal(ids, off[:-1], off[1:], kw, 3)
		assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and len(np.unique(got)) == 4
	finally:
		c.close()


@pytest.fixture(scope="module")
def filter_handle(hip):
	X = np.random.default_rng(2).standard_normal((N_FILTER, 16)).astype(np.float32)
	c = contextual_handle(hip, X, off=np.arange(N_FILTER + 1, dtype=np.int64), keep_magnitudes=False)
	yield c
	c.close()


@pytest.mark.parametrize("case", sc.filter_cases(N_FILTER), ids=lambda c: c[0])
def test_filters_are_the_restatements(hip, filter_handle, case):
	name, kind, width, pulse, off, x, want = case
	c = filter_handle
	c.signal_set(3, x)
	c.signal_filter(3, kind, width, off, pulse=pulse)
	got = read_signal(c, 3)
	c.clear_saliency()
	sc.assert_filtered(got, case)


def test_two_filtered_signals_and_a_custom_one_averaged(hip, mixed):
	m = mixed
	n = len(m["start"])
	custom = sc.signal_values(n, 9)
	pulse = sc.normalized(sc.gauss_pulse(5))
	k_max = sc.per_document(lambda x: sc.max_filter(x, 3), sc.keyword_signal(m["ids"], m["start"], m["end"], KEYWORDS, 2), m["docs"])
	k_conv = sc.per_document(lambda x: sc.conv_filter(x, pulse), sc.keyword_signal(m["ids"], m["start"], m["end"], KEYWORDS[:3], 1), m["docs"])
	c = m["stat"]
	before = c.device_bytes
	for conv in (False, True):
		c.signal_keywords(0, KEYWORDS, max_count=2)
		c.signal_filter(0, hip.VK_SIGNAL_FILTER_MAX, 3, m["docs"])
		c.signal_keywords(5, KEYWORDS[:3], max_count=1)
		if conv:
			c.signal_filter(5, hip.VK_SIGNAL_FILTER_CONV, 5, m["docs"], pulse=pulse)
		else:
			c.signal_filter(5, hip.VK_SIGNAL_FILTER_MAX, 4, m["docs"])
			c.signal_filter(5, hip.VK_SIGNAL_FILTER_MAX, 2, m["docs"])   # a filter on a filtered signal
		c.signal_set(2, custom)
		assert c.device_bytes > before
		w = np.array(sc.saliency_weights([2.0, 1.0, 0.5], 0.5))
		got = c.set_saliency([0, 5, 2], w)
		if conv:
			want = sc.average([k_max, k_conv, custom], w, n)
			assert int(sc.ulps(got, want).max()) <= 1, (got, want)
		else:
			second = sc.per_document(lambda x: sc.max_filter(x, 2), sc.per_document(lambda x: sc.max_filter(x, 4),
				sc.keyword_signal(m["ids"], m["start"], m["end"], KEYWORDS[:3], 1), m["docs"]), m["docs"])
			want = sc.average([k_max, second, custom], w, n)
			assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
		assert len(np.unique(got)) > 5 and got.min() >= 0.5 and got.max() <= 1.0
		# the slots are freed; what stays is the booster per row of the slice table (a long slice sits in a padded group of rows)
		resident = c.device_bytes - before
		assert 4 * (n + 8) <= resident <= 4 * (4 * n + 8)
		with pytest.raises(hip.VkError) as e:
			c.set_saliency([0], [0.5, 0.5])
		assert e.value.status == hip.VK_ERR_STATE
	# no signal: all ones
	assert (c.set_saliency([], [1.0]) == 1.0).all()
	c.clear_saliency()
	assert c.device_bytes == before


# ---- queries under the resident booster against the same array per query

W = (1 - 2.0 ** (-np.arange(0, 700) / 5)).astype(np.float32)
ALIGN = dict(gap_s=("table", W), gap_t=("table", W[:520]), max_matches=10)


def compile_booster(hip, c, ids, doc_off, strength=0.5):
	"""a booster of two smoothed keyword signals over token ids in [0, V)"""
	static = c.layout == hip.VK_LAYOUT_STATIC
	c.signal_keywords(0, KEYWORDS, max_count=2, token_ids=None if static else ids, vocab_size=V)
	c.signal_filter(0, hip.VK_SIGNAL_FILTER_MAX, 3, doc_off)
	c.signal_keywords(1, np.array([1, 4, 5, 11], np.int32), max_count=1, token_ids=None if static else ids, vocab_size=V)
	c.signal_filter(1, hip.VK_SIGNAL_FILTER_CONV, 7, doc_off, pulse=sc.normalized(sc.gauss_pulse(7)))
	b = c.set_saliency([0, 1], sc.saliency_weights([1.0, 2.0], strength))
	assert len(np.unique(b)) > 5
	return b


def restated_booster(ids, start, end, doc_off, strength=0.5):
	"""compile_booster in numpy / scipy (ids without -1 or ids beyond V)"""
	pulse = sc.normalized(sc.gauss_pulse(7))
	k0 = sc.per_document(lambda x: sc.max_filter(x, 3), sc.keyword_signal(ids, start, end, KEYWORDS, 2), doc_off)
	k1 = sc.per_document(lambda x: sc.conv_filter(x, pulse), sc.keyword_signal(ids, start, end, [1, 4, 5, 11], 1), doc_off)
	return sc.average([k0, k1], sc.saliency_weights([1.0, 2.0], strength), len(start))


def docs_of(n, per=50):
	return np.unique(np.concatenate((np.arange(0, n, per), [n]))).astype(np.int64)


def same_under_both(c, b, qv, n_min=1, **options):
	"""the query under the resident booster and with the same array of its own: the same result set, bit for bit"""
	resident = c.query(qv, boost=None, **options)
	own = c.query(qv, boost=b.copy(), **options)
	bc.same_results(resident, own)
	assert resident.n >= n_min
	return resident


@pytest.fixture(scope="module")
def ragged(hip):
	"""3,000 slices of 1 .. 64 tokens, five of them empty: several workgroups, slices across tile borders"""
	corpus = bc.ragged_with_empties(64, 3000, seed=61)
	c = contextual_handle(hip, corpus["X"], off=corpus["sent_off"])
	ids = (corpus["tok_id"] % V).astype(np.int32)
	plain = {len_t: c.query(synth.make_queries(corpus, 1, len_t)[0]["vectors"], **ALIGN) for len_t in (10, 20, 70)}
	b = compile_booster(hip, c, ids, docs_of(3000))
	off = corpus["sent_off"]
	assert int(sc.ulps(b, restated_booster(ids, off[:-1], off[1:], docs_of(3000))).max()) <= 1
	yield dict(c=c, corpus=corpus, b=b, plain=plain, ids=ids)
	c.close()


@pytest.mark.parametrize("len_t", [10, 20, 70])
def test_alignments_of_every_query_length(hip, ragged, len_t):
	r = ragged
	qv = synth.make_queries(r["corpus"], 1, len_t)[0]["vectors"]
	for locality in (0, 1):
		got = same_under_both(r["c"], r["b"], qv, locality=locality, min_score=0.0 if locality == 0 else -1e9, **ALIGN)
	got = same_under_both(r["c"], r["b"], qv, n_min=10, **ALIGN)
	# the booster shows: the scores are the unboosted ones times the slices' boosts, so some result differs
	plain = r["plain"][len_t]
	assert not np.array_equal(got.score[:got.n], plain.score[:plain.n])
	if len_t == 10:   # without tracebacks, and more matches than one block selects
		same_under_both(r["c"], r["b"], qv, want_flow=False, **ALIGN)
		same_under_both(r["c"], r["b"], qv, **dict(ALIGN, max_matches=100))


def test_transports_batches_and_listed_slices(hip, ragged):
	r = ragged
	c, b = r["c"], r["b"]
	qs = [q["vectors"] for q in synth.make_queries(r["corpus"], 6, 10)]
	same_under_both(c, b, qs[0], algorithm=hip.VK_ALG_RWMD, max_matches=10)
	same_under_both(c, b, qs[0], algorithm=hip.VK_ALG_WRD, max_matches=10)
	listed = np.array([7, 1, 2999, 1500, 8], dtype=np.int64)
	got = same_under_both(c, b, qs[0], only_slices=listed, min_score=-1.0, **ALIGN)
	assert got.sentence[:got.n].tolist() == [s for s in listed.tolist() if s in got.sentence[:got.n]]
	same_under_both(c, b, qs[0], submatch_weight=0.5, **ALIGN)
	# batches: alignments (the shared pass) and relaxed WMD (the GEMM pass); one call against one call
	for options in (dict(ALIGN), dict(algorithm=hip.VK_ALG_RWMD, max_matches=10)):
		resident = c.query_batch(qs, boost=None, **options)
		own = c.query_batch(qs, boost=b.copy(), **options)
		for x, y in zip(resident, own):
			bc.same_results(x, y)
			assert x.n == 10


def test_a_query_of_its_own_overrides_and_views_inherit_and_clear_restores(hip, ragged):
	r = ragged
	c, b = r["c"], r["b"]
	qv = synth.make_queries(r["corpus"], 1, 10)[0]["vectors"]
	resident = c.query(qv, **ALIGN)
	other = (2.0 - b).astype(np.float32)
	with_other = c.query(qv, boost=other, **ALIGN)
	assert not np.array_equal(with_other.score[:10], resident.score[:10])
	v = c.view()
	try:
		bc.same_results(v.query(qv, **ALIGN), resident)
		bc.same_results(v.query(qv, boost=other, **ALIGN), with_other)
		with pytest.raises(hip.VkError) as e:   # the booster belongs to the owning handle
			v.set_saliency([], [1.0])
		assert e.value.status == hip.VK_ERR_STATE
		bc.same_results(v.query(qv, **ALIGN), resident)
		c.clear_saliency()
		bc.same_results(c.query(qv, **ALIGN), r["plain"][10])
		bc.same_results(v.query(qv, **ALIGN), r["plain"][10])
		bc.same_results(c.query(qv, boost=other, **ALIGN), with_other)
		# set again with the view alive: both see it
		again = compile_booster(hip, c, r["ids"], docs_of(3000))
		assert np.array_equal(again, b)
		bc.same_results(v.query(qv, **ALIGN), resident)
		bc.same_results(c.query(qv, **ALIGN), resident)
	finally:
		v.close()


def test_the_bound_pass_runs_under_the_resident_booster(hip):
	"""VK_BOUND_PASS=force: the pass asks whether every boost is >= 0 -- for the resident booster that was answered when it was
	compiled.  A negative per-query boost still keeps its query off the pass"""
	corpus = bc.ragged_with_empties(300, 2000, seed=71)
	with bc.Env(VK_BOUND_PASS="force"):
		c = contextual_handle(hip, corpus["X"], off=corpus["sent_off"])
		try:
			ids = (corpus["tok_id"] % V).astype(np.int32)
			b = compile_booster(hip, c, ids, docs_of(2000))
			qv = synth.make_queries(corpus, 1, 10)[0]["vectors"]
			own = c.query(qv, boost=b.copy(), **ALIGN)
			assert bc.state(hip, c, bounds=False)[1][0] == 1
			resident = c.query(qv, **ALIGN)
			cnt = bc.state(hip, c, bounds=False)[1]
			assert cnt[0] == 1 and cnt[3] == 0   # the bound pass ran and did not fall back
			bc.same_results(resident, own)
			assert resident.n == 10
			negative = b.copy()
			negative[5] = -1.0
			c.query(qv, boost=negative, **ALIGN)
			assert bc.state(hip, c, bounds=False)[1][0] == 0
		finally:
			c.close()
	with bc.Env(VK_BOUND_PASS="off"):
		e = contextual_handle(hip, corpus["X"], off=corpus["sent_off"])
		try:
			bc.same_results(e.query(qv, boost=b, **ALIGN), resident)
		finally:
			e.close()


@pytest.mark.parametrize("layout", ["static", "contextual"])
def test_a_corpus_with_long_slices(hip, layout):
	"""slices of up to 400 tokens among short ones: the slice table has padded groups of rows, and the booster sits per row"""
	rng = np.random.default_rng(81)
	lens = rng.integers(1, 60, 600)
	lens[[3, 100, 101, 350, 599]] = [400, 65, 130, 257, 90]
	off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
	n_tokens = int(off[-1])
	ids = rng.integers(0, V, n_tokens).astype(np.int32)
	E = synth.make_vocab(V, 32)
	if layout == "static":
		c = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=32, n_tokens=n_tokens, n_sentences=600, vocab_size=V)
		c.append_vectors(E, normalize=True)
		c.set_token_ids(ids)
		c.set_sentences(off)
		c.finalize()
	else:
		c = contextual_handle(hip, E[ids] + 0.1 * rng.standard_normal((n_tokens, 32)).astype(np.float32), off=off)
	try:
		b = compile_booster(hip, c, ids, docs_of(600, 40))
		assert int(sc.ulps(b, restated_booster(ids, off[:-1], off[1:], docs_of(600, 40))).max()) <= 1   # per slice, not per row of the table
		for len_t in (10, 20, 70):
			qids = ids[off[3] + 5:off[3] + 5 + len_t]
			qv = E[qids] + 0.05 * rng.standard_normal((len_t, 32)).astype(np.float32)
			extra = dict(q_token_ids=qids) if layout == "static" else {}
			same_under_both(c, b, qv, n_min=10, **extra, **ALIGN)
		if layout == "contextual":
			same_under_both(c, b, qv[:10], algorithm=hip.VK_ALG_RWMD, max_matches=10)
	finally:
		c.close()


# ---- refusals

def test_refusals_return_their_status_and_leave_the_handle_as_it_was(hip, ragged):
	r = ragged
	c, b = r["c"], r["b"]
	qv = synth.make_queries(r["corpus"], 1, 10)[0]["vectors"]
	before = c.query(qv, **ALIGN)
	n = c.n_sentences

	def refused(status, call, *args, **kw):
		with pytest.raises(hip.VkError) as e:
			call(*args, **kw)
		assert e.value.status == status, str(e.value)
		bc.same_results(c.query(qv, **ALIGN), before)

	refused(hip.VK_ERR_INVALID, c.signal_keywords, 0, KEYWORDS)                                    # a contextual handle without ids
	refused(hip.VK_ERR_INVALID, c.signal_keywords, 8, KEYWORDS, token_ids=r["ids"], vocab_size=V)    # no such slot
	refused(hip.VK_ERR_INVALID, c.signal_keywords, -1, KEYWORDS, token_ids=r["ids"], vocab_size=V)
	refused(hip.VK_ERR_INVALID, c.signal_keywords, 0, [V], token_ids=r["ids"], vocab_size=V)         # a keyword outside the vocabulary
	refused(hip.VK_ERR_INVALID, c.signal_keywords, 0, KEYWORDS, max_count=0, token_ids=r["ids"], vocab_size=V)
	refused(hip.VK_ERR_STATE, c.signal_filter, 4, hip.VK_SIGNAL_FILTER_MAX, 3, docs_of(n))         # an empty slot
	c.signal_set(4, np.zeros(n, np.float32))
	refused(hip.VK_ERR_INVALID, c.signal_filter, 4, 2, 3, docs_of(n))                                # no such filter
	refused(hip.VK_ERR_INVALID, c.signal_filter, 4, hip.VK_SIGNAL_FILTER_MAX, 0, docs_of(n))
	refused(hip.VK_ERR_INVALID, c.signal_filter, 4, hip.VK_SIGNAL_FILTER_MAX, 4097, docs_of(n))
	refused(hip.VK_ERR_INVALID, c.signal_filter, 4, hip.VK_SIGNAL_FILTER_CONV, 3, docs_of(n))        # a convolution without its pulse
	refused(hip.VK_ERR_INVALID, c.signal_filter, 4, hip.VK_SIGNAL_FILTER_MAX, 3, docs_of(n)[:-1])   # documents that end before the slices
	refused(hip.VK_ERR_INVALID, c.signal_filter, 4, hip.VK_SIGNAL_FILTER_MAX, 3, np.array([0, 50, 40, n]))
	refused(hip.VK_ERR_INVALID, c.set_saliency, [4], [-0.5, 1.5])
	refused(hip.VK_ERR_INVALID, c.set_saliency, [4], [0.0, 0.0])
	refused(hip.VK_ERR_STATE, c.set_saliency, [4, 6], [0.5, 0.25, 0.25])                             # slot 6 holds nothing
	# the slot is still there after all of that, and the booster compiles as before
	assert np.array_equal(compile_booster(hip, c, r["ids"], docs_of(n)), b)
	bc.same_results(c.query(qv, **ALIGN), before)
	# before finalize: VK_ERR_STATE; under a span similarity: VK_ERR_UNSUPPORTED
	u = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=16, n_tokens=4, n_sentences=4)
	try:
		for call, args in ((u.signal_set, (0, np.zeros(4, np.float32))), (u.set_saliency, ([], [1.0])), (u.clear_saliency, ()),
				(u.signal_keywords, (0, [1], 1, np.zeros(4, np.int32), V)), (u.signal_filter, (0, 0, 3, [0, 4]))):
			with pytest.raises(hip.VkError) as e:
				call(*args)
			assert e.value.status == hip.VK_ERR_STATE
		u.set_span_sim((hip.VK_SIMSRC_PNORM, 2.0), [])
		u.append_vectors(np.random.default_rng(0).standard_normal((4, 16)).astype(np.float32))
		u.set_sentences(np.arange(5, dtype=np.int64))
		u.finalize()
		span_before = u.query(np.ones((1, 16), np.float32), max_matches=4, want_flow=False)
		for call, args in ((u.signal_set, (0, np.zeros(4, np.float32))), (u.set_saliency, ([], [1.0])), (u.signal_keywords, (0, [1], 1, np.zeros(4, np.int32), V))):
			with pytest.raises(hip.VkError) as e:
				call(*args)
			assert e.value.status == hip.VK_ERR_UNSUPPORTED
		bc.same_results(u.query(np.ones((1, 16), np.float32), max_matches=4, want_flow=False), span_before)
	finally:
		u.close()


def test_one_token_batches_leave_the_span_pass_for_a_booster(hip):
	"""the span batch pass takes no boost: a handle with a resident booster is kept off it as a query with a boost of its own is"""
	rng = np.random.default_rng(91)
	n = 500
	X = rng.standard_normal((n, 32)).astype(np.float32)
	c = contextual_handle(hip, X, off=np.arange(n + 1, dtype=np.int64), keep_magnitudes=False)
	try:
		lib = hip.lib()
		lib.vk_batch_state.argtypes = [C.c_void_p, C.c_void_p]

		def route():
			st = np.zeros(32, dtype=np.int64)
			hip._check(lib.vk_batch_state(c._h, st.ctypes.data))
			return int(st[0])
		qs = [X[i:i + 1] + 0.01 for i in (3, 77, 400, 9)]
		opts = dict(max_matches=5, want_flow=False)
		c.query_batch(qs, **opts)
		assert route() == 4   # the span pass
		b = compile_booster(hip, c, rng.integers(0, V, n).astype(np.int32), docs_of(n))
		resident = c.query_batch(qs, **opts)
		assert route() != 4
		own = c.query_batch(qs, boost=b.copy(), **opts)
		for x, y in zip(resident, own):
			bc.same_results(x, y)
			assert x.n == 5
	finally:
		c.close()


# ---- through Session

def test_through_session_the_matches_are_those_of_the_restatements_array(hip):
	from test_host_api import toy_session
	from test_saliency_backend import span_sim
	from vectorian_amd.saliency import CustomSignal, KeywordSignal, Saliency

	class EverySecond(CustomSignal):
		def spans_to_signal(self, spans):
			return np.array([0.25 * (i % 2) for i in range(len(spans))])

	session, emb, words, rng = toy_session(n_docs=4, sents_per_doc=30, V=200, d=32)
	part = session.partition("sentence", 3, 2)
	chosen = [words[i] for i in (20, 35, 50, 64, 80)]   # (the most chosen words would saturate every window)
	saliency = Saliency(strength=0.5)
	saliency.add_signal(KeywordSignal(*chosen, "nowhere", max_count=2).smoothed(3), weight=2)
	saliency.add_signal(KeywordSignal(words[30], words[45], same=lambda x, y: x == y).smoothed(2))
	saliency.add_signal(EverySecond(), weight=0.5)
	ids_all = np.concatenate([session.doc_token_ids(i) for i in range(4)])
	with part.index(span_sim(emb), saliency=saliency) as index:
		n, doc_off = index.n_slices, np.arange(0, 61, 15)
		assert n == 60
		vocab = session.vocab
		k0 = sc.keyword_signal(ids_all, index._slice_start, index._slice_end, [vocab.token_to_id(w) for w in chosen], 2)
		k1 = sc.keyword_signal(ids_all, index._slice_start, index._slice_end, [vocab.token_to_id(words[30]), vocab.token_to_id(words[45])], 1)
		want = sc.average([sc.per_document(lambda x: sc.max_filter(x, 3), k0, doc_off), sc.per_document(lambda x: sc.max_filter(x, 2), k1, doc_off),
			np.tile(np.array([0.25 * (i % 2) for i in range(15)], np.float32), 4)], sc.saliency_weights([2, 1.0, 0.5], 0.5), n)
		assert np.array_equal(index.boost.view(np.uint32), want.view(np.uint32)) and len(np.unique(want)) > 4
		doc = session.documents[2]
		texts = [" ".join(doc.tokens[40:48]), " ".join(session.documents[0].tokens[3:9])]
		res = [index.find(t, n=8) for t in texts]
		many = index.find_many(texts, n=8)
	with part.index(span_sim(emb), saliency=want) as by_array:
		ref = [by_array.find(t, n=8) for t in texts]
	key = lambda r: [(m.doc_index, m.slice_id, np.float32(m.score).view(np.uint32)) for m in r]
	for a, b, c in zip(res, many, ref):
		assert len(a) == 8 and key(a) == key(c) and key(b) == key(c)
	# a gauss-smoothed signal: the booster within one ulp of the restatement's
	smooth = Saliency(strength=0.5)
	smooth.add_signal(KeywordSignal(*chosen).smoothed(5, method="gauss"))
	with part.index(span_sim(emb), saliency=smooth) as index:
		k = sc.keyword_signal(ids_all, index._slice_start, index._slice_end, [vocab.token_to_id(w) for w in chosen], 1)
		pulse = sc.normalized(sc.gauss_pulse(5))
		want = sc.average([sc.per_document(lambda x: sc.conv_filter(x, pulse), k, doc_off)], sc.saliency_weights([1.0], 0.5), n)
		assert int(sc.ulps(index.boost, want).max()) <= 1 and len(np.unique(want)) > 4
