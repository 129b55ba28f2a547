"""-m gpu: every embedding width at which a kernel family changes form (width_cases.py holds the table and says which arm each
width is the edge of), on every route of its layout, HIP through the C-ABI against the oracle.  The rows are tail-heavy
(width_cases.tail_heavy; test_widths_host.py shows on the oracle alone that a lost or doubled tail feature cannot pass here).

Corpus per width (width_cases.slice_lengths): 240 slices of 0..40 tokens with empty ones, two of 65..200, one of 697 as the last
slice (`full`).  The library refuses some routes over such a corpus by contract (vk_validate_query): queries of more than 64 tokens
want slices of at most 64 (`short`: the 240 leading slices), the 1:n relaxed WMD and the exact transports slices of at most 512
(`mid`: the 242 leading slices, with magnitudes).  The GEMM forms of the batched relaxed WMD bucket slices of at most 64 tokens:
`short` again.  The handles take the raw rows and normalise them on the device (vk_pack.hip at every width too).

last_scores() against the oracle's score of every slice: width_cases.tol.  The largest difference per width is printed at the end
of the module (run with -s); DESIGN 7.3 records them."""

import numpy as np
import pytest

import width_cases as wc
from helpers import assert_same_results

pytestmark = pytest.mark.gpu

EXP5 = ("table", (1 - 2.0 ** (-np.arange(0, 1024) / 5)).astype(np.float32))   # covers the longest slice and the longest query
AFF = ("affine", 0.2, 0.05)
GAPS = {"linear": (0.1, 0.1), "affine": (AFF, AFF), "table": (EXP5, EXP5)}
CONTEXTUAL = [(layout, d) for layout in ("bf16", "f32") for d in wc.TABLES[layout]]
STATIC = list(wc.STATIC_WIDTHS)
# the shipped switches of the single-query pass (vk_query.cpp reads them per query), at the widths whose arm they choose
SWITCHES = [("bf16", d, name) for d in (289, 303, 304) for name in ("VK_QLDS", "VK_QREG")] + \
	[("bf16", d, "VK_NO_QLDS1") for d in (200, 512)] + [("f32", d, "VK_NO_F32_SPECIAL") for d in (289, 304)]

MAXIMA = {}             # (layout, d, route) -> largest |last_scores - oracle| seen


def note(layout, d, route, got, want):
	m = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if len(got) else 0.0
	MAXIMA[(layout, d, route)] = max(MAXIMA.get((layout, d, route), 0.0), m)


def norm(oracle, layout, x):
	"""(stored unit rows, magnitudes) as the oracle normalises and rounds them"""
	if layout == "f32":
		return oracle.normalize_rows(x), oracle.magnitudes(x)
	return oracle.normalize_rows_bf16(x)


class World:
	"""the inputs of one (layout, width) and the handles over them, built when first asked for"""

	def __init__(self, hip, oracle, layout, d):
		self.hip, self.oracle, self.layout, self.d = hip, oracle, layout, d
		self.case = wc.Case(layout, d)
		self.f32 = layout == "f32"
		self.rows, self.mag = self.norm(self.case.raw)
		self.handles = {}

	def norm(self, x):
		return norm(self.oracle, self.layout, x)

	def n_slices(self, which):
		c = self.case
		return {"full": c.n, "mid": min(c.n, c.n_short + 2), "short": c.n_short}[which]

	def off(self, which):
		return self.case.off[:self.n_slices(which) + 1]

	def handle(self, which):
		if which not in self.handles:
			hip, c, off = self.hip, self.case, self.off(which)
			T = int(off[-1])
			if self.layout == "static":
				h = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=self.d, n_tokens=T, n_sentences=len(off) - 1, vocab_size=wc.VOCAB)
				h.append_vectors(c.raw, normalize=True)
				h.set_token_ids(c.tok_id[:T])
			else:
				h = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=self.d, n_tokens=T, n_sentences=len(off) - 1,
					keep_magnitudes=which == "mid", precision="f32" if self.f32 else "bf16")
				h.append_vectors(c.raw[:T], normalize=True)
			h.set_sentences(off)
			h.finalize()
			self.handles[which] = h
		return self.handles[which]

	def sim(self, Q):
		"""the oracle's similarity rows of every token against one query (vko_sim_*: the arithmetic vko_find itself uses), computed once
		and handed to every vko_find over that query (S_rows) -- the dot products are most of the oracle's time at wide rows"""
		if self.layout == "static":
			return None
		return (self.oracle.sim_f32 if self.f32 else self.oracle.sim_bf16)(self.rows, Q)

	def find(self, which, Q, S=None, **kw):
		off = self.off(which)
		T = int(off[-1])
		if self.layout == "static":
			return self.oracle.find(layout=self.oracle.LAYOUT_STATIC, d=self.d, sent_off=off, tok_id=self.case.tok_id[:T], E=self.rows, Q=Q,
				n_threads=8, **kw)
		return self.oracle.find(layout=self.oracle.LAYOUT_CONTEXTUAL, d=self.d, sent_off=off, X=self.rows[:T], Q=Q, n_threads=8,
			S_rows=None if S is None else [S[:T]], **kw)

	def close(self):
		for h in self.handles.values():
			h.close()
		self.handles = {}


@pytest.fixture(scope="module")
def worlds(hip, oracle):
	made = {}

	def get(layout, d):
		if (layout, d) not in made:
			made[(layout, d)] = World(hip, oracle, layout, d)
		return made[(layout, d)]
	yield get
	for w in made.values():
		w.close()
	print("\nlargest |last_scores - oracle| per width and route")
	for key in sorted(MAXIMA):
		print("  %-6s d %-5d %-12s %.3g" % (*key, MAXIMA[key]))


def every_slice(w, which, route, project, ref):
	"""last_scores() of the handle against the oracle's score of every slice; empty slices are -inf"""
	every = w.handle(which).last_scores()
	live = np.diff(w.off(which)) > 0
	note(w.layout, w.d, route, every[live], ref["all_scores"][live])
	np.testing.assert_allclose(every[live], ref["all_scores"][live], atol=wc.tol(w.d, project), rtol=0)
	assert np.isneginf(every[~live]).all()


def alignments(w, which, lengths, route, among_short=False):
	"""every locality and gap family at each query length: winners bit for bit, every slice's score within the tolerance"""
	h = w.handle(which)
	for len_t in lengths:
		qv = w.case.query(len_t, among_short=among_short)
		Q = w.norm(qv)[0]
		S = w.sim(Q)
		for loc in (0, 1, 2):
			for name, (gs, gt) in GAPS.items():
				kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=10, min_score=0.0 if loc == 0 else -1e9)
				ref = w.find(which, Q, S, want_all_scores=True, **kw)
				got = h.query(qv, q_normalize=True, **kw)
				assert_same_results(got.trimmed(), ref)
				every_slice(w, which, route, 1e-4, ref)


@pytest.mark.parametrize("layout,d", CONTEXTUAL)
def test_single_query_alignments(worlds, layout, d):
	alignments(worlds(layout, d), "full", (1, 7, 16), "align")


@pytest.mark.parametrize("layout,d,switch", SWITCHES)
def test_single_query_alignments_under_a_switch(worlds, monkeypatch, layout, d, switch):
	"""MODE 0 with general gaps and MODE 3-300 with linear ones (VK_QREG / VK_QLDS), the generic kernel without its staged query tile
	(VK_NO_QLDS1), fp32 rows of 289..304 features on the generic fp32 kernel (VK_NO_F32_SPECIAL)"""
	monkeypatch.setenv(switch, "1")
	alignments(worlds(layout, d), "full", (1, 7, 16), "align")


@pytest.mark.parametrize("layout,d", CONTEXTUAL)
def test_long_queries(worlds, layout, d):
	"""24 and 40 tokens: vk_score32_kernel where its tiles fit, the sweeps (vk_docw / vk_docg / vk_wide) elsewhere; 100 tokens: vk_longq"""
	w = worlds(layout, d)
	alignments(w, "full", (24, 40), "align>16")
	alignments(w, "short", (100,), "align>64", among_short=True)


RWMD_FORMS = (("full", (True, True, True)), ("full", (True, False, False)), ("mid", (False, False, True)))


@pytest.mark.parametrize("layout,d", CONTEXTUAL)
def test_transports(worlds, layout, d):
	"""relaxed WMD, 1:1 symmetric / 1:1 one-sided bow / 1:n: winners restated from canonical rows, the oracle's floats; full WMD and WRD
	at the project's score_tol = tie_tol = 2e-5"""
	w = worlds(layout, d)
	hip, oracle = w.hip, w.oracle
	for len_t in (7, 16):
		qv = w.case.query(len_t, seed=1)
		Q, qmag = w.norm(qv)
		S = w.sim(Q)
		for which, flags in RWMD_FORMS:
			ref = w.find(which, Q, S, algorithm=oracle.ALG_RWMD, rwmd=flags, max_matches=10, min_score=-10.0, want_all_scores=True)
			got = w.handle(which).query(qv, q_normalize=True, algorithm=hip.VK_ALG_RWMD, rwmd=flags, max_matches=10, min_score=-10.0)
			assert_same_results(got.trimmed(), ref, check_mapping=False, exact=True)
			every_slice(w, which, "rwmd", 2e-5, ref)
		T = int(w.off("mid")[-1])
		for nbow in (False, True):
			ref = w.find("mid", Q, S, algorithm=oracle.ALG_RWMD, rwmd=(False, False, nbow), wmd_full=True, max_matches=10, min_score=0.0)
			got = w.handle("mid").query(qv, q_normalize=True, algorithm=hip.VK_ALG_RWMD, rwmd=(False, False, nbow), wmd_full=True,
				max_matches=10, min_score=0.0)
			assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)
		for norm in (False, True):
			ref = w.find("mid", Q, S, algorithm=oracle.ALG_WRD, X_mag=w.mag[:T], Q_mag=qmag, wrd_normalize=norm, max_matches=10, min_score=0.0)
			got = w.handle("mid").query(qv, q_normalize=True, algorithm=hip.VK_ALG_WRD, wrd_normalize=norm, max_matches=10, min_score=0.0)
			assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)


def alignment_batch(w, which, lengths):
	"""one vk_query_batch per locality and gap family: each result the oracle's and the single query's, bit for bit"""
	h = w.handle(which)
	qs = [w.case.query(m, seed=i, among_short=which == "short") for i, m in enumerate(lengths)]
	Qs = [w.norm(qv)[0] for qv in qs]
	Ss = [w.sim(Q) for Q in Qs]
	for loc in (0, 1, 2):
		for name, (gs, gt) in GAPS.items():
			kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=9, min_score=0.0 if loc == 0 else -1e9)
			outs = h.query_batch(qs, q_normalize=True, **kw)
			assert len(outs) == len(qs)
			for qv, Q, S, got in zip(qs, Qs, Ss, outs):
				assert_same_results(got.trimmed(), w.find(which, Q, S, **kw))
				single = h.query(qv, q_normalize=True, **kw)
				assert got.n == single.n and (got.sentence[:got.n] == single.sentence[:single.n]).all()
				assert (got.score[:got.n].view(np.uint32) == single.score[:single.n].view(np.uint32)).all()
				np.testing.assert_array_equal(got.mapping[:got.n], single.mapping[:single.n])


@pytest.mark.parametrize("layout,d", CONTEXTUAL)
def test_alignment_batch(worlds, layout, d):
	"""seven queries of 1..16 tokens, common options, over the slices of at most 40 tokens: what query_batch_shared_pass takes
	(vk_batch.cpp: bf16 rows, nk32 <= 10, no slice of more than 64 tokens, no query of more than 16) -- vk_score_batch_kernel and its
	(10,1) arm at 289 / 303 / 304, its last nk32 at 305; wider rows and fp32 rows are answered query by query"""
	alignment_batch(worlds(layout, d), "short", (11, 3, 16, 1, 8, 12, 5))


@pytest.mark.parametrize("layout,d", CONTEXTUAL)
def test_alignment_batch_falls_back(worlds, layout, d):
	"""a batch with a 24-token query over the corpus that ends with the 697-token slice: the shared pass refuses both, vk_query_batch
	answers query by query"""
	alignment_batch(worlds(layout, d), "full", (11, 24, 1, 16))


def rwmd_batches(hip, oracle, layout, h, find, make_query):
	for n_q, len_t, flags in ((9, 6, (True, True, True)), (40, 10, (True, False, True))):
		qs = [make_query(len_t, i) for i in range(n_q)]
		qs[1] = qs[1][:max(1, len_t - 3)]
		qs[-1] = qs[-1][:1]
		for i in range(5, n_q, 7):
			qs[i] = qs[i][:1 + (i * 3) % len_t]
		kw = dict(rwmd=flags, max_matches=9, min_score=0.0)
		outs = h.query_batch(qs, q_normalize=True, algorithm=hip.VK_ALG_RWMD, **kw)
		assert len(outs) == n_q
		for qv, got in zip(qs, outs):
			ref = find(norm(oracle, layout, qv)[0], algorithm=oracle.ALG_RWMD, **kw)
			assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)
			single = h.query(qv, q_normalize=True, algorithm=hip.VK_ALG_RWMD, **kw)
			assert got.n == single.n
			np.testing.assert_allclose(got.score[:got.n], single.score[:single.n], atol=2e-6, rtol=0)


@pytest.mark.parametrize("layout,d", CONTEXTUAL)
def test_rwmd_batch_ragged(worlds, layout, d):
	"""batches of 9 and 40 relaxed-WMD queries over the ragged slices of at most 40 tokens: vk_rwmd_batch<4> / <10,true> / <24> at their
	edge widths, the shared pass or the per-query path elsewhere"""
	w = worlds(layout, d)
	rwmd_batches(w.hip, w.oracle, layout, w.handle("short"), lambda Q, **kw: w.find("short", Q, **kw), lambda len_t, i: w.case.query(len_t, seed=i, among_short=True))


@pytest.mark.parametrize("layout,d", CONTEXTUAL)
def test_rwmd_batch_uniform32(hip, oracle, layout, d):
	"""200 slices of 32 tokens: the 32-row kernels (queries share A tiles; 16 queries per five tiles from 32 queries on)"""
	rng = np.random.default_rng(d)
	n = 20 if d in wc.SMALL else 200
	raw = wc.tail_heavy(wc.with_common_direction(rng.standard_normal((n * 32, d)), rng))
	rows = norm(oracle, layout, raw)[0]
	off = np.arange(n + 1, dtype=np.int64) * 32
	h = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=n * 32, n_sentences=n, precision="f32" if layout == "f32" else "bf16")
	h.append_vectors(raw, normalize=True)
	h.set_sentences(off)
	h.finalize()

	def make_query(len_t, i):
		a = 32 * (i * 7 % n) + i % 20
		return wc.noisy_copy(raw[a:a + len_t], np.random.default_rng(1000 * d + i))

	try:
		rwmd_batches(hip, oracle, layout, h, lambda Q, **kw: oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=d, sent_off=off, X=rows, Q=Q, n_threads=8, **kw), make_query)
	finally:
		h.close()


@pytest.mark.parametrize("layout,d", CONTEXTUAL)
def test_span_index(hip, oracle, layout, d):
	"""500 one-token slices, a one-token local query (launch_span<10,true> / <24> / <12> / <32> and the generic form, bf16 and fp32): every
	slice's score is the clipped cosine of the stored rows in double precision, the winners are the oracle's"""
	n = 500
	rng = np.random.default_rng(3 * d + 1)
	raw = wc.tail_heavy(wc.with_common_direction(rng.standard_normal((n, d)), rng))
	raw[n // 2] = -raw[0]            # a negative cosine: clipped to 0
	rows = norm(oracle, layout, raw)[0]
	h = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=n, n_sentences=n, precision="f32" if layout == "f32" else "bf16")
	h.append_vectors(raw, normalize=True)
	h.set_sentences(np.arange(n + 1, dtype=np.int64))
	h.finalize()
	try:
		qv = wc.noisy_copy(raw[0:1], rng)
		Q = norm(oracle, layout, qv)[0]
		as_f64 = lambda r: (r if layout == "f32" else oracle.bf16_to_f32(r)).astype(np.float64)
		cos = np.clip(as_f64(rows) @ as_f64(Q)[0], 0.0, 1.0)
		kw = dict(locality=0, gap_s=0.1, gap_t=0.1, max_matches=20, min_score=-1.0)
		got = h.query(qv, q_normalize=True, **kw)
		every = h.last_scores()
		note(layout, d, "span", every, cos)
		# 2e-6 holds in the suite up to 1,024 features (test_span_kernel_every_slice); beyond: width_cases.tol
		np.testing.assert_allclose(every, cos, atol=2e-6 if wc.d_pad(d) <= 1024 else wc.tol(d, 2e-6), rtol=0)
		assert cos[n // 2] == 0.0 and got.n == 20
		ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=d, sent_off=np.arange(n + 1, dtype=np.int64), X=rows, Q=Q, **kw)
		assert_same_results(got.trimmed(), ref)
	finally:
		h.close()


def static_query(w, len_t, seed=0):
	"""(raw vectors, ids): tokens of a slice, one id twice, one id of -1 whose vector is a noisy copy of the word that stood there"""
	ids = w.case.static_ids(len_t, seed)
	qv = w.case.query(len_t, seed)                # noisy copies of those tokens' vectors ...
	known = ids >= 0
	qv[known] = w.case.raw[ids[known]]            # ... kept only where the id is -1
	return qv, ids


@pytest.mark.parametrize("d", STATIC)
def test_static_alignments(worlds, d):
	w = worlds("static", d)
	h = w.handle("full")
	for len_t in (7, 24):
		qv, ids = static_query(w, len_t)
		Q = w.norm(qv)[0]
		for loc in (0, 1, 2):
			for name, (gs, gt) in GAPS.items():
				kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=10, min_score=0.0 if loc == 0 else -1e9)
				ref = w.find("full", Q, q_ids=ids, want_all_scores=True, **kw)
				got = h.query(qv, q_token_ids=ids, q_normalize=True, **kw)
				assert_same_results(got.trimmed(), ref)
				every_slice(w, "full", "align", 1e-4, ref)


@pytest.mark.parametrize("d", STATIC)
def test_static_rwmd_single_and_batched(worlds, d):
	"""relaxed WMD over the static layout: the similarity table over the vocabulary at this width (vk_table_batch_kernel), single and
	as a batch with token_ids=; winners bit for bit with flows, within 2e-5 without"""
	w = worlds("static", d)
	hip, oracle = w.hip, w.oracle
	h = w.handle("short")
	qs, qids = zip(*[static_query(w, (7, 10, 4, 16, 10, 2, 9, 10, 5)[i], seed=i) for i in range(9)])
	for flags in ((True, True, True), (True, False, False)):
		kw = dict(rwmd=flags, max_matches=10, min_score=0.0)
		refs = [w.find("short", w.norm(qv)[0], q_ids=ids, algorithm=oracle.ALG_RWMD, want_all_scores=True, **kw) for qv, ids in zip(qs, qids)]
		outs = h.query_batch(list(qs), token_ids=list(qids), q_normalize=True, algorithm=hip.VK_ALG_RWMD, **kw)
		for qv, ids, got, ref in zip(qs, qids, outs, refs):
			assert_same_results(got.trimmed(), ref, check_mapping=False, exact=True)
			one = h.query(qv, q_token_ids=ids, q_normalize=True, algorithm=hip.VK_ALG_RWMD, **kw)
			assert got.n == one.n and (got.sentence[:got.n] == one.sentence[:one.n]).all()
			assert (got.score[:got.n].view(np.uint32) == one.score[:one.n].view(np.uint32)).all()
			every_slice(w, "short", "rwmd", 2e-5, ref)
		outs = h.query_batch(list(qs), token_ids=list(qids), q_normalize=True, algorithm=hip.VK_ALG_RWMD, want_flow=False, **kw)
		for got, ref in zip(outs, refs):
			assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)


def host_filter(pos, pos_mask):
	"""TokenFilter::pass over POS codes (test_gpu_token_filter.host_filter, one mask)"""
	keep = ~np.array([(int(pos_mask) >> int(p)) & 1 for p in pos], dtype=bool)
	return keep, np.concatenate(([0], np.cumsum(keep))).astype(np.int64)


@pytest.mark.parametrize("d", (5, 289, 1024))
def test_token_filter(worlds, d):
	"""vk_corpus_filter repacks the tiles on the device (vk_filter.hip): the filtered handle answers as the oracle does on the corpus
	compacted on the host"""
	w = worlds("bf16", d)
	hip, oracle, case = w.hip, w.oracle, w.case
	T = int(case.off[-1])
	pos = np.random.default_rng(d).integers(0, 7, size=T).astype(np.int8)
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=T, n_sentences=case.n)
	c.append_vectors(case.raw, normalize=True)
	c.set_sentences(case.off)
	c.finalize()
	c.set_token_pos(pos)
	pos_mask = (1 << 2) | (1 << 5)
	keep, new_index = host_filter(pos, pos_mask)
	f = c.filtered(pos_mask, 0)
	try:
		f_off = new_index[case.off]
		live = np.diff(f_off) > 0
		base = dict(layout=oracle.LAYOUT_CONTEXTUAL, d=d, sent_off=f_off, X=w.rows[keep], max_matches=12, want_all_scores=True, n_threads=8)
		for len_t in (7, 16):
			qv = case.query(len_t, seed=2)
			Q = w.norm(qv)[0]
			S = w.sim(Q)[keep]
			for kw in (dict(gap_s=0.1, gap_t=0.1), dict(gap_s=EXP5, gap_t=EXP5, locality=2, min_score=-1e9), dict(algorithm=hip.VK_ALG_RWMD)):
				ref = oracle.find(Q=Q, S_rows=[S], **base, **kw)
				got = f.query(qv, q_normalize=True, max_matches=12, **kw)
				assert_same_results(got.trimmed(), ref, check_mapping="algorithm" not in kw, exact=True)
				every = f.last_scores()
				note("bf16", d, "filter", every[live], ref["all_scores"][live])
				np.testing.assert_allclose(every[live], ref["all_scores"][live], atol=wc.tol(d, 2e-5 if "algorithm" in kw else 1e-4), rtol=0)
				assert np.isneginf(every[~live]).all()
	finally:
		f.close()
		c.close()
