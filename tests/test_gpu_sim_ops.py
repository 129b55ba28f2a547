"""-m gpu: operator chains on the cosine over static corpora (vk_corpus_set_sim_ops).

The reference of every check: the oracle only knows the clipped cosine, so the table of a chain is stated around it
(sim_ops_cases.chain_table) -- the unclipped canonical cosine as sim_bf16(E, Q) - sim_bf16(E, -Q), the chain in numpy float32 exactly as
vectorian_amd/kernel.py states it, sim[id(t_j)][j] = 1, the clip -- and handed to the oracle's contextual route as a caller-supplied
matrix (S_rows), whose alignments are those of its static route.  Transports key their bags of words by token id, so their slices are
scored one by one (oracle.rwmd / wmd / wrd on the gathered rows) and ranked here as the oracle ranks."""

import numpy as np
import pytest

import sim_ops_cases as sc
from helpers import assert_same_results
from sim_ops_backend import ChainOracleCorpus
from vectorian_amd import alignment, synth
from vectorian_amd.corpus import Document
from vectorian_amd.embedding import StaticEmbedding
from vectorian_amd.session import Session
from vectorian_amd.sim import Bias, CosineSim, EmbeddingTokenSim, ModifiedVectorSim, OptimizedSpanSim, Scale

pytestmark = pytest.mark.gpu


def exp5(n):
	return (1 - 2.0 ** (-np.arange(n) / 5)).astype(np.float32)


def gaps(name, longest):
	return {"linear": (0.1, 0.05), "affine": (("affine", 0.2, 0.05), ("affine", 0.1, 0.02)),
		"exp5": (("table", exp5(max(512, longest) + 1)), ("table", exp5(513)))}[name]


LOCALITIES = ((0, 0.0), (1, -1e9), (2, -1e9))   # (locality, min_score)


class Case:
	"""a static corpus on the device and what the oracle needs of it"""

	def __init__(self, hip, V, d, n, lo, hi, extra=(), seed=7):
		st = synth.make_static_corpus(n, lo, hi, V, d, seed=seed)
		rng = np.random.default_rng(seed + 100)
		lens = list(np.diff(st["sent_off"])) + list(extra)
		ids = np.concatenate([st["tok_id"], synth.zipf_ids(int(sum(extra)), V, rng)]).astype(np.int32)
		self.off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
		self.ids, self.V, self.d = ids, V, d
		self.E = st["E"]
		self.Eb = synth.to_bf16_bits(synth.normalize_rows(self.E))
		self.longest = int(max(lens))
		self.hip = hip
		self.c = self.handle()

	def handle(self):
		c = self.hip.Corpus(layout=self.hip.VK_LAYOUT_STATIC, d=self.d, n_tokens=len(self.ids), n_sentences=len(self.off) - 1, vocab_size=self.V)
		c.append_vectors(self.Eb, normalize=False)
		c.set_token_ids(self.ids)
		c.set_sentences(self.off)
		c.finalize()
		return c

	def query(self, len_t, seed, noise=0.15):
		"""len_t tokens quoted from a slice (from several, when none is that long), with a repeated word (the same vector twice), a word
		outside the vocabulary (id -1, a vector of its own) and noise on every vector: no cosine reaches 1.  noise = 0: the vocabulary's
		own vectors, as the transports need them -- upstream writes a distance of its joint vocabulary twice where both documents hold
		both words (wmd.h:121-133), and the two writes agree because cos(u, v) = cos(v, u) bit for bit"""
		rng = np.random.default_rng(1000 * len_t + seed)
		start = int(rng.integers(0, len(self.ids) - len_t))
		q_ids = self.ids[start:start + len_t].copy()
		q_ids[2] = q_ids[0]
		vec = self.E[q_ids] + noise * rng.standard_normal((len_t, self.d)).astype(np.float32)
		vec[2] = vec[0]
		q_ids[4] = -1
		vec[4] = rng.standard_normal(self.d).astype(np.float32)
		return q_ids.astype(np.int32), synth.to_bf16_bits(synth.normalize_rows(vec))


def chain_for(name, oracle, case, Qb):
	"""the operators of chain `name` for this query: (b)'s threshold sits in the widest gap of the cells that reach it (the condition on
	the inputs of a chain with a Threshold: asserted, never skipped)"""
	if name != "b":
		return sc.chain(name)
	raw = sc.raw_cosine(oracle, case.Eb, Qb)
	return sc.chain("b", sc.pick_threshold(sc.chain("a"), raw))


def reference(oracle, case, q_ids, Qb, ops, **kw):
	T, raw, _ = sc.chain_table(oracle, case.Eb, Qb, q_ids, ops)
	ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=case.d, sent_off=case.off, Q=Qb, S_rows=[T[case.ids]], **kw)
	return ref, T, raw


def check_alignment(oracle, case, c, q_ids, Qb, ops, loc, ms, gs, gt, k=9):
	"""with and without tracebacks: ids, scores, mappings and the edges' similarities are the oracle's, bit for bit"""
	kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=k, min_score=ms)
	ref, T, raw = reference(oracle, case, q_ids, Qb, ops, **kw)
	assert len(ref["score"]) > 0
	got = c.query(Qb, q_token_ids=q_ids, q_normalize=False, **kw)
	assert_same_results(got.trimmed(), ref, exact=True)
	for i in range(got.n):
		a = int(case.off[int(got.sentence[i])])
		for j in range(len(q_ids)):
			m = int(got.mapping[i, j])
			if m >= 0:
				want = T[case.ids[a + m], j]
				assert got.edge_sim[i, j].view(np.uint32) == want.view(np.uint32), (i, j, got.edge_sim[i, j], want)
	noflow = c.query(Qb, q_token_ids=q_ids, q_normalize=False, want_flow=False, **kw)
	assert_same_results(noflow.trimmed(), ref, check_mapping=False, exact=True)
	return got, T, raw


@pytest.fixture(scope="module")
def case_a(hip):
	case = Case(hip, V=500, d=64, n=350, lo=3, hi=30)
	yield case
	case.c.close()


@pytest.fixture(scope="module")
def case_b(hip):
	case = Case(hip, V=37, d=100, n=320, lo=3, hi=30, seed=11)
	yield case
	case.c.close()


@pytest.mark.parametrize("len_t", [7, 16, 17, 32, 40, 70])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_alignments_under_a_chain_are_the_oracles(hip, oracle, case_a, case_b, name, len_t):
	"""every route with a scoring kernel and a restatement site of its own (fused, vk_score32, wide, vk_longq), all three localities,
	linear / affine / table gaps; V = 500 with d = 64 and V = 37 (a partial last vocabulary tile) with d = 100 (a feature tail)"""
	for case in (case_a, case_b):
		q_ids, Qb = case.query(len_t, seed=ord(name))
		ops = chain_for(name, oracle, case, Qb)
		case.c.set_sim_ops(ops)
		for gap in ("linear", "affine", "exp5"):
			gs, gt = gaps(gap, case.longest)
			for loc, ms in LOCALITIES:
				check_alignment(oracle, case, case.c, q_ids, Qb, ops, loc, ms, gs, gt)


@pytest.fixture(scope="module")
def long_cases(hip):
	cases = {600: Case(hip, V=500, d=64, n=300, lo=3, hi=30, extra=(70, 200, 600), seed=13),
		512: Case(hip, V=500, d=64, n=300, lo=3, hi=30, extra=(70, 200, 512), seed=13)}
	yield cases
	for case in cases.values():
		case.c.close()


@pytest.mark.parametrize("len_t", [7, 20, 70])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_long_slices_under_a_chain(hip, oracle, long_cases, name, len_t):
	"""slices of 70, 200 and 600 tokens among the short ones (vk_doc*, the block form of vk_longq); queries of more than 64 tokens
	stop at slices of 512 tokens, so theirs is 512 long"""
	case = long_cases[512 if len_t > 64 else 600]
	q_ids, Qb = case.query(len_t, seed=ord(name) + 1)
	ops = chain_for(name, oracle, case, Qb)
	case.c.set_sim_ops(ops)
	longs = set(range(len(case.off) - 4, len(case.off) - 1))
	seen = set()
	for gap in ("linear", "affine", "exp5"):
		gs, gt = gaps(gap, case.longest)
		for loc, ms in LOCALITIES:
			got, _, _ = check_alignment(oracle, case, case.c, q_ids, Qb, ops, loc, ms, gs, gt, k=12)
			seen |= longs & {int(s) for s in got.sentence[:got.n]}
	assert seen   # a long slice is among the winners somewhere (local alignments favour them)


def test_the_order_of_operations(hip, oracle, case_a):
	"""two facts a wrong order cannot pass, under (a) = (cos + 1) / 2: a slice token that IS a query word reports similarity 1.0, not
	0.5 + eps (the rewrite runs after the chain), and cells of negative cosine are positive (the chain runs before the clip)"""
	case = case_a
	q_ids, Qb = case.query(7, seed=3)
	ops = sc.chain("a")
	case.c.set_sim_ops(ops)
	T, raw, mod = sc.chain_table(oracle, case.Eb, Qb, q_ids, ops)
	own, negative = 0, 0
	for loc, ms in LOCALITIES:
		got = case.c.query(Qb, q_token_ids=q_ids, q_normalize=False, locality=loc, gap_s=0.05, gap_t=0.05, max_matches=9, min_score=ms, want_rows=True)
		for i in range(got.n):
			s = int(got.sentence[i])
			a, b = int(case.off[s]), int(case.off[s + 1])
			rows = got.sim_rows[i, :b - a, :7]
			assert (rows.view(np.uint32) == T[case.ids[a:b]].view(np.uint32)).all()
			neg = raw[case.ids[a:b]] < 0
			negative += int(neg.sum())
			assert (rows[neg & ~sc.rewrite_mask(case.V, q_ids)[case.ids[a:b]]] > 0).all()
			for j in range(7):
				m = int(got.mapping[i, j])
				if m >= 0 and case.ids[a + m] == q_ids[j]:
					own += 1
					assert got.edge_sim[i, j] == np.float32(1.0)
					assert mod[q_ids[j], j] < 1.0     # what the chain alone leaves of the cell: the noisy copy's cosine, halved towards 1
	assert own >= 3 and negative >= 20


# ---- transports

def transport_case(hip, oracle):
	V, d = 500, 64
	st = synth.make_static_corpus(350, 3, 30, V, d, seed=23)
	rng = np.random.default_rng(24)
	E = (st["E"] * rng.lognormal(0, 0.3, size=(V, 1))).astype(np.float32)
	Eb, emag = oracle.normalize_rows_bf16(E)
	c = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=d, n_tokens=len(st["tok_id"]), n_sentences=350, vocab_size=V, keep_magnitudes=True)
	c.append_vectors(E, normalize=True)
	c.set_token_ids(st["tok_id"])
	c.set_sentences(st["sent_off"])
	c.finalize()
	return c, E, Eb, emag, st["tok_id"], st["sent_off"]


def rank(values, k, min_score):
	"""the oracle's result set: scores above min_score, best first, the later slice first among equals (result_set.h:32-93)"""
	idx = [s for s in range(len(values)) if values[s] > min_score]
	idx.sort(key=lambda s: (-float(values[s]), -s))
	idx = idx[:k]
	return dict(score=np.asarray([values[s] for s in idx], np.float32), sentence=np.asarray(idx, np.int64))


FORMS = {
	"rwmd 1:1": ("rwmd", dict(rwmd=(True, True, True))),
	"rwmd 1:n": ("rwmd", dict(rwmd=(False, True, True))),
	"wmd": ("rwmd", dict(rwmd=(False, False, True), wmd_full=True)),
	"wrd": ("wrd", dict(wrd_normalize=True)),
}


@pytest.mark.parametrize("len_t", [7, 20])
@pytest.mark.parametrize("name", ["a", "b"])
def test_transports_under_a_chain(hip, oracle, name, len_t):
	c, E, Eb, emag, ids, off = transport_case(hip, oracle)
	rng = np.random.default_rng(len_t + ord(name))
	start = int(rng.integers(0, len(ids) - len_t))
	q_ids = ids[start:start + len_t].astype(np.int32).copy()
	q_ids[2] = q_ids[0]
	# the vocabulary's own vectors, as the reference's queries have them: upstream writes a distance of its joint vocabulary twice where
	# both documents hold both words (wmd.h:121-133), and the two writes agree because cos(u, v) = cos(v, u) bit for bit
	qv = E[q_ids].astype(np.float32)
	q_ids[4] = -1
	qv[4] = rng.standard_normal(E.shape[1]).astype(np.float32)
	Qb, qmag = oracle.normalize_rows_bf16(qv)
	own = sc.rewrite_mask(len(Eb), q_ids)   # a word against itself may reach 1.0: those cells are rewritten to 1 anyway
	if name == "b":
		ops = sc.chain("b", sc.pick_threshold(sc.chain("a"), sc.raw_cosine(oracle, Eb, Qb, own)))
	else:
		ops = sc.chain("a")
	c.set_sim_ops(ops)
	T, _, _ = sc.chain_table(oracle, Eb, Qb, q_ids, ops, strict=False)
	n = len(off) - 1
	for form, (alg, kw) in FORMS.items():
		values = np.empty(n, np.float32)
		for s in range(n):
			a, b = int(off[s]), int(off[s + 1])
			S = T[ids[a:b]]
			if alg == "wrd":
				raw = oracle.wrd(S, emag[ids[a:b]], qmag, normalize_magnitudes=True)
			elif kw.get("wmd_full"):
				raw = oracle.wmd(S, ids[a:b], q_ids, relaxed=False, injective=kw["rwmd"][0], symmetric=kw["rwmd"][1], normalize_bow=kw["rwmd"][2])
			else:
				raw = oracle.rwmd(S, ids[a:b], q_ids, injective=kw["rwmd"][0], symmetric=kw["rwmd"][1], normalize_bow=kw["rwmd"][2])
			values[s] = oracle.score(raw, len_t, len_t, 0.0, 1.0)
		ref = rank(values, 10, 0.0)
		h_alg = hip.VK_ALG_WRD if alg == "wrd" else hip.VK_ALG_RWMD
		got = c.query(qv, q_token_ids=q_ids, algorithm=h_alg, q_normalize=True, max_matches=10, min_score=0.0, want_flow=False, **kw)
		assert_same_results(got.trimmed(), ref, check_mapping=False, score_tol=2e-5, tie_tol=2e-5)
		if form == "rwmd 1:1":
			# with the winners' similarity rows the host restates the scores from canonical rows (vk_transport_host.h): the oracle's floats
			rows = c.query(qv, q_token_ids=q_ids, algorithm=h_alg, q_normalize=True, max_matches=10, min_score=0.0, want_flow=True, **kw)
			assert rows.sim_rows is not None
			assert_same_results(rows.trimmed(), ref, check_mapping=False, exact=True)
			for i in range(rows.n):
				a, b = int(off[int(rows.sentence[i])]), int(off[int(rows.sentence[i]) + 1])
				assert (rows.sim_rows[i, :b - a, :len_t].view(np.uint32) == T[ids[a:b]].view(np.uint32)).all()
	c.close()


# ---- powf / expf

@pytest.mark.parametrize("len_t", [7, 20, 70])
@pytest.mark.parametrize("name", ["e", "f"])
def test_transcendental_chains_within_the_transport_tolerance(hip, oracle, case_a, name, len_t):
	"""device powf / expf and numpy's differ by a few ulp per cell: below 1e-6 on a score normalised by len_t.  A cell off by an ulp can
	flip a tie of the traceback: no mapping check"""
	case = case_a
	q_ids, Qb = case.query(len_t, seed=ord(name))
	ops = sc.chain(name)
	case.c.set_sim_ops(ops)
	for gap in ("linear", "exp5"):
		gs, gt = gaps(gap, case.longest)
		for loc, ms in LOCALITIES:
			kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=9, min_score=ms)
			ref, _, _ = reference(oracle, case, q_ids, Qb, ops, **kw)
			got = case.c.query(Qb, q_token_ids=q_ids, q_normalize=False, **kw)
			assert_same_results(got.trimmed(), ref, check_mapping=False, exact=False, score_tol=2e-5, tie_tol=2e-5)


# ---- the chain is state of the handle

def same(a, b):
	assert a.n == b.n
	for f in ("score", "raw_score", "sentence", "mapping", "edge_sim"):
		x, y = getattr(a, f)[:a.n], getattr(b, f)[:b.n]
		assert (x.view(np.uint32) == y.view(np.uint32)).all() if x.dtype == np.float32 else (x == y).all(), f


def test_views_filters_clearing_and_batches_carry_the_chain(hip, oracle, case_a):
	case = case_a
	c = case.c
	ops = sc.chain("a")
	kw = dict(q_normalize=False, locality=0, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=0.0)
	q_ids, Qb = case.query(7, seed=9)
	c.set_sim_ops([])
	plain = c.query(Qb, q_token_ids=q_ids, **kw)
	c.set_sim_ops(ops)
	owner = c.query(Qb, q_token_ids=q_ids, **kw)
	ref, _, _ = reference(oracle, case, q_ids, Qb, ops, locality=0, gap_s=0.1, gap_t=0.05, max_matches=9, min_score=0.0)
	assert_same_results(owner.trimmed(), ref, exact=True)
	assert not (owner.score[:owner.n] == plain.score[:plain.n]).all()
	# a view and a filtered corpus made after set_sim_ops: the owner's results (the filter drops nothing: no codes were set)
	view = c.view()
	same(view.query(Qb, q_token_ids=q_ids, **kw), owner)
	filt = c.filtered(0, 0)
	same(filt.query(Qb, q_token_ids=q_ids, **kw), owner)
	# ... after that each handle is set on its own
	view.set_sim_ops([])
	same(view.query(Qb, q_token_ids=q_ids, **kw), plain)
	same(c.query(Qb, q_token_ids=q_ids, **kw), owner)
	same(filt.query(Qb, q_token_ids=q_ids, **kw), owner)
	view.close()
	filt.close()
	# batches: 9 relaxed-WMD queries (the table of the batch) and 5 alignment queries equal the per-query calls
	qs = [case.query(7 + i % 4, seed=20 + i, noise=0.0) for i in range(9)]
	tkw = dict(algorithm=hip.VK_ALG_RWMD, rwmd=(True, True, True), q_normalize=False, max_matches=10, min_score=0.0)
	outs = c.query_batch([q for _, q in qs], token_ids=[i for i, _ in qs], **tkw)
	for (ids_i, Q_i), out in zip(qs, outs):
		one = c.query(Q_i, q_token_ids=ids_i, **tkw)
		# both restate their winners on the host from canonical rows: the oracle's floats, slice by slice
		T, _, _ = sc.chain_table(oracle, case.Eb, Q_i, ids_i, ops, strict=False)
		values = np.array([oracle.score(oracle.rwmd(T[case.ids[a:b]], case.ids[a:b], ids_i), len(ids_i), len(ids_i), 0.0, 1.0)
			for a, b in zip(case.off[:-1], case.off[1:])], dtype=np.float32)
		ref_t = rank(values, 10, 0.0)
		assert_same_results(out.trimmed(), ref_t, check_mapping=False, exact=True)
		assert_same_results(one.trimmed(), ref_t, check_mapping=False, exact=True)
	qs = [case.query(7 + i % 4, seed=20 + i) for i in range(5)]
	outs = c.query_batch([q for _, q in qs[:5]], token_ids=[i for i, _ in qs[:5]], **kw)
	for (ids_i, Q_i), out in zip(qs[:5], outs):
		same(out, c.query(Q_i, q_token_ids=ids_i, **kw))
	# clearing the chain restores the unmodified results: those of a handle that never had one
	c.set_sim_ops([])
	same(c.query(Qb, q_token_ids=q_ids, **kw), plain)
	fresh = case.handle()
	same(fresh.query(Qb, q_token_ids=q_ids, **kw), plain)
	fresh.close()


def test_what_the_entry_point_refuses(hip, case_a):
	ctx = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=16, n_tokens=32, n_sentences=2)
	ctx.append_vectors(np.random.default_rng(0).standard_normal((32, 16)).astype(np.float32))
	ctx.set_sentences(np.array([0, 16, 32]))

	def status(corpus, ops):
		with pytest.raises(hip.VkError) as e:
			corpus.set_sim_ops(ops)
		return e.value.status, str(e.value)
	st, msg = status(ctx, [(hip.VK_SIMOP_BIAS, 1.0)])
	assert st == hip.VK_ERR_UNSUPPORTED and "CONTEXTUAL" in msg
	ctx.set_sim_ops([])                     # no chain: nothing to refuse, before finalize or after
	ctx.finalize()
	assert status(ctx, [(hip.VK_SIMOP_SCALE, 0.5)])[0] == hip.VK_ERR_UNSUPPORTED
	ctx.set_sim_ops([])
	ctx.close()
	c = case_a.c
	assert status(c, [(hip.VK_SIMOP_BIAS, 0.1)] * 9)[0] == hip.VK_ERR_INVALID
	assert status(c, [(hip.VK_SIMOP_BIAS, 0.1), (6, 1.0)])[0] == hip.VK_ERR_INVALID
	assert status(c, [(-1, 1.0)])[0] == hip.VK_ERR_INVALID
	assert status(c, [(hip.VK_SIMOP_SCALE, float("nan"))])[0] == hip.VK_ERR_INVALID
	assert status(c, [(hip.VK_SIMOP_POWER, float("inf"))])[0] == hip.VK_ERR_INVALID
	c.set_sim_ops([(hip.VK_SIMOP_BIAS, 0.1)] * 8)
	c.set_sim_ops([])


# ---- the Python surface

def test_index_find_under_a_modified_vector_sim(hip):
	"""Index.find / find_many with ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5)) over a StaticEmbedding: the slices, scores and
	flows of the oracle-backed double that states the chain around the oracle (sim_ops_backend.ChainOracleCorpus); a pos_filter gives a
	filtered corpus that carries the chain"""
	rng = np.random.default_rng(5)
	V, d = 300, 48
	E = synth.make_vocab(V, d)
	words = [f"w{i}" for i in range(V)]
	tags = ["NOUN", "VERB", "PRON", "ADJ"]
	docs = []
	for di in range(4):
		sents = [[words[i] for i in synth.zipf_ids(int(rng.integers(4, 30)), V, rng)] for _ in range(40)]
		pos = [[tags[int(w[1:]) % 4] for w in s] for s in sents]
		docs.append(Document(sents, pos=pos, tags=pos, unique_id=f"doc{di}"))
	emb = StaticEmbedding("toy-48", words, E)
	session = Session(docs, embeddings=[emb])
	vsim = ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5))
	sim = OptimizedSpanSim(EmbeddingTokenSim(emb, vsim), alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5)))
	gpu = session.partition("sentence").index(sim)
	cpu = session.partition("sentence").index(sim, corpus_factory=ChainOracleCorpus)
	assert gpu.metric_name == "toy-48-((cosine + 1) * 0.5)"
	doc = session.documents[2]
	st = doc.spans["sentence"]["start"][7]
	texts = [" ".join(doc.tokens[st:st + 5]), "w3 w17 w4 w250 w2 w3", " ".join(doc.tokens[st:st + 22])]

	def key(res):
		return [(m.doc_index, m.slice_id, m.score) for m in res]
	for options in ({}, {"pos_filter": ["PRON"]}):
		for text in texts:
			a = gpu.find(text, n=8, min_score=-100.0, options=options)
			b = cpu.find(text, n=8, min_score=-100.0, options=options)
			assert key(a) == key(b)
			for x, y in zip(a, b):
				assert (x.flow["target"] == y.flow["target"]).all() and (x.flow["dist"] == y.flow["dist"]).all()
		many = gpu.find_many(texts, n=8, min_score=-100.0, options=options)
		assert [key(r) for r in many] == [key(gpu.find(t, n=8, min_score=-100.0, options=options)) for t in texts]
	assert len(gpu._filtered) == 1
	# the plain cosine on the same session scores otherwise: the chain reached the device
	plain = session.partition("sentence").index(OptimizedSpanSim(EmbeddingTokenSim(emb, CosineSim()), alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5))))
	assert key(plain.find(texts[1], n=8, min_score=-100.0)) != key(gpu.find(texts[1], n=8, min_score=-100.0))
	plain.close()
	gpu.close()
