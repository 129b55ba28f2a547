"""-m gpu: queries of 65 .. 512 tokens (vk_longq_kernel, vk_longq_blocks_kernel) under every form of the gap costs, under exact ties,
with more winners than traceback workgroups and on both sides of the LDS / scratch switch of the general-gap matrix.  The inputs and
what they are good for: tests/long_query_cases.py, proved on the oracle by tests/test_long_query_cases_host.py.

Exact corpora (0 / 1 similarities, dyadic costs): ids, scores, mappings, edge similarities AND the scoring pass -- the score of every
slice, the aligner scores of the run without tracebacks -- equal the oracle's with ==.  Float corpora: the pattern of
test_gpu_long_query_long_slices.py::check_contextual, the score vector within 1e-4."""

import ctypes as C

import numpy as np
import pytest

from vectorian_amd import alignment, synth
from vectorian_amd.corpus import Corpus, Document
from vectorian_amd.embedding import StaticEmbedding
from vectorian_amd.session import Session
from vectorian_amd.sim import CosineSim, EmbeddingTokenSim, OptimizedSpanSim

import long_query_cases as L
from fake_backend import OracleCorpus
from helpers import assert_same_results
from test_gpu_long_query_long_slices import Seen, contextual_handle, mixed_corpus

pytestmark = pytest.mark.gpu


def bits(a):
	return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. exact corpora ------------------------------------------------------------------------------------------------------------

LAYOUTS = ("static", "contextual64", "contextual300")


@pytest.fixture(scope="module")
def exact_handles(hip):
	"""the exact corpora (with and without slices of more than 64 tokens) in the static layout, the contextual one at d = 64 and d = 300 (the QFrag<10, true> fill), and with fp32
	rows: {(stream, layout): (handle, rows of the query's tokens)}"""
	handles = {}
	for stream in L.STREAMS:
		c = L.corpus_of(stream)
		n_tok, n = len(c["ids"]), len(c["lens"])
		E64, E300 = L.one_hot(64), L.one_hot(300)
		h = hip.Corpus(layout=hip.VK_LAYOUT_STATIC, d=64, n_tokens=n_tok, n_sentences=n, vocab_size=L.V)
		h.append_vectors(synth.to_bf16_bits(E64), normalize=False)
		h.set_token_ids(c["ids"])
		h.set_sentences(c["sent_off"])
		h.finalize()
		handles[(stream, "static")] = (h, synth.to_bf16_bits(E64))
		for name, E in (("contextual64", E64), ("contextual300", E300)):
			handles[(stream, name)] = (contextual_handle(hip, c, synth.to_bf16_bits(E[c["ids"]])), synth.to_bf16_bits(E))
		handles[(stream, "f32")] = (contextual_handle(hip, c, np.ascontiguousarray(E64[c["ids"]]), precision="f32"), E64)
	yield handles
	for h, _ in handles.values():
		h.close()


def check_exact(handles, oracle, layout, name, loc, len_t, stream, seen):
	"""one run of the plan on one layout against the oracle's one answer: everything with =="""
	c = L.corpus_of(stream)
	lens, off = c["lens"], c["sent_off"]
	s = L.gap_settings(len_t)[name]
	ref = L.oracle_exact(oracle, stream, name, loc, len_t)
	q_ids = L.exact_query(stream, len_t, L.query_place(stream, loc))
	h, rows = handles[(stream, layout)]
	kw = dict(q_normalize=False, locality=loc, gap_s=s.gap_s, gap_t=s.gap_t, max_matches=L.EXACT_MATCHES, min_score=L.min_score_of(loc))
	if layout == "static":
		kw["q_token_ids"] = q_ids
	where = (layout, name, loc, len_t, stream)
	got = h.query(rows[q_ids], **kw)
	assert_same_results(got.trimmed(), ref)
	assert (bits(got.raw_score[:got.n]) == bits(ref["raw"])).all(), where
	# the scoring pass: the score of EVERY slice is raw / len_t, the division the oracle makes -- no tolerance
	every = c_scores = h.last_scores()
	live = lens > 0
	want = np.asarray(ref["all_scores"], dtype=np.float32)
	assert (every[live] == want[live]).all(), (where, np.nonzero(live & (every != want))[0], every[live & (every != want)], want[live & (every != want)])
	assert np.isneginf(every[~live]).all()
	# ... and times len_t the oracle's aligner score again, wherever the oracle's own product is exact
	back = np.float32(len_t) * np.asarray(ref["score"], dtype=np.float32) == np.asarray(ref["raw"], dtype=np.float32)
	at = np.asarray(ref["sentence"], dtype=np.int64)[back]
	assert (np.float32(len_t) * c_scores[at] == np.asarray(ref["raw"], dtype=np.float32)[back]).all(), where
	seen["product"] += int(back.sum())
	for i in range(got.n):   # the edges: 1 where the words are one word, else 0
		sl = int(got.sentence[i])
		S = L.sim01(c["ids"][off[sl]:off[sl + 1]], q_ids)
		j = np.nonzero(got.mapping[i] >= 0)[0]
		assert (got.edge_sim[i, j] == S[got.mapping[i, j], j]).all(), where
	seen["flow"].note(lens, got)
	# without tracebacks: the result of the scoring pass alone, not retraced
	noflow = h.query(rows[q_ids], want_flow=False, **kw)
	assert_same_results(noflow.trimmed(), ref, check_mapping=False, exact=True)
	assert (bits(noflow.raw_score[:noflow.n]) == bits(ref["raw"])).all(), where
	if stream.startswith("planted") and loc != L.GLOBAL:
		# the triples: the start cell of "both" is that of "first only" (lanes, blocks, adjacent blocks); whichever of them are among the winners
		by_slice = {int(sl): i for i, sl in enumerate(got.sentence[:got.n])}
		for triple, (both, first, second) in c["triples"].items():
			if both in by_slice and first in by_slice:
				assert (got.mapping[by_slice[both]] == got.mapping[by_slice[first]]).all(), (where, triple)
				seen["triples"].add(triple)


@pytest.mark.parametrize("name", L.SETTINGS)
def test_exact_corpora(hip, oracle, exact_handles, name):
	"""every locality under this setting, the query length and the stream in rotation (long_query_cases.exact_plan), on the static
	layout and the contextual one at d = 64 and d = 300"""
	seen = dict(flow=Seen(), product=0, triples=set())
	runs = [r for r in L.exact_plan() if r[0] == name]
	assert {r[1] for r in runs} == {L.LOCAL, L.GLOBAL, L.SEMIGLOBAL}
	for layout in LAYOUTS:
		for run in runs:
			check_exact(exact_handles, oracle, layout, *run, seen)
	assert seen["flow"].long_winner and seen["flow"].short_beside_long, vars(seen["flow"])
	assert seen["product"] > 0 and seen["triples"] == set(L.TRIPLES) | set(L.SHORT_TRIPLES), seen


@pytest.mark.parametrize("name", L.CONCAVE_SETTINGS)
def test_exact_corpora_concave_tails(hip, oracle, exact_handles, name):
	"""tails of 2, 8, 9 and 10 under tables whose one gap no two gaps equal (long_query_cases.csat), GLOBAL: a candidate that the
	running maximum of the tail misses shows in the score"""
	seen = dict(flow=Seen(), product=0, triples=set())
	runs = [r for r in L.exact_plan() if r[0] == name]
	assert {r[3] for r in runs} == {"shared", "shared64", "planted"}
	for layout in LAYOUTS:
		for run in runs:
			check_exact(exact_handles, oracle, layout, *run, seen)
	assert seen["flow"].long_winner and seen["product"] > 0, seen


@pytest.mark.parametrize("name", ["lin_asym", "aff0", "sat9"])
def test_exact_corpora_f32_rows(hip, oracle, exact_handles, name):
	"""one setting per gap form on fp32 rows (v_mfma_f32_16x16x4_f32 tiles)"""
	seen = dict(flow=Seen(), product=0, triples=set())
	for run in [r for r in L.exact_plan() if r[0] == name]:
		check_exact(exact_handles, oracle, "f32", *run, seen)
	assert seen["flow"].long_winner and seen["product"] > 0, seen


# ---- 2. float corpora ------------------------------------------------------------------------------------------------------------

MEASURED = {}   # per case family, the largest |last_scores() - oracle| met (printed; DESIGN 7.5 records it)


def check_float(oracle, c, corpus, Xb, Qb, gs, gt, loc, family, seen=None, max_matches=9):
	"""check_contextual's pattern under given gap costs and one locality"""
	off, lens = corpus["sent_off"], corpus["lens"]
	n = len(lens)
	boost = (np.random.default_rng(len(Qb)).uniform(0.5, 1.0, size=n) * np.where(lens <= 64, 4.0, 1.0)).astype(np.float32)
	kw = dict(locality=loc, gap_s=gs, gap_t=gt, max_matches=max_matches, min_score=L.min_score_of(loc), boost=boost if loc == L.SEMIGLOBAL else None)
	ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=Xb.shape[1], sent_off=off, X=Xb, Q=Qb, want_all_scores=True, n_threads=8, **kw)
	got = c.query(Qb, q_normalize=False, **kw)
	assert_same_results(got.trimmed(), ref)
	every = c.last_scores()
	err = float(np.abs(every[lens > 0].astype(np.float64) - np.asarray(ref["all_scores"], dtype=np.float64)[lens > 0]).max())
	MEASURED[family] = max(MEASURED.get(family, 0.0), err)
	print(f"{family}: max |last_scores() - oracle| = {err:.3e} (so far {MEASURED[family]:.3e})")
	np.testing.assert_allclose(every[lens > 0], np.asarray(ref["all_scores"])[lens > 0], atol=1e-4)
	assert np.isneginf(every[lens == 0]).all()
	for i in range(got.n):   # edge similarities of the matched pairs
		sl = int(got.sentence[i])
		S = oracle.sim_bf16(Xb[off[sl]:off[sl + 1]], Qb)
		for j in np.nonzero(got.mapping[i] >= 0)[0]:
			assert abs(got.edge_sim[i, j] - S[int(got.mapping[i, j]), j]) < 2e-6
	if seen is not None:
		seen.note(lens, got)
	noflow = c.query(Qb, q_normalize=False, want_flow=False, **kw)
	assert_same_results(noflow.trimmed(), ref, check_mapping=False, score_tol=1e-4, tie_tol=1e-4)


@pytest.mark.parametrize("d,len_t", L.FLOAT_CASES)
def test_float_corpora(hip, oracle, d, len_t):
	"""0.1 sqrt(k), min(0.1 k, 0.1 c) and sqrt against sat9 over mixed_corpus, queries of 80 and 200 tokens"""
	corpus, Xb, Qb = L.float_case(d, len_t)
	c = contextual_handle(hip, corpus, Xb)
	seen = Seen()
	S = L.float_settings()
	for d_, len_t_, name, loc in L.float_plan():
		if (d_, len_t_) == (d, len_t):
			check_float(oracle, c, corpus, Xb, Qb, S[name].gap_s, S[name].gap_t, loc, f"float corpora, {'tail' if S[name].tail else 'no tail'}, len_t {len_t}", seen)
	assert seen.long_winner and seen.short_beside_long, vars(seen)
	c.close()


# ---- 3. the LDS / scratch switch of the general-gap matrix --------------------------------------------------------------------------

@pytest.mark.parametrize("max_len", [64, 32])
def test_matrix_in_lds_and_just_outside(hip, oracle, max_len):
	"""the last query length whose matrix H[v][lane] the scoring pass keeps in LDS behind the strip, and the first whose matrix goes to
	the scratch region, as the library itself reports them for this corpus's stride"""
	lib = hip.lib()
	lib.vk_longq_hm_in_lds.restype = C.c_int32
	lib.vk_longq_hm_in_lds.argtypes = [C.c_int32, C.c_int32]
	inside = [lt for lt in range(65, hip.VK_MAX_LONG_QUERY_LEN + 1) if lib.vk_longq_hm_in_lds(lt, max_len) == 1]
	assert inside and inside == list(range(65, inside[-1] + 1)) and inside[-1] < hip.VK_MAX_LONG_QUERY_LEN
	last_in, first_out = inside[-1], inside[-1] + 1
	print(f"longest slice {max_len}: the matrix is in LDS up to len_t = {last_in}, in scratch from {first_out}")
	corpus = synth.make_contextual_corpus(90, 0, max_len, 600, 64, seed=max_len)
	corpus["lens"] = np.diff(corpus["sent_off"])
	assert int(corpus["lens"].max()) == max_len
	Xb = synth.to_bf16_bits(synth.normalize_rows(corpus["X"]))
	c = contextual_handle(hip, corpus, Xb)
	rng = np.random.default_rng(max_len)
	S = L.float_settings()
	for len_t, route in ((last_in, 1), (first_out, 0)):
		assert lib.vk_longq_hm_in_lds(len_t, max_len) == route
		toks = (int(corpus["sent_off"][20]) + np.arange(len_t)) % int(corpus["sent_off"][-1])
		Qb = synth.to_bf16_bits(synth.normalize_rows(corpus["X"][toks] + 0.3 * rng.standard_normal((len_t, 64)).astype(np.float32)))
		for name in ("fsat9", "fsqrt"):
			for loc in (L.LOCAL, L.GLOBAL):
				check_float(oracle, c, corpus, Xb, Qb, S[name].gap_s, S[name].gap_t, loc, f"matrix {'in LDS' if route else 'in scratch'}, longest slice {max_len}")
	c.close()


# ---- 4. more winners than traceback workgroups ---------------------------------------------------------------------------------------

def many_winners(hip, oracle, corpus, max_matches, seed):
	lens, off = corpus["lens"], corpus["sent_off"]
	Xb = synth.to_bf16_bits(synth.normalize_rows(corpus["X"]))
	c = contextual_handle(hip, corpus, Xb)
	rng = np.random.default_rng(seed)
	toks = (int(off[len(lens) // 2]) + np.arange(65)) % int(off[-1])
	Qb = synth.to_bf16_bits(synth.normalize_rows(corpus["X"][toks] + 0.3 * rng.standard_normal((65, Xb.shape[1])).astype(np.float32)))
	S = L.gap_settings(65)
	for name in ("lin_asym", "sat9"):
		kw = dict(locality=L.GLOBAL, gap_s=S[name].gap_s, gap_t=S[name].gap_t, max_matches=max_matches, min_score=-1e9)
		ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, d=Xb.shape[1], sent_off=off, X=Xb, Q=Qb, n_threads=8, **kw)
		got = c.query(Qb, q_normalize=False, **kw)
		assert got.n == len(ref["score"]) == min(max_matches, int((lens > 0).sum()))
		t = got.trimmed()
		# the k boundary: the candidates are the min(k + 8, 1024) best of the scoring pass -- with no margin left at k = 1024 a slice the
		# oracle ranks last may give way to its neighbour (assert_same_results' boundary rule); everything else is the oracle's, bit for bit
		assert_same_results(t, ref, exact=False, check_mapping=True, score_tol=1e-6)
		same = np.asarray(t["sentence"]) == np.asarray(ref["sentence"])
		assert same.sum() >= got.n - 8 and (bits(t["score"])[same] == bits(ref["score"])[same]).all()
		if max_matches + 8 <= hip.VK_MAX_MATCHES:
			assert_same_results(t, ref)
	c.close()
	return Qb


def test_more_winners_than_workgroups(hip, oracle):
	"""300 matches over a corpus with slices of up to 512 tokens: the block form's traceback launch has fewer workgroups than winners,
	so a workgroup restates several winners in one scratch region (matrix, records, unmodified similarities), and the winners are
	selected by select_blocks (more than 64)"""
	lib = hip.lib()
	lib.vk_longq_blocks_grid.restype = C.c_int32
	lib.vk_longq_blocks_grid.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]
	corpus = mixed_corpus(64, n_short=300)
	assert (corpus["lens"] > 0).sum() >= 308
	for gap_mode in (0, 2):
		assert lib.vk_longq_blocks_grid(65, int(corpus["lens"].max()), gap_mode, 308, 308) < 308
	many_winners(hip, oracle, corpus, 300, seed=1)


@pytest.mark.parametrize("max_matches", [300, 1024])
def test_hundreds_of_winners_over_short_slices(hip, oracle, max_matches):
	"""the same over slices of at most 64 tokens (vk_longq_kernel's tracebacks: a workgroup per winner), 300 and 1,024 of 1,100"""
	corpus = synth.make_contextual_corpus(1100, 1, 64, 600, 64, seed=3)
	corpus["lens"] = np.diff(corpus["sent_off"])
	many_winners(hip, oracle, corpus, max_matches, seed=2)


# ---- 5. the operator surface -----------------------------------------------------------------------------------------------------------

def test_through_session_the_same_words_twice(hip):
	"""a sentence of 200 tokens that is one passage of 100 tokens twice -- the same 12 words twice, 100 tokens apart, in the same
	surroundings, so that whatever aligns with the first aligns as well with the second -- and a 90-token paragraph that quotes them:
	Index.find against the oracle-backed double"""
	rng = np.random.default_rng(21)
	Vn, d = 400, 48
	E = synth.make_vocab(Vn, d)
	words = [f"w{i}" for i in range(Vn)]
	docs = []
	for di in range(3):
		sents = [[words[i] for i in synth.zipf_ids(int(n), Vn, rng)] for n in rng.integers(4, 41, size=12)]
		if di == 1:
			passage = [words[i] for i in synth.zipf_ids(100, Vn, rng)]
			sents[5] = passage + passage
			sents[9] = [words[i] for i in synth.zipf_ids(70, Vn, rng)]
		docs.append(Document(sents, unique_id=f"doc{di}"))
	emb = StaticEmbedding("toy-48", words, E)
	session = Session(Corpus(docs), embeddings=[emb])
	twelve = passage[32:44]
	paragraph = [words[i] for i in synth.zipf_ids(90, Vn, rng)]
	paragraph[30:42] = twelve
	text = " ".join(paragraph)
	# a stiff linear cost: the best alignment stays inside the first copy of the passage, so the same alignment 100 tokens further on
	# scores the same and the first one is to be stated; the smooth table: general gaps through the same surface
	for optimizer, tie in ((alignment.LocalAlignment(gap=alignment.LinearGapCost(0.6)), True), (alignment.LocalAlignment(gap=alignment.smooth_gap_cost(5)), False)):
		sim = OptimizedSpanSim(EmbeddingTokenSim(emb, CosineSim()), optimizer)
		gpu = session.partition("sentence").index(sim)
		cpu = session.partition("sentence").index(sim, corpus_factory=OracleCorpus)
		a = gpu.find(text, n=5, min_score=-100.0)
		b = cpu.find(text, n=5, min_score=-100.0)
		assert len(a) == len(b) == 5
		assert [(m.doc_index, m.slice_id) for m in a] == [(m.doc_index, m.slice_id) for m in b]
		assert [m.score for m in a] == [m.score for m in b]
		for x, y in zip(a, b):
			assert (x.flow["target"] == y.flow["target"]).all()
			assert (x.flow["dist"] == y.flow["dist"]).all()
			assert x.to_json() == y.to_json()
		assert b[0].doc_index == 1 and b[0]._len_s == 200 and a[0]._len_s == 200
		if tie:
			target = np.asarray(b[0].flow["target"])
			assert (target[30:42] == np.arange(32, 44)).all() and target.max() < 100, target
		gpu.close()
		cpu.close()
