"""What the token-similarity-combinator tests share (CPU and GPU tiers): corpora over several static embeddings of
different widths, the operand combinations, and the reference -- each operand's table stated in numpy (sim_ops_cases.chain_table for a
cosine operand, on the bf16 unit rows; vector_sim_cases.table for a source operand, on the raw rows), the tables combined with the
reference's own numpy call (vectorian_amd.modifier, which mirrors vectorian/sim/modifier.py), and the conditions on the inputs that
every case asserts:
  - at least a third of the combined table's cells lie strictly inside (0, 1);
  - under MAXIMUM every operand supplies the strict maximum in at least a fifth of those cells;
  - (asserted by the tests over the queries of a case) the reference's winners under the combinator differ from its winners under
    operand 0 alone for at least one query -- a kernel that ignored the other operands would fail."""

import numpy as np

import sim_ops_cases as sc
import vector_sim_cases as vc
from vectorian_amd import core, synth
from vectorian_amd.kernel import Bias, DistanceToSimilarity, Power, Scale, Threshold
from vectorian_amd.modifier import MaximumTokenSimilarity, MinimumTokenSimilarity, MixedTokenSimilarity
from vectorian_amd.sim import ImprovedSqrtCosineSim, PNormDistance

# the widths of the operands' embeddings: they differ, and all but the first have a feature tail
WIDTHS = {"two": (64, 100), "wide": (67, 300), "three": (32, 67, 100)}

# the combinators: (kind of vk_corpus_set_sim_mix, weights)
MIXES = {
	"avg-float": (core.VK_SIMMIX_AVERAGE, {2: [0.3, 0.7], 3: [0.5, 0.2, 0.3]}),
	"avg-int": (core.VK_SIMMIX_AVERAGE, {2: [2, 1], 3: [1, 2, 1]}),
	"max": (core.VK_SIMMIX_MAXIMUM, None),
}


# The cases of the GPU tier: name -> (widths, V, slices, operand combination, combinator).  V = 37: a vocabulary of 48 padded rows, a
# partly empty workgroup of the table kernels; 320 .. 350 slices of 3 .. 30 tokens.  cc and pw run under AVERAGE only: one of their
# operands is the larger in (nearly) every cell, which the condition on MAXIMUM rules out.
CASES = {
	"cc-avg-float": ("two", 500, 350, "cc", "avg-float"),
	"cc-avg-int-v37": ("wide", 37, 320, "cc", "avg-int"),
	"aa-max": ("two", 500, 350, "aa", "max"),
	"tp-avg-int": ("two", 500, 340, "tp", "avg-int"),
	"tp-max-v37": ("wide", 37, 320, "tp", "max"),
	"three-max": ("three", 500, 330, "three", "max"),
	"three-avg-float-v37": ("three", 37, 320, "three", "avg-float"),
	"pw-avg-float": ("two", 500, 350, "pw", "avg-float"),
}
QUERY_LENGTHS = (7, 16, 17, 40, 70)   # nine padding columns; one whole tile; two tiles; three; the long-query route
QUERY_SEED = 3


def case(name, extra=()):
	"""(corpus, operand combination, combinator) of a case; extra: the lengths of further, long slices"""
	widths, V, n, combo, mix = CASES[name]
	return Corpus(V, WIDTHS[widths], n, 3, 30, extra=extra, seed=7 + len(name)), combo, mix


class Corpus:
	"""a static corpus over len(dims) embeddings of raw standard_normal rows; operand m's embedding is E[m] (V x dims[m])"""

	def __init__(self, V, dims, n, lo, hi, extra=(), seed=7):
		st = synth.make_static_corpus(n, lo, hi, V, dims[0], seed=seed)
		rng = np.random.default_rng(seed + 100)
		lens = list(np.diff(st["sent_off"])) + list(extra)
		self.ids = np.concatenate([st["tok_id"], synth.zipf_ids(int(sum(extra)), V, rng)]).astype(np.int32)
		self.off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
		self.V, self.dims = V, tuple(dims)
		self.E = [rng.standard_normal((V, d)).astype(np.float32) for d in dims]
		self.longest = int(max(lens))

	def query(self, len_t, seed, noise=0.15):
		"""len_t tokens quoted from the corpus with a repeated word and a word outside the vocabulary (id -1, a vector of its own under
		every embedding), noise on every vector (noise = 0: the vocabulary's own vectors, as transports need them).  Returns the ids
		and one [len_t x d_m] float32 array per operand"""
		rng = np.random.default_rng(1000 * len_t + seed)
		start = int(rng.integers(0, len(self.ids) - len_t))
		q_ids = self.ids[start:start + len_t].copy()
		q_ids[2] = q_ids[0]
		Qs = []
		for E in self.E:
			vec = E[q_ids] + np.float32(noise) * rng.standard_normal((len_t, E.shape[1])).astype(np.float32)
			vec[2] = vec[0]
			vec[4] = rng.standard_normal(E.shape[1]).astype(np.float32)
			Qs.append(np.ascontiguousarray(vec, dtype=np.float32))
		q_ids[4] = -1
		return q_ids.astype(np.int32), Qs


def operands(name, dims):
	"""per operand (source similarity or None for the cosine, operators) of combination `name` over embeddings of these widths.
	  cc     cosine + cosine under (a) = (x + 1) / 2
	  aa     both cosines under (a): comparable cells, for MAXIMUM
	  tp     cosine under (b) -- (a), then Threshold(0.47): on a mixed handle both passes read one cell, so the threshold needs no gap
	         between the cells around it -- + PNormDistance(2) under Scale / DistanceToSimilarity, the median cell near
	         one half (rows and queries are standard normal with noise 0.15: a squared difference has mean 2.02 per feature)
	  pw     cosine under (a) + cosine under Bias(1), Scale(0.5), Power(2.5): powf on the device
	  three  cosine under (a), ImprovedSqrtCosineSim under a Bias, PNormDistance(1) under Scale / DistanceToSimilarity / Bias (a mean
	         absolute difference of 1.122 per feature): three operands whose cells spread alike around one half, for MAXIMUM"""
	a = sc.chain("a")
	if name == "cc":
		return [(None, []), (None, a)]
	if name == "aa":
		return [(None, a), (None, a)]
	if name == "tp":
		return [(None, a + [Threshold(0.47)]), (PNormDistance(2), [Scale(1 / (2 * float(np.sqrt(2.02 * dims[1])))), DistanceToSimilarity()])]
	if name == "pw":
		return [(None, a), (None, a + [Power(2.5)])]
	assert name == "three"
	return [(None, a), (ImprovedSqrtCosineSim(), [Bias(0.073)]), (PNormDistance(1), [Scale(0.9 / (1.122 * dims[2])), DistanceToSimilarity(), Bias(0.4)])]


EXACT = {"cc": True, "aa": True, "tp": True, "pw": False, "three": True}   # operands of exactly rounded operations: ==


def operand_table(vo, E, Q, q_ids, source, ops):
	"""[V x len_t] float32: one operand's table as build_static_similarity_matrix leaves it -- VectorSim, chain, sim[id(t_j)][j] = 1,
	clip.  The cosine runs on the bf16 unit rows (the handle's tiles, the query's tile), a source on the rows as given"""
	if source is None:
		Eb, Qb = vo.normalize_rows_bf16(E)[0], vo.normalize_rows_bf16(Q)[0]
		return sc.chain_table(vo, Eb, Qb, q_ids, ops, strict=False)[0]
	return vc.table(E, Q, q_ids, vc.source_of(source), ops)[0]


def modifier_of(mix, n, metrics=None):
	"""the reference's object for combinator `mix` over n operands"""
	kind, weights = MIXES[mix] if isinstance(mix, str) else mix
	metrics = metrics if metrics is not None else [None] * n
	if kind == core.VK_SIMMIX_AVERAGE:
		return MixedTokenSimilarity(metrics, weights[n] if isinstance(weights, dict) else weights)
	return MaximumTokenSimilarity(metrics)


def combine(modifier, tables):
	"""the reference's own call on the operands' clipped tables (metric/modifier.cpp:56-70: one dict per operand, `out` preallocated)"""
	out = {"similarity": np.empty_like(tables[0])}
	modifier([{"similarity": t} for t in tables], out)
	assert out["similarity"].dtype == np.float32
	return out["similarity"]


def tables(vo, corpus, q_ids, Qs, ops_of, mix):
	"""(combined table, the operands' tables) of a query, with the conditions on the inputs asserted"""
	each = [operand_table(vo, E, Q, q_ids, src, ops) for E, Q, (src, ops) in zip(corpus.E, Qs, ops_of)]
	modifier = modifier_of(mix, len(each))
	T = combine(modifier, each)
	inside = (T > 0) & (T < 1)
	assert inside.mean() >= 1 / 3, inside.mean()
	if isinstance(modifier, MaximumTokenSimilarity):
		stack = np.array(each)
		for m in range(len(each)):
			others = np.delete(stack, m, axis=0).max(axis=0)
			share = float((stack[m] > others)[inside].mean())
			assert share >= 1 / 5, (m, share)
		assert (combine(MinimumTokenSimilarity([None] * len(each)), each) == T).all()   # upstream's "minimum" IS the maximum
	return T, each


def set_up(corpus_handle, mix, dims, ops_of):
	"""the combinator and operands 1 .. on a fresh handle, before its first append (operand 0's source goes through set_sim_source)"""
	kind, weights = MIXES[mix]
	corpus_handle.set_sim_mix(kind, len(dims), None if weights is None else weights[len(dims)])
	for i in range(1, len(dims)):
		src, ops = ops_of[i]
		corpus_handle.set_sim_operand(i, dims[i], None if src is None else vc.source_of(src), sc.pairs(ops))
