"""Similarity operators: the surface of `vectorian.sim` on the hot path.

VectorSim / CosineSim   vectorian/sim/vector.py:17-78
ModifiedVectorSim       vectorian/sim/vector.py:179-200 (its operators: vectorian_amd/kernel.py, re-exported here)
TokenSim / EmbeddingTokenSim   vectorian/sim/token.py:4-44
SpanSim / OptimizedSpanSim     vectorian/sim/span.py:9-71
PNormDistance / EuclideanDistance / ImprovedSqrtCosineSim   vectorian/sim/vector.py:98-167
A ModifiedVectorSim -- a chain of up to 8 operators on the unclipped output of its source -- runs on the device over static
embeddings: `EmbeddingTokenSim(emb, ModifiedVectorSim(CosineSim(), Bias(1), Scale(0.5)))`.  Its source, or the
similarity itself, is CosineSim, PNormDistance or ImprovedSqrtCosineSim (the latter two over static embeddings only, on
the unmodified vectors): `ModifiedVectorSim(PNormDistance(2), Scale(1 / 12), DistanceToSimilarity())`.
TokenSimilarityModifier / MixedTokenSimilarity / MaximumTokenSimilarity / MinimumTokenSimilarity   vectorian/sim/modifier.py
(vectorian_amd/modifier.py, re-exported here): combinators of up to four EmbeddingTokenSims over static embeddings run on the device
(DESIGN 14): `MixedTokenSimilarity([EmbeddingTokenSim(a, CosineSim()), EmbeddingTokenSim(b, CosineSim())], [2, 1])`.
SpanEmbedding / AggregatedSpanEmbedding / EmbeddedSpanSim   vectorian/embedding/span.py:27-93, vectorian/sim/span.py:74-95: one vector
per span, from the caller or -- the mean, minimum or maximum of the span's token vectors -- pooled on the device:
`AggregatedSpanEmbedding(emb, np.mean).to_sentence_sim()`.  The VectorSim of a span index is any of the above, unclipped, over span
vectors of any origin: `emb.to_sentence_sim(ModifiedVectorSim(PNormDistance(2), RadialBasis(0.5)))`.
FuzzyJaccardSim, DirectionalDistance, user-defined VectorSims, chains and combinators over contextual TOKEN embeddings, nested
combinators, UnaryTokenSimilarityModifier and a combinator under WordRotatorsDistance are out of scope and are rejected explicitly
rather than ignored; the tag-weighted variant is a "next" row.
"""

import numpy as np

from vectorian_amd.alignment import ConstantGapCost, LocalAlignment, Optimizer
from vectorian_amd.embedding import AbstractVectors
from vectorian_amd.query import tokenize
from vectorian_amd.kernel import (  # noqa: F401  (the reference's users import the operators next to the similarities)
	Bias, DistanceToSimilarity, Kernel, Power, RadialBasis, Scale, Threshold, UnaryOperator)


class VectorSim:
	"""a scalar similarity in [0, 1] for pairs of vectors (vectorian/sim/vector.py:17-44)"""

	def __call__(self, a: AbstractVectors, b: AbstractVectors, out: np.ndarray):
		self.compute(a, b, out)

	def compute(self, a: AbstractVectors, b: AbstractVectors, out: np.ndarray):
		raise NotImplementedError()

	@property
	def name(self) -> str:
		raise NotImplementedError()


class CosineSim(VectorSim):
	"""cosine of the angle between two vectors (vectorian/sim/vector.py:63-82); negative
	values are clipped to 0 downstream (SimilarityMatrix::clip, metric/metric.h:28-30)"""

	def compute(self, a, b, out):
		np.linalg.multi_dot([a.normalized, b.normalized.T], out=out)

	@property
	def name(self):
		return "cosine"


class ImprovedSqrtCosineSim(VectorSim):
	"""Sohangir & Wang's improved sqrt-cosine on vectors made non-negative by doubling every feature into max(0, x), max(0, -x)
	(vectorian/sim/vector.py:98-132); a pair with a zero vector scores 0"""

	@staticmethod
	def _to_non_negative(x):
		t = np.repeat(x, 2, axis=-1)
		t[:, 1::2] = -t[:, 1::2]
		return np.maximum(0, t)

	def compute(self, a, b, out):
		a_pos = self._to_non_negative(a.unmodified)
		b_pos = self._to_non_negative(b.unmodified)
		num = np.sum(np.sqrt(a_pos[:, np.newaxis] * b_pos[np.newaxis, :]), axis=-1)
		x = np.sqrt(np.sum(a_pos, axis=-1))
		y = np.sqrt(np.sum(b_pos, axis=-1))
		denom = x[:, np.newaxis] * y[np.newaxis, :]
		with np.errstate(divide="ignore", invalid="ignore"):
			out[:, :] = num / denom
		np.nan_to_num(out, copy=False, nan=0)

	@property
	def name(self):
		return "improved-sqrt-cosine"

	@property
	def sim_source(self):
		"""(kind, float32 argument) of vk_corpus_set_sim_source"""
		return 2, np.float32(0)   # core.VK_SIMSRC_SQRT_COSINE


class PNormDistance(VectorSim):
	"""the p-norm of the difference of the unmodified vectors (vectorian/sim/vector.py:135-160).  A DISTANCE: combine it with
	DistanceToSimilarity (or RadialBasis) in a ModifiedVectorSim"""

	def __init__(self, p: float = 2):
		self._p = p

	@property
	def p(self):
		return self._p

	def compute(self, a, b, out):
		d = a.unmodified[:, np.newaxis] - b.unmodified[np.newaxis, :]
		d = np.sum(np.power(np.abs(d), self._p), axis=-1)
		d = np.power(d, 1 / self._p)
		out[:, :] = d  # distance, not a similarity

	@property
	def name(self):
		return f"p-norm({self._p})"

	@property
	def sim_source(self):
		"""(kind, float32 argument) of vk_corpus_set_sim_source"""
		return 1, np.float32(self._p)   # core.VK_SIMSRC_PNORM


class EuclideanDistance(PNormDistance):
	"""PNormDistance(2).  (The reference's class passes a `scale` its base class does not take and cannot be constructed,
	vectorian/sim/vector.py:163-167; this one takes no argument.)"""

	def __init__(self):
		super().__init__(p=2)


class ModifiedVectorSim(VectorSim):
	"""a VectorSim whose output is modified by one or more operators (vectorian/sim/vector.py:179-200)"""

	def __init__(self, source: VectorSim, *operators: UnaryOperator):
		self._source = source
		self._kernel = Kernel(operators)

	@property
	def source(self):
		return self._source

	@property
	def operators(self):
		return self._kernel.operators

	def compute(self, a, b, out):
		self._source(a, b, out)
		self._kernel(out)

	@property
	def name(self):
		return self._kernel.name(self._source.name)


class TokenSim:
	@property
	def is_modifier(self):
		return False

	@property
	def name(self):
		raise NotImplementedError()

	@property
	def embeddings(self):
		raise NotImplementedError()


class EmbeddingTokenSim(TokenSim):
	def __init__(self, embedding, sim: VectorSim):
		self._embedding = embedding
		self._sim = sim

	@property
	def name(self):
		return f"{self._sim.name}[{self._embedding.name}]"

	@property
	def embeddings(self):
		return [self._embedding]

	@property
	def embedding(self):
		return self._embedding

	@property
	def similarity(self):
		return self._sim

	def to_args(self, index):
		return {
			"name": self._embedding.name + "-" + self._sim.name,
			"embedding": self._embedding.name,
			"metric": self._sim
		}


# the combinators of vectorian/sim/modifier.py live in vectorian_amd/modifier.py (which needs TokenSim above) and are re-exported
# here on first use, so that either module may be imported first
_MODIFIERS = ("TokenSimilarityModifier", "UnaryTokenSimilarityModifier", "MixedTokenSimilarity", "ExtremumTokenSimilarity",
	"MaximumTokenSimilarity", "MinimumTokenSimilarity")


def __getattr__(name):
	if name in _MODIFIERS:
		from vectorian_amd import modifier
		return getattr(modifier, name)
	raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class SpanSim:
	def create_index(self, partition, **kwargs):
		raise NotImplementedError()

	def to_args(self, index):
		raise NotImplementedError()


class OptimizedSpanSim(SpanSim):
	def __init__(self, token_sim: TokenSim, optimizer: Optimizer = None, tag_weights: dict = None, **kwargs):
		if not isinstance(token_sim, TokenSim):
			raise TypeError(token_sim)
		if optimizer is None:
			# vectorian/sim/span.py:28-32
			optimizer = LocalAlignment(gap={"s": ConstantGapCost(0), "t": ConstantGapCost(0)})
		if not isinstance(optimizer, Optimizer):
			raise TypeError(optimizer)
		self._token_sim = token_sim
		self._optimizer = optimizer
		self._tag_weights = tag_weights
		self._options = kwargs

	@property
	def token_sim(self):
		return self._token_sim

	@property
	def optimizer(self):
		return self._optimizer

	def create_index(self, partition, **kwargs):
		# the plugin seam: SpanSim.create_index -> Index (vectorian/sim/span.py:50-51).
		# The reference returns BruteForceIndex here; this package returns its MI355X twin.
		from vectorian_amd.index import HipBruteForceIndex
		return HipBruteForceIndex(partition, self, **kwargs)

	def to_args(self, index):
		if not self._tag_weights:
			if self._options:
				raise ValueError(f"illegal option(s): {', '.join(self._options.keys())}")
			return {
				"metric": "alignment-isolated",
				"token_metric": self._token_sim,
				"alignment": self._optimizer.to_args(index.partition)
			}
		else:
			return {
				"metric": "alignment-tag-weighted",
				"token_metric": self._token_sim,
				"alignment": self._optimizer.to_args(index.partition),
				"pos_mismatch_penalty": self._options.get("pos_mismatch_penalty", 0),
				"similarity_threshold": self._options.get("similarity_threshold", 0),
				"tag_weights": self._tag_weights
			}


class SpanEmbedding:
	"""one vector per span (vectorian/embedding/span.py).  The sentence encoders of the reference are out of
	scope; vectors come precomputed, `encode(texts) -> [n x d]` embeds queries."""

	def __init__(self, name, dimension, encode):
		self._name, self._dimension, self._encode = name, int(dimension), encode

	@property
	def name(self):
		return self._name

	@property
	def dimension(self):
		return self._dimension

	def encode(self, texts):
		v = np.ascontiguousarray(self._encode(texts), dtype=np.float32)
		return v.reshape(len(texts), self._dimension)


class AggregatedSpanEmbedding(SpanEmbedding):
	"""the mean, minimum or maximum of a span's token vectors, static or contextual (AggregatedTokenImpl,
	vectorian/embedding/span.py:27-93): `AggregatedSpanEmbedding(emb, np.max).to_sentence_sim()`.  The spans of an index are pooled on
	the device from the token rows the alignment index uses (HipSpanEncoderIndex -> Corpus.append_pooled) -- np.mean,
	np.min and np.max only: there is no other place in this package to pool.  A query is one span and is pooled here, on the host,
	by the reference's own numpy call."""

	_default_functions = {np.mean: "mean", np.min: "min", np.max: "max"}

	def __init__(self, token_embedding, agg=np.mean, agg_name=None, nlp=None):
		try:
			known = AggregatedSpanEmbedding._default_functions.get(agg)
		except TypeError:   # (not hashable)
			known = None
		if known is None:
			raise NotImplementedError(f"{agg}: span vectors are pooled on the device with np.mean, np.min or np.max; there is no CPU path for other aggregates")
		self._token_embedding = token_embedding
		self._agg = agg
		self._agg_name = known if agg_name is None else agg_name
		self._nlp = nlp

	@property
	def name(self):
		return f"aggregated-{self._agg_name}-{self._token_embedding.name}"

	@property
	def dimension(self):
		return self._token_embedding.dimension

	@property
	def token_embedding(self):
		return self._token_embedding

	@property
	def agg(self):
		return self._agg

	def with_nlp(self, nlp):
		"""this embedding with `nlp` as the tokenizer of its queries (an index hands its own on)"""
		return AggregatedSpanEmbedding(self._token_embedding, self._agg, self._agg_name, nlp=nlp)

	def to_sentence_sim(self, vector_sim=None):
		return EmbeddedSpanSim(self, vector_sim)

	def encode(self, texts):
		out = np.full((len(texts), self.dimension), np.nan, dtype=np.float32)   # a text without tokens: the reference's out.fill(np.nan)
		for i, text in enumerate(texts):
			tokens = [t["text"] if isinstance(t, dict) else t for t in tokenize(text, self._nlp)]
			v = self._token_embedding.encode_tokens(tokens).unmodified
			if v.shape[0] > 0:
				out[i, :] = self._agg(v, axis=0)
		return out


class EmbeddedSpanSim(SpanSim):
	"""span similarity by ONE embedding per span (vectorian/sim/span.py:74-95)"""

	def __init__(self, embedding: SpanEmbedding, sim: VectorSim = None):
		if sim is None:
			sim = CosineSim()
		if not isinstance(sim, VectorSim):
			raise TypeError(f"{sim} is expected to be a VectorSim")
		self._embedding = embedding
		self._vector_sim = sim

	@property
	def embedding(self):
		return self._embedding

	@property
	def vector_sim(self):
		return self._vector_sim

	def create_index(self, partition, **kwargs):
		# the reference picks FaissCosineIndex / SpanEncoderIndex here (vectorian/sim/span.py:83-88)
		# (the index resolves the VectorSim -- DESIGN 17 -- or says why it does not run here)
		from vectorian_amd.index import HipSpanEncoderIndex
		return HipSpanEncoderIndex(partition, self._embedding, self, **kwargs)

	def to_args(self, index):
		return None

	@property
	def name(self):
		return "EmbeddedSpanSim"
