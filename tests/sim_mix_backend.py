"""Test doubles for the token-similarity-combinator tests: tests/vector_sim_backend.SourceRecordingCorpus with the four calls of a
mixed handle (set_sim_mix, set_sim_operand, append_operand_vectors, query(q_operand_vectors=...)).  MixOracleCorpus also answers
alignment queries: it keeps every operand's unmodified rows, states each operand's table in numpy (sim_mix_cases.operand_table),
combines them with the reference's own numpy call (vectorian_amd.modifier) and hands the result to the oracle's contextual route as a
caller-supplied similarity matrix."""

import numpy as np

import sim_mix_cases as mc
from fake_backend import _gap
from oracle import vk_oracle as vo
from sim_ops_backend import _OPERATOR
from vector_sim_backend import SourceOracleCorpus, SourceRecordingCorpus
from vectorian_amd import core, synth
from vectorian_amd import kernel as K
from vectorian_amd.sim import ImprovedSqrtCosineSim, PNormDistance


class MixRecordingCorpus(SourceRecordingCorpus):
	def __init__(self, **kw):
		super().__init__(**kw)
		self.sim_mix = None
		self.operand = {}        # i -> (d, source or None, [(kind, float32 arg)])
		self.operand_rows = {}   # i -> [float32 rows as given]
		self.query_operands = []   # per query: the arrays it was given

	def set_sim_mix(self, kind, n_operands, weights=None):
		self.calls.append(("set_sim_mix", kind, n_operands, weights))
		self.sim_mix = (int(kind), int(n_operands), None if weights is None else np.asarray(weights))

	def set_sim_operand(self, i, d, source=None, ops=()):
		self.calls.append(("set_sim_operand", i, d, source, [(k, a) for k, a in ops]))
		self.operand[int(i)] = (int(d), None if source is None else (int(source[0]), np.float32(source[1])), [(int(k), np.float32(a)) for k, a in ops])

	def append_operand_vectors(self, i, rows, normalize=True):
		rows = np.ascontiguousarray(rows)
		self.calls.append(("append_operand_vectors", i, rows.shape, rows.dtype, normalize))
		self.operand_rows.setdefault(int(i), []).append(synth.bf16_bits_to_f32(rows) if rows.dtype == np.uint16 else rows.astype(np.float32))

	def query(self, q_vectors, q_operand_vectors=None, **kw):
		self.query_operands.append(q_operand_vectors)
		return super().query(q_vectors, **kw)

	def query_batch(self, queries, token_ids=None, q_operand_vectors=None, **options):
		"""vk_query_batch's contract: n_queries calls of vk_query, each with its own operand rows"""
		if q_operand_vectors is None:
			return super().query_batch(queries, token_ids=token_ids, **options)
		assert len(q_operand_vectors) == len(queries)
		ids = token_ids if token_ids is not None else [None] * len(queries)
		return [self.query(q, q_operand_vectors=rows, **dict(options, q_token_ids=t)) for q, rows, t in zip(queries, q_operand_vectors, ids)]


def _operators(pairs):
	return [K.DistanceToSimilarity() if k == K.VK_SIMOP_ONE_MINUS else _OPERATOR[k](np.float32(a)) for k, a in pairs]


def _source(pair):
	if pair is None or pair[0] == core.VK_SIMSRC_COSINE:
		return None
	return PNormDistance(float(pair[1])) if pair[0] == core.VK_SIMSRC_PNORM else ImprovedSqrtCosineSim()


class MixOracleCorpus(MixRecordingCorpus, SourceOracleCorpus):
	def filtered(self, pos_mask=0, tag_mask=0):
		f = super().filtered(pos_mask, tag_mask)
		g = MixOracleCorpus(layout=f.layout, d=f.d, n_tokens=f.n_tokens, n_sentences=f.n_sentences, vocab_size=f.vocab_size, precision=f.precision)
		g.__dict__.update({k: v for k, v in f.__dict__.items() if k not in ("calls", "lock")})
		for name in ("sim_mix", "operand", "operand_rows", "sim_source", "_raw"):   # a filtered corpus carries its source's similarity
			setattr(g, name, getattr(self, name))
		g.sim_ops = list(self.sim_ops)
		return g

	def query(self, q_vectors, q_operand_vectors=None, *, locality=0, gap_s=0.0, gap_t=0.0, algorithm=0, q_token_ids=None, q_normalize=True,
			max_matches=10, min_score=0.0, boost=None, want_flow=True, **rest):
		if self.sim_mix is None:
			return SourceOracleCorpus.query(self, q_vectors, locality=locality, gap_s=gap_s, gap_t=gap_t, algorithm=algorithm, q_token_ids=q_token_ids,
				q_normalize=q_normalize, max_matches=max_matches, min_score=min_score, boost=boost, want_flow=want_flow, **rest)
		self.query_operands.append(q_operand_vectors)
		assert algorithm == core.VK_ALG_ALIGN and self.layout == core.VK_LAYOUT_STATIC and self.precision == "bf16" and q_normalize
		assert all(v is None or v is False or v == 0 or k in ("rwmd", "wrd_normalize") for k, v in rest.items()), rest
		kind, n, weights = self.sim_mix
		assert q_operand_vectors is not None and len(q_operand_vectors) == n - 1
		q0 = np.ascontiguousarray(q_vectors)
		q0 = synth.bf16_bits_to_f32(q0) if q0.dtype == np.uint16 else q0.astype(np.float32)
		ids = np.full(len(q0), -1, np.int32) if q_token_ids is None else np.asarray(q_token_ids, dtype=np.int32)
		each = [mc.operand_table(vo, np.concatenate(self._raw), q0, ids, _source(self.sim_source), _operators(self.sim_ops))]
		for i in range(1, n):
			d, source, ops = self.operand[i]
			qi = np.ascontiguousarray(q_operand_vectors[i - 1], dtype=np.float32)
			assert qi.shape == (len(q0), d)
			each.append(mc.operand_table(vo, np.concatenate(self.operand_rows[i]), qi, ids, _source(source), _operators(ops)))
		T = mc.combine(mc.modifier_of((kind, None if weights is None else list(weights)), n), each)
		S = T[self._ids]
		r = vo.find(layout=vo.LAYOUT_CONTEXTUAL, d=self.d, sent_off=self._off, sent_end=self._end, Q=vo.normalize_rows_bf16(q0)[0], S_rows=[S], locality=int(locality),
			gap_s=_gap(gap_s, max(core.VK_MAX_SENT_LEN, self._longest()) + 1), gap_t=_gap(gap_t), max_matches=max_matches, min_score=min_score,
			boost=boost, want_all_scores=True)
		self._all = np.array(r["all_scores"], dtype=np.float32)
		top = core.TopK(max_matches, len(q0))
		k = top.n = len(r["score"])
		top.score[:k], top.raw_score[:k], top.sentence[:k], top.mapping[:k] = r["score"], r["raw"], r["sentence"], r["mapping"]
		for i in range(k):
			a = int(self._off[int(r["sentence"][i])])
			for j in np.nonzero(r["mapping"][i] >= 0)[0]:
				top.edge_sim[i, j] = S[a + int(r["mapping"][i][j])][j]
		return top
