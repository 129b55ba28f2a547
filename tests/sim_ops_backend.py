"""Test doubles for the similarity-operator tests: tests/fake_backend.OracleCorpus with `set_sim_ops`.  RecordingCorpus notes the
calls the index makes; ChainOracleCorpus also answers alignment queries over a static bf16 corpus under the chain, through the
oracle's caller-supplied similarity matrix (sim_ops_cases.chain_table; oracle.find(layout=LAYOUT_CONTEXTUAL, S_rows=...))."""

import numpy as np

import sim_ops_cases as sc
from fake_backend import OracleCorpus, _gap
from oracle import vk_oracle as vo
from vectorian_amd import core, synth
from vectorian_amd import kernel as K


class RecordingCorpus(OracleCorpus):
	def __init__(self, **kw):
		super().__init__(**kw)
		self.calls = []
		self.sim_ops = []

	def set_sim_ops(self, ops):
		self.calls.append(("set_sim_ops", [(k, a) for k, a in ops]))
		self.sim_ops = [(int(k), np.float32(a)) for k, a in ops]

	def finalize(self):
		self.calls.append(("finalize",))
		super().finalize()


_OPERATOR = {K.VK_SIMOP_BIAS: K.Bias, K.VK_SIMOP_SCALE: K.Scale, K.VK_SIMOP_THRESHOLD: K.Threshold, K.VK_SIMOP_POWER: K.Power,
	K.VK_SIMOP_RADIAL_BASIS: K.RadialBasis}


class ChainOracleCorpus(RecordingCorpus):
	def _operators(self):
		return [K.DistanceToSimilarity() if k == K.VK_SIMOP_ONE_MINUS else _OPERATOR[k](np.float32(a)) for k, a in self.sim_ops]

	def filtered(self, pos_mask=0, tag_mask=0):
		f = super().filtered(pos_mask, tag_mask)
		g = ChainOracleCorpus(layout=f.layout, d=f.d, n_tokens=f.n_tokens, n_sentences=f.n_sentences, vocab_size=f.vocab_size, precision=f.precision)
		g.__dict__.update({k: v for k, v in f.__dict__.items() if k not in ("calls", "lock")})
		g.sim_ops = list(self.sim_ops)   # a filtered corpus carries its source's chain (vk_corpus_filter)
		return g

	def query(self, q_vectors, *, locality=0, gap_s=0.0, gap_t=0.0, algorithm=0, q_token_ids=None, q_normalize=True, max_matches=10,
			min_score=0.0, boost=None, want_flow=True, **rest):
		if not self.sim_ops:
			return super().query(q_vectors, locality=locality, gap_s=gap_s, gap_t=gap_t, algorithm=algorithm, q_token_ids=q_token_ids,
				q_normalize=q_normalize, max_matches=max_matches, min_score=min_score, boost=boost, want_flow=want_flow, **rest)
		assert algorithm == core.VK_ALG_ALIGN and self.layout == core.VK_LAYOUT_STATIC and self.precision == "bf16"
		assert all(v is None or v is False or v == 0 or k in ("rwmd", "wrd_normalize") for k, v in rest.items()), rest
		q = np.ascontiguousarray(q_vectors)
		q = synth.bf16_bits_to_f32(q) if q.dtype == np.uint16 else q.astype(np.float32)
		Qb = vo.normalize_rows_bf16(q)[0] if q_normalize else synth.to_bf16_bits(q)
		ids = np.full(len(q), -1, np.int32) if q_token_ids is None else np.asarray(q_token_ids, dtype=np.int32)
		T, _, _ = sc.chain_table(vo, self._X, Qb, ids, self._operators(), strict=False)
		S = T[self._ids]
		r = vo.find(layout=vo.LAYOUT_CONTEXTUAL, d=self.d, sent_off=self._off, sent_end=self._end, Q=Qb, S_rows=[S], locality=int(locality),
			gap_s=_gap(gap_s, max(core.VK_MAX_SENT_LEN, self._longest()) + 1), gap_t=_gap(gap_t), max_matches=max_matches, min_score=min_score,
			boost=boost, want_all_scores=True)
		self._all = np.array(r["all_scores"], dtype=np.float32)
		top = core.TopK(max_matches, len(q))
		n = top.n = len(r["score"])
		top.score[:n], top.raw_score[:n], top.sentence[:n], top.mapping[:n] = r["score"], r["raw"], r["sentence"], r["mapping"]
		for i in range(n):
			a = int(self._off[int(r["sentence"][i])])
			for j in np.nonzero(r["mapping"][i] >= 0)[0]:
				top.edge_sim[i, j] = S[a + int(r["mapping"][i][j]), j]
		return top
