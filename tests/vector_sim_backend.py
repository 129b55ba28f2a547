"""Test doubles for the vector-similarity tests: tests/sim_ops_backend.RecordingCorpus with `set_sim_source` and a record of
`append_vectors`.  SourceOracleCorpus also answers alignment queries over a static corpus under a source that is not the cosine: it
keeps the unmodified rows it is given, states the table in numpy (vector_sim_cases.table) and hands it to the oracle's contextual
route as a caller-supplied similarity matrix."""

import numpy as np

import vector_sim_cases as vc
from fake_backend import _gap
from oracle import vk_oracle as vo
from sim_ops_backend import ChainOracleCorpus, RecordingCorpus
from vectorian_amd import core, synth


class SourceRecordingCorpus(RecordingCorpus):
	def __init__(self, **kw):
		super().__init__(**kw)
		self.sim_source = None
		self._raw = []

	def set_sim_source(self, kind, arg=0.0):
		self.calls.append(("set_sim_source", kind, arg))
		self.sim_source = (int(kind), np.float32(arg))

	def append_vectors(self, rows, normalize=True):
		self.calls.append(("append_vectors",))
		rows = np.ascontiguousarray(rows)
		self._raw.append(synth.bf16_bits_to_f32(rows) if rows.dtype == np.uint16 else rows.astype(np.float32))
		super().append_vectors(rows, normalize=normalize)


class SourceOracleCorpus(SourceRecordingCorpus, ChainOracleCorpus):
	def view(self):
		return self

	def query(self, q_vectors, *, locality=0, gap_s=0.0, gap_t=0.0, algorithm=0, q_token_ids=None, q_normalize=True, max_matches=10,
			min_score=0.0, boost=None, want_flow=True, **rest):
		if self.sim_source is None or self.sim_source[0] == core.VK_SIMSRC_COSINE:
			return super().query(q_vectors, locality=locality, gap_s=gap_s, gap_t=gap_t, algorithm=algorithm, q_token_ids=q_token_ids,
				q_normalize=q_normalize, max_matches=max_matches, min_score=min_score, boost=boost, want_flow=want_flow, **rest)
		assert algorithm == core.VK_ALG_ALIGN and self.layout == core.VK_LAYOUT_STATIC
		assert all(v is None or v is False or v == 0 or k in ("rwmd", "wrd_normalize") for k, v in rest.items()), rest
		q = np.ascontiguousarray(q_vectors)
		q = synth.bf16_bits_to_f32(q) if q.dtype == np.uint16 else q.astype(np.float32)   # the query's rows as given
		ids = np.full(len(q), -1, np.int32) if q_token_ids is None else np.asarray(q_token_ids, dtype=np.int32)
		T, _ = vc.table(np.concatenate(self._raw), q, ids, self.sim_source, self._operators())
		S = T[self._ids]
		r = vo.find(layout=vo.LAYOUT_CONTEXTUAL, d=self.d, sent_off=self._off, sent_end=self._end, Q=synth.to_bf16_bits(q), S_rows=[S], locality=int(locality),
			gap_s=_gap(gap_s, max(core.VK_MAX_SENT_LEN, self._longest()) + 1), gap_t=_gap(gap_t), max_matches=max_matches, min_score=min_score,
			boost=boost, want_all_scores=True)
		self._all = np.array(r["all_scores"], dtype=np.float32)
		top = core.TopK(max_matches, len(q))
		n = top.n = len(r["score"])
		top.score[:n], top.raw_score[:n], top.sentence[:n], top.mapping[:n] = r["score"], r["raw"], r["sentence"], r["mapping"]
		for i in range(n):
			a = int(self._off[int(r["sentence"][i])])
			for j in np.nonzero(r["mapping"][i] >= 0)[0]:
				top.edge_sim[i, j] = S[a + int(r["mapping"][i][j])][j]
		return top
