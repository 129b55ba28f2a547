"""What the tests of operator chains over contextual corpora share: small corpora on the device, queries quoted from them,
and the reference -- the oracle only knows the clipped cosine, so the chain is stated around it.  T = clip(chain(raw)): the unclipped
canonical cosine of the token rows against the query (sim_ops_cases.raw_cosine on the token rows instead of the vocabulary; for fp32
rows the same construction on oracle.sim_f32), the chain in numpy float32 as vectorian_amd/kernel.py states it, the clip; there is no
sim[id(t_j)][j] = 1 rewrite.  The oracle's contextual route takes the finished matrix (S_rows) for every algorithm."""

import numpy as np

import sim_ops_cases as sc
from vectorian_amd import synth


def raw_cosine(vo, X, Q):
	"""the unclipped canonical cosine of the token rows X against the query rows Q, bf16 bits or fp32 unit rows.  No cell may be 1.0 --
	a cosine above 1 would have been lost to the oracle's clip: the queries carry noise on every vector"""
	if np.asarray(X).dtype == np.uint16:
		return sc.raw_cosine(vo, X, Q)
	X, Q = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)
	pos, neg = vo.sim_f32(X, Q), vo.sim_f32(X, -Q)
	assert not ((pos != 0) & (neg != 0)).any()
	assert not ((pos == 1.0) | (neg == 1.0)).any()
	return pos - neg


def chain_rows(vo, X, Q, ops):
	"""(T, raw): the similarity matrix [n_tokens x len_t] of a contextual corpus under a chain, and the unclipped cosine"""
	raw = raw_cosine(vo, X, Q)
	T = np.clip(np.nan_to_num(sc.apply_numpy(ops, raw), nan=0.0), 0.0, 1.0).astype(np.float32)
	return T, raw


class Case:
	"""a contextual corpus on the device and what the oracle needs of it: n slices of lo .. hi tokens, then one slice per entry of
	`extra`; rows of d features as bf16 bits or (precision "f32") as fp32 unit rows"""

	def __init__(self, hip, vo, d, n=350, lo=3, hi=30, extra=(), seed=7, precision="bf16", V=500, pos=False, magnitudes=False):
		co = synth.make_contextual_corpus(n, lo, hi, V, d, seed=seed)
		rng = np.random.default_rng(seed + 100)
		more = int(sum(extra))
		X = co["X"]
		if more:
			X = np.concatenate([X, co["E"][synth.zipf_ids(more, V, rng)] + 0.1 * rng.standard_normal((more, d)).astype(np.float32)])
		if magnitudes:
			X = (X * rng.lognormal(0, 0.3, size=(len(X), 1))).astype(np.float32)
		lens = list(np.diff(co["sent_off"])) + list(extra)
		self.off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
		self.raw_rows = np.ascontiguousarray(X, dtype=np.float32)
		self.d, self.precision, self.hip, self.vo = d, precision, hip, vo
		self.mag = vo.magnitudes(self.raw_rows)
		self.X = vo.normalize_rows(self.raw_rows) if precision == "f32" else vo.normalize_rows_bf16(self.raw_rows)[0]
		self.pos = rng.integers(0, 4, size=len(X)).astype(np.int8) if pos else None
		self.longest = int(max(lens))
		self.magnitudes = magnitudes
		self.c = self.handle()

	def handle(self):
		hip = self.hip
		c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=self.d, n_tokens=len(self.X), n_sentences=len(self.off) - 1, precision=self.precision,
			keep_magnitudes=self.magnitudes)
		if self.magnitudes:
			c.append_vectors(self.raw_rows, normalize=True)
		else:
			c.append_vectors(self.X, normalize=False)
		if self.pos is not None:
			c.set_token_pos(self.pos)
		c.set_sentences(self.off)
		c.finalize()
		return c

	def rows(self, vec):
		"""unit rows of a query in the corpus's precision"""
		return self.vo.normalize_rows(vec) if self.precision == "f32" else self.vo.normalize_rows_bf16(vec)[0]

	def query(self, len_t, seed, noise=0.15):
		"""len_t tokens quoted from the corpus (across slices where none is that long) with noise on every vector -- no cosine reaches
		1 -- and one repeated token (the same vector twice: co-optimal tracebacks tie exactly).  Returns (raw vectors, unit rows)"""
		rng = np.random.default_rng(1000 * len_t + seed)
		start = int(rng.integers(0, len(self.raw_rows) - len_t))
		vec = self.raw_rows[start:start + len_t] / self.mag[start:start + len_t, None]
		vec = (vec + noise / np.sqrt(self.d / 64.0) * rng.standard_normal((len_t, self.d)).astype(np.float32)).astype(np.float32)
		if len_t > 2:
			vec[2] = vec[0]
		return vec, self.rows(vec)

	def reference(self, Q, ops, **kw):
		T, raw = chain_rows(self.vo, self.X, Q, ops)
		ref = self.vo.find(layout=self.vo.LAYOUT_CONTEXTUAL, d=self.d, sent_off=self.off, Q=Q, S_rows=[T], **kw)
		return ref, T, raw


def chain_for(name, vo, case, Q):
	"""the operators of chain `name` for this query: (b)'s threshold sits in the widest gap of the cells that reach it, window
	[0.55, 0.65], half a gap of at least 1e-5 (sim_ops_cases.pick_threshold: asserted, never skipped)"""
	if name != "b":
		return sc.chain(name)
	return sc.chain("b", sc.pick_threshold(sc.chain("a"), raw_cosine(vo, case.X, Q)))


# ---- the oracle-backed double of the public surface (tests/fake_backend.OracleCorpus with the chain stated around the oracle)

def _double():
	from fake_backend import _gap
	from oracle import vk_oracle as vo
	from sim_ops_backend import _OPERATOR, RecordingCorpus
	from vectorian_amd import core
	from vectorian_amd import kernel as K

	class ContextualChainOracleCorpus(RecordingCorpus):
		"""answers alignment queries over a contextual corpus under the chain set_contextual_sim_ops gave it, through the oracle's
		caller-supplied similarity matrix (chain_rows)"""

		def set_contextual_sim_ops(self, ops):
			self.calls.append(("set_contextual_sim_ops", [(k, a) for k, a in ops]))
			self.sim_ops = [(int(k), np.float32(a)) for k, a in ops]

		def _operators(self):
			return [K.DistanceToSimilarity() if k == K.VK_SIMOP_ONE_MINUS else _OPERATOR[k](np.float32(a)) for k, a in self.sim_ops]

		def filtered(self, pos_mask=0, tag_mask=0):
			f = super().filtered(pos_mask, tag_mask)
			g = ContextualChainOracleCorpus(layout=f.layout, d=f.d, n_tokens=f.n_tokens, n_sentences=f.n_sentences, vocab_size=f.vocab_size, precision=f.precision)
			g.__dict__.update({k: v for k, v in f.__dict__.items() if k not in ("calls", "lock")})
			g.sim_ops = list(self.sim_ops)   # a filtered corpus carries its source's chain (vk_corpus_filter)
			return g

		def query(self, q_vectors, *, locality=0, gap_s=0.0, gap_t=0.0, algorithm=0, q_normalize=True, max_matches=10, min_score=0.0, boost=None,
				want_flow=True, **rest):
			if not self.sim_ops:
				return super().query(q_vectors, locality=locality, gap_s=gap_s, gap_t=gap_t, algorithm=algorithm, q_normalize=q_normalize,
					max_matches=max_matches, min_score=min_score, boost=boost, want_flow=want_flow, **rest)
			assert algorithm == core.VK_ALG_ALIGN and self.layout == core.VK_LAYOUT_CONTEXTUAL
			assert all(v is None or v is False or v == 0 or k in ("rwmd", "wrd_normalize") for k, v in rest.items()), rest
			q = np.ascontiguousarray(q_vectors)
			q = synth.bf16_bits_to_f32(q) if q.dtype == np.uint16 else q.astype(np.float32)
			if self.precision == "f32":
				Q = vo.normalize_rows(q) if q_normalize else q
			else:
				Q = vo.normalize_rows_bf16(q)[0] if q_normalize else synth.to_bf16_bits(q)
			T, _ = chain_rows(vo, self._X, Q, self._operators())
			r = vo.find(layout=vo.LAYOUT_CONTEXTUAL, d=self.d, sent_off=self._off, sent_end=self._end, Q=Q, S_rows=[T], locality=int(locality),
				gap_s=_gap(gap_s, max(core.VK_MAX_SENT_LEN, self._longest()) + 1), gap_t=_gap(gap_t), max_matches=max_matches, min_score=min_score,
				boost=boost, want_all_scores=True)
			self._all = np.array(r["all_scores"], dtype=np.float32)
			top = core.TopK(max_matches, len(q))
			n = top.n = len(r["score"])
			top.score[:n], top.raw_score[:n], top.sentence[:n], top.mapping[:n] = r["score"], r["raw"], r["sentence"], r["mapping"]
			for i in range(n):
				a = int(self._off[int(r["sentence"][i])])
				for j in np.nonzero(r["mapping"][i] >= 0)[0]:
					top.edge_sim[i, j] = T[a + int(r["mapping"][i][j]), j]
			return top
	return ContextualChainOracleCorpus
