"""The independent reference of the exact transports: each slice's problem stated from the floats the library uses, and solved as a
float64 linear program (scipy's HiGHS) -- nothing of the solvers under test, nor of the oracle's vko_emd, is in it.

scipy is imported by lp_score alone: the GPU tier reads the stored scores (tests/golden/transport_lp.npz) and only calls the
functions that state the problems."""

import os

import numpy as np

from transport_cases import MODES, cases, input_hash

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transport_lp.npz")


def lp_score(a, b, C):
	"""a [n], b [m]: float64 masses; C [n x m]: float64 costs.  Minimises C.G over G >= 0 with row sums <= a, column sums <= b and
	total = min(sum a, sum b); returns 1 - optimum / moved (wrd.h:139: sum((1 - D) G) / sum(G))"""
	from scipy.optimize import linprog
	from scipy.sparse import csr_matrix, vstack

	a, b, C = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(C, np.float64)
	n, m = C.shape
	moved = min(a.sum(), b.sum())
	cell = np.arange(n * m)
	rows = csr_matrix((np.ones(n * m), (cell // m, cell)), shape=(n, n * m))
	cols = csr_matrix((np.ones(n * m), (cell % m, cell)), shape=(m, n * m))
	res = linprog(C.ravel(), A_ub=vstack([rows, cols], format="csr"), b_ub=np.concatenate([a, b]),
		A_eq=csr_matrix(np.ones((1, n * m))), b_eq=[moved], bounds=(0, None), method="highs",
		options=dict(primal_feasibility_tolerance=1e-9, dual_feasibility_tolerance=1e-9))
	if res.status != 0:
		raise RuntimeError(f"linprog: {res.message}")
	return 1.0 - res.fun / moved


def _sum_f32(x):
	"""float32 sum in position order (wrd.h:99-102)"""
	s = np.float32(0.0)
	for v in np.asarray(x, np.float32):
		s = np.float32(s + v)
	return s


class Problems:
	"""the transport problems of one case, from the floats the library uses: unit rows rounded to bf16 and the magnitudes of
	oracle.normalize_rows_bf16, similarities of oracle.sim_bf16 (static layout: 1 where the ids are equal)"""

	def __init__(self, vo, c):
		self.c, self.vo = c, vo
		self.static = c["layout"] == "static"
		self.off = c["off"]
		if self.static:
			self.Eb, self.emag = vo.normalize_rows_bf16(c["E"])
			self.ids = c["tok_id"]
			self.Xb, self.mag = self.Eb[self.ids], self.emag[self.ids]
		else:
			self.Xb, self.mag = vo.normalize_rows_bf16(c["X"])
		self.q = [vo.normalize_rows_bf16(q["vectors"]) for q in c["queries"]]

	def n_slices(self):
		return len(self.off) - 1

	def sim(self, qi, s):
		"""S [len_s x len_t], float32, in [0, 1]"""
		a, b = int(self.off[s]), int(self.off[s + 1])
		S = np.clip(self.vo.sim_bf16(self.Xb[a:b], self.q[qi][0]), 0.0, 1.0).astype(np.float32)
		if self.static:
			S[self.ids[a:b, None] == self.c["queries"][qi]["ids"][None, :]] = 1.0
		return S

	def masses(self, qi, s, mode):
		"""(query masses [len_t], slice masses [len_s]) as float32 -- exactly the library's"""
		a, b = int(self.off[s]), int(self.off[s + 1])
		qmag, smag = self.q[qi][1], self.mag[a:b]
		n, m = len(qmag), b - a
		if mode == "wrd_norm":
			return (qmag / _sum_f32(qmag)).astype(np.float32), (smag / _sum_f32(smag)).astype(np.float32)
		if mode == "wrd_raw":
			return qmag.astype(np.float32), smag.astype(np.float32)
		if mode == "nbow":
			return np.full(n, np.float32(1) / np.float32(n), np.float32), np.full(m, np.float32(1) / np.float32(m), np.float32)
		return np.ones(n, np.float32), np.ones(m, np.float32)

	def problem(self, qi, s, mode):
		"""(a [len_t], b [len_s], C [len_t x len_s]) in float64, or None for an empty slice"""
		if self.off[s + 1] - self.off[s] < 1:
			return None
		mt, ms = self.masses(qi, s, mode)
		C = np.maximum(np.float32(0), np.float32(1) - self.sim(qi, s)).T
		return mt.astype(np.float64), ms.astype(np.float64), C.astype(np.float64)

	def relaxed(self, qi, s):
		"""the nearest-neighbour relaxation's score over both directions (the oracle's rwmd), NaN for an empty slice"""
		a, b = int(self.off[s]), int(self.off[s + 1])
		if b - a < 1:
			return np.nan
		ids = dict(ids_s=self.ids[a:b], ids_t=self.c["queries"][qi]["ids"]) if self.static else {}
		return float(self.vo.rwmd(self.sim(qi, s), injective=True, symmetric=True, **ids))

	def oracle_find(self, qi, mode, max_matches, min_score):
		"""the oracle's result set of one query under one mode"""
		vo, c = self.vo, self.c
		alg, kw = MODES[mode]
		Qb, qmag = self.q[qi]
		if self.static:
			corpus = dict(layout=vo.LAYOUT_STATIC, tok_id=self.ids, E=self.Eb, X_mag=self.mag, q_ids=c["queries"][qi]["ids"])
		else:
			corpus = dict(layout=vo.LAYOUT_CONTEXTUAL, X=self.Xb, X_mag=self.mag)
		return vo.find(d=c["d"], sent_off=self.off, Q=Qb, Q_mag=qmag, algorithm=vo.ALG_WRD if alg == "wrd" else vo.ALG_RWMD,
			max_matches=max_matches, min_score=min_score, n_threads=8, **corpus, **kw)

	def oracle_scores(self, qi, mode):
		"""(raw score, score) of every slice as the oracle has them, NaN for the empty ones it skips"""
		n = self.n_slices()
		ref = self.oracle_find(qi, mode, n, -10.0)
		raw, score = np.full(n, np.nan), np.full(n, np.nan)
		raw[ref["sentence"]], score[ref["sentence"]] = ref["raw"], ref["score"]
		return raw, score


def _solve(job):
	return np.nan if job is None else lp_score(*job)


def case_scores(vo, c, pool=None):
	"""float64 [queries x modes (in MODES' order) x slices]: the LP score of every slice of a case (NaN: empty); pool: a
	multiprocessing pool"""
	P = Problems(vo, c)
	jobs = []
	for qi in range(len(c["queries"])):
		for mode in MODES:
			jobs.extend(P.problem(qi, s, mode) for s in range(P.n_slices()))
	# the largest problems first: the pool's tail is then made of small ones
	order = sorted(range(len(jobs)), key=lambda i: -(jobs[i][2].size if jobs[i] is not None else 0))
	solved = pool.map(_solve, [jobs[i] for i in order], chunksize=4) if pool is not None else [_solve(jobs[i]) for i in order]
	flat = np.empty(len(jobs), np.float64)
	flat[order] = solved
	return flat.reshape(len(c["queries"]), len(MODES), P.n_slices())


def all_scores(vo, n_procs=None):
	"""the fixture's content: every case's LP scores and input hashes"""
	import multiprocessing as mp
	out = {}
	with mp.get_context("fork").Pool(n_procs or min(16, os.cpu_count() or 1)) as pool:
		for c in cases():
			out[c["name"] + "/lp"] = case_scores(vo, c, pool)
			out[c["name"] + "/sha256"] = np.array(input_hash(c))
	return out


def load_golden():
	"""{case name: (LP scores [queries x modes x slices], sha256 of the inputs)}"""
	with np.load(GOLDEN) as z:
		return {c["name"]: (z[c["name"] + "/lp"], str(z[c["name"] + "/sha256"])) for c in cases()}


def mode_index(mode):
	return list(MODES).index(mode)
