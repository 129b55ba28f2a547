"""The operator chains the similarity-operator tests share (CPU and GPU tiers), and their reference: the operators of
vectorian_amd/kernel.py run in numpy float32 on a matrix, as the reference runs its callback (vectorian/sim/vector.py:194-196)."""

import numpy as np

from vectorian_amd.kernel import Bias, DistanceToSimilarity, Power, RadialBasis, Scale, Threshold


def chain(name, t=0.6):
	"""(a) .. (f); t: the threshold of (b)"""
	return {
		"a": [Bias(1), Scale(0.5)],
		"b": [Bias(1), Scale(0.5), Threshold(t)],
		"c": [DistanceToSimilarity()],
		"d": [Bias(1), Scale(0.5), Bias(-0.125), Scale(1.25), DistanceToSimilarity(), DistanceToSimilarity(), Bias(0.0625), Scale(0.9)],
		"e": [Power(2.5)],
		"f": [DistanceToSimilarity(), RadialBasis(1.5)],
	}[name]


def pairs(ops):
	"""(kind, float32 arg) per operator: what Corpus.set_sim_ops sends"""
	return [(int(op.sim_op[0]), np.float32(op.sim_op[1])) for op in ops]


def apply_numpy(ops, x):
	"""the chain on a float32 array of any shape, in place semantics of the reference on a copy"""
	m = np.array(x, dtype=np.float32).reshape(-1, 1)
	for op in ops:
		op.kernel(m)
		assert m.dtype == np.float32
	return m.reshape(np.shape(x))


# ---- the reference of the GPU checks: the oracle only knows the clipped cosine, so the chain is stated around it

def raw_cosine(vo, Eb, Qb, rewritten=None):
	"""the unclipped canonical cosine of bf16 rows: sim_bf16(E, Q) - sim_bf16(E, -Q).  Negating the query negates every product and
	every sum exactly, so one of the two clipped terms is 0.  A cell of 1.0 would have lost a cosine above 1 to the clip: none may,
	except (rewritten: a boolean matrix) where sim[id(t_j)][j] = 1 overwrites the cell anyway."""
	Eb, Qb = np.ascontiguousarray(Eb, dtype=np.uint16), np.ascontiguousarray(Qb, dtype=np.uint16)
	pos, neg = vo.sim_bf16(Eb, Qb), vo.sim_bf16(Eb, Qb ^ np.uint16(0x8000))
	assert not ((pos != 0) & (neg != 0)).any()
	one = (pos == 1.0) | (neg == 1.0)
	if rewritten is not None:
		one &= ~rewritten
	assert not one.any(), np.argwhere(one)[:5]
	return pos - neg


def rewrite_mask(V, q_ids):
	m = np.zeros((V, len(q_ids)), dtype=bool)
	for j, t in enumerate(q_ids):
		if 0 <= t < V:
			m[t, j] = True
	return m


def chain_table(vo, Eb, Qb, q_ids, ops, strict=True):
	"""the static similarity table under a chain: raw cosine, the chain in numpy float32 (vectorian_amd/kernel.py), sim[id(t_j)][j] = 1
	(metric/static.cpp:58-67), the clip (:75).  Returns (table, raw cosine, chain's output before the rewrite)"""
	mask = rewrite_mask(Eb.shape[0], q_ids)
	raw = raw_cosine(vo, Eb, Qb, None if strict else mask)
	mod = apply_numpy(ops, raw)
	T = mod.copy()
	T[mask] = 1.0
	T = np.clip(np.nan_to_num(T, nan=0.0), 0.0, 1.0).astype(np.float32)
	return T, raw, mod


def pick_threshold(ops_before, raw, lo=0.55, hi=0.65):
	"""the threshold of chain (b) for this case: the midpoint of the widest gap between the sorted cell values in [lo, hi] as they reach
	the Threshold -- the scoring pass (MFMA sums) and the restatement (canonical sums) differ by at most (d + 1) 2^-24 < 1e-5 per cell
	for unit rows of d <= 100 features, so with half a gap of at least 1e-5 both see every cell on the same side"""
	v = np.sort(apply_numpy(ops_before, raw).ravel())
	v = v[(v >= lo) & (v <= hi)].astype(np.float64)
	assert len(v) >= 2
	gaps = np.diff(v)
	i = int(np.argmax(gaps))
	assert gaps[i] / 2 >= 1e-5, gaps[i]
	return float(np.float32((v[i] + v[i + 1]) / 2))
