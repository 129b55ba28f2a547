"""What the vector-similarity tests share (CPU and GPU tiers): the numpy restatement of vectorian_amd/csrc/vk_sim_src_host.h -- every
term in float32 with one rounding per numpy operation of the reference, every sum over the features in float64 in the header's fixed
order (four partial sums over the features k mod 4 = g in ascending k, combined as (s0 + s1) + (s2 + s3), rounded to float32 once),
the finish in float32 -- the six chains of the GPU tier, and the static table under a source: source, chain, sim[id(t_j)][j] = 1, clip."""

import numpy as np

import sim_ops_cases as sc
from vectorian_amd import core
from vectorian_amd.kernel import Bias, DistanceToSimilarity, RadialBasis, Scale, Threshold
from vectorian_amd.sim import ImprovedSqrtCosineSim, PNormDistance


def _sum_in_order(terms):
	"""terms: float32 [..., d] -> float32 [...]: the header's order"""
	s = [np.zeros(terms.shape[:-1], np.float64) for _ in range(4)]
	for k in range(terms.shape[-1]):
		s[k & 3] = s[k & 3] + terms[..., k].astype(np.float64)
	return ((s[0] + s[1]) + (s[2] + s[3])).astype(np.float32)


def source_matrix(A, B, source):
	"""[n x m] float32: the cell of every row of A against every row of B under `source` = (kind, arg)"""
	kind, p = int(source[0]), np.float32(source[1])
	A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
	a, b = A[:, None, :], B[None, :, :]
	with np.errstate(divide="ignore", invalid="ignore"):
		if kind == core.VK_SIMSRC_SQRT_COSINE:
			num = _sum_in_order(np.sqrt(np.maximum(np.float32(0), a * b)))
			x, y = np.sqrt(_sum_in_order(np.abs(A))), np.sqrt(_sum_in_order(np.abs(B)))
			out = num / (x[:, None] * y[None, :])
			out[~np.isfinite(out)] = 0
			return out.astype(np.float32)
		assert kind == core.VK_SIMSRC_PNORM
		t = np.abs(a - b)
		if p == 1:
			return _sum_in_order(t)
		if p == 2:
			return np.sqrt(_sum_in_order(t * t))
		return np.power(_sum_in_order(np.power(t, p)), np.float32(1.0 / float(p)))


def source_of(sim):
	"""(kind, float32 arg) of a PNormDistance / ImprovedSqrtCosineSim"""
	kind, arg = sim.sim_source
	return int(kind), np.float32(arg)


def table(E, Q, q_ids, source, ops):
	"""the static table [V x len_t] under a source and a chain.  Returns (table, the chain's output before the rewrite)"""
	mod = sc.apply_numpy(ops, source_matrix(E, Q, source))
	T = mod.copy()
	T[sc.rewrite_mask(E.shape[0], q_ids)] = 1.0
	return np.clip(np.nan_to_num(T, nan=0.0), 0.0, 1.0).astype(np.float32), mod


def chain(name, E, Q):
	"""(source similarity, operators) of chain (i) .. (vi) for these vectors: the scale s / the width gamma put the median cell at
	one half (1 - s x = 1/2 at the median distance; exp(-gamma x^2) = 1/2 there)"""
	def median(sim):
		return float(np.median(source_matrix(E, Q, source_of(sim))))
	if name == "i":
		src = PNormDistance(2)
		return src, [Scale(1 / (2 * median(src))), DistanceToSimilarity()]
	if name == "ii":
		src = PNormDistance(1)
		return src, [Scale(1 / (2 * median(src))), DistanceToSimilarity(), Threshold(0.3)]
	if name == "iii":
		return ImprovedSqrtCosineSim(), []
	if name == "iv":
		return ImprovedSqrtCosineSim(), [Bias(-0.2), Scale(1.25)]
	if name == "v":
		src = PNormDistance(3)
		return src, [RadialBasis(np.log(2) / median(src) ** 2)]
	assert name == "vi"
	src = PNormDistance(0.5)
	return src, [Scale(1 / (2 * median(src))), DistanceToSimilarity()]


def assert_inside(T):
	"""the condition on the inputs every GPU test asserts: at least a third of the table's cells lie strictly inside (0, 1)"""
	inside = float(((T > 0) & (T < 1)).mean())
	assert inside >= 1 / 3, inside
