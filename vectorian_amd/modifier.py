"""Token similarity modifiers: the combinators of `vectorian.sim.modifier` (vectorian/sim/modifier.py).

The reference builds every operand's similarity matrix completely -- VectorSim, chain, sim[id(t_j)][j] = 1, clip -- and hands the
clipped float32 matrices to one of these objects (ModifiedSimilarityMatrixFactory::create, metric/modifier.cpp:18-74): `__call__`
receives one dict of arrays per operand and fills `out`.  Nothing is clipped afterwards.

MixedTokenSimilarity(metrics, weights)   np.average over the operands, in float64, assigned into the float32 `out`
MaximumTokenSimilarity(metrics)          the cell-wise maximum, the first of equal values
MinimumTokenSimilarity(metrics)          ALSO the cell-wise maximum: upstream's ExtremumTokenSimilarity.__call__ selects with np.argmax
                                         for both subclasses and never reads the class attribute that would tell them apart.  This
                                         class mirrors that `__call__`, and the index runs what it computes.
UnaryTokenSimilarityModifier             an operator chain on ONE clipped matrix; it leaves [0, 1] unclipped and does not run on the
                                         device -- shape the vector similarity with ModifiedVectorSim instead.

HipBruteForceIndex runs Mixed / Maximum / Minimum over up to four EmbeddingTokenSim operands on static embeddings: one
per-query table per operand, combined cell by cell by vk_table_mix_kernel in the arithmetic of csrc/vk_sim_mix_host.h, which is the
arithmetic of the `__call__`s below.
"""

import numpy as np

from vectorian_amd.kernel import Kernel
from vectorian_amd.sim import TokenSim


class TokenSimilarityModifier(TokenSim):
	@property
	def is_modifier(self):
		return True

	@property
	def operands(self):
		raise NotImplementedError()


class UnaryTokenSimilarityModifier(TokenSimilarityModifier):
	"""operators of vectorian_amd.kernel on the clipped matrix of one operand; every other array is passed through"""

	def __init__(self, operand, operators):
		self._operand = operand
		self._kernel = Kernel(operators)

	def __call__(self, operands, out):
		only = operands[0]
		for key, values in only.items():
			out[key][:] = values
		self._kernel(out["similarity"])

	@property
	def operands(self):
		return [self._operand]

	@property
	def name(self):
		return self._kernel.name(self._operand.name)

	@property
	def embeddings(self):
		return list(self._operand.embeddings)


class MixedTokenSimilarity(TokenSimilarityModifier):
	"""the weighted mean of the operands' arrays -- similarities and magnitudes alike"""

	def __init__(self, metrics, weights):
		self._metrics = list(metrics)
		self._weights = weights

	@property
	def operands(self):
		return self._metrics

	@property
	def weights(self):
		return self._weights

	def __call__(self, operands, out):
		for key, dst in out.items():
			mean = np.average([x[key] for x in operands], axis=0, weights=self._weights)
			if mean.shape != dst.shape:
				raise ValueError(f"{key}: operands of shape {mean.shape}, output of shape {dst.shape}")
			dst[:] = mean   # float64 -> the array's float32: the one rounding

	@property
	def name(self):
		total = np.sum(self._weights)
		return "(" + " + ".join(f"{w / total} * {m.name}" for m, w in zip(self._metrics, self._weights)) + ")"

	@property
	def embeddings(self):
		return [m.embedding for m in self._metrics]


class ExtremumTokenSimilarity(TokenSimilarityModifier):
	"""the operand with the LARGEST similarity supplies a cell, whatever the subclass (see the module docstring)"""

	_label = None

	def __init__(self, metrics):
		self._metrics = list(metrics)

	@property
	def operands(self):
		return self._metrics

	def __call__(self, operands, out):
		stack = np.array([x["similarity"] for x in operands])
		chosen = np.argmax(stack, axis=0)   # the first of equal values
		out["similarity"][:] = np.take_along_axis(stack, chosen[np.newaxis], axis=0)[0]
		# (upstream would average magnitudes under a key "magnitudes" that its C++ side never passes: they stay unwritten there,
		# and here)

	@property
	def name(self):
		return f"{self._label}({', '.join(m.name for m in self._metrics)})"

	@property
	def embeddings(self):
		return [m.embedding for m in self._metrics]


class MaximumTokenSimilarity(ExtremumTokenSimilarity):
	_label = "maximum"


class MinimumTokenSimilarity(ExtremumTokenSimilarity):
	"""computes the cell-wise MAXIMUM, as upstream's does"""
	_label = "minimum"
