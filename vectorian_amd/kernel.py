"""Operators that shape a vector similarity: the surface of `vectorian.sim.kernel`.

UnaryOperator                     vectorian/sim/kernel.py:6-11
RadialBasis                       vectorian/sim/kernel.py:14-22
DistanceToSimilarity              vectorian/sim/kernel.py:25-30
Bias / Scale / Power / Threshold  vectorian/sim/kernel.py:33-76
Kernel                            vectorian/sim/kernel.py:79-97

The same constructor arguments, the same in-place numpy semantics on the similarity matrix and the same `name(operand)`
strings as the reference.  Each operator also states itself as `sim_op = (kind, arg)`: what `vk_corpus_set_sim_ops` takes, and
what the device then runs on every cell of a static corpus's similarity table (csrc/vk_sim_ops_host.h) -- in float32, one
rounding per numpy operation below, so that the two agree bit for bit wherever the operation is exactly rounded.
"""

import numpy as np

# the kinds of include/vectorian_hip.h (spelled out: this module needs no library to load)
VK_SIMOP_BIAS, VK_SIMOP_SCALE, VK_SIMOP_THRESHOLD, VK_SIMOP_ONE_MINUS, VK_SIMOP_POWER, VK_SIMOP_RADIAL_BASIS = 0, 1, 2, 3, 4, 5


class UnaryOperator:
	def kernel(self, data: np.ndarray):
		raise NotImplementedError()

	def name(self, operand):
		raise NotImplementedError()

	@property
	def sim_op(self):
		"""(kind, arg) for vk_corpus_set_sim_ops"""
		raise NotImplementedError()


class RadialBasis(UnaryOperator):
	def __init__(self, gamma: float):
		self._gamma = gamma

	def kernel(self, data: np.ndarray):
		data[:, :] = np.exp(-self._gamma * np.power(data, 2))

	def name(self, operand):
		return f'radialbasis({operand}, {self._gamma})'

	@property
	def sim_op(self):
		return VK_SIMOP_RADIAL_BASIS, float(self._gamma)


class DistanceToSimilarity(UnaryOperator):
	def kernel(self, data: np.ndarray):
		data[:, :] = np.maximum(0, 1 - data)

	def name(self, operand):
		return f'(1 - {operand})'

	@property
	def sim_op(self):
		return VK_SIMOP_ONE_MINUS, 0.0


class Bias(UnaryOperator):
	def __init__(self, bias: float):
		self._bias = bias

	def kernel(self, data: np.ndarray):
		data += self._bias

	def name(self, operand):
		return f'({operand} + {self._bias})'

	@property
	def sim_op(self):
		return VK_SIMOP_BIAS, float(self._bias)


class Scale(UnaryOperator):
	def __init__(self, scale: float):
		self._scale = scale

	def kernel(self, data: np.ndarray):
		data *= self._scale

	def name(self, operand):
		return f'({operand} * {self._scale})'

	@property
	def sim_op(self):
		return VK_SIMOP_SCALE, float(self._scale)


class Power(UnaryOperator):
	def __init__(self, exp: float):
		self._exp = exp

	def kernel(self, data: np.ndarray):
		data[:, :] = np.power(np.maximum(data, 0), self._exp)

	def name(self, operand):
		return f'({operand} ** {self._exp})'

	@property
	def sim_op(self):
		return VK_SIMOP_POWER, float(self._exp)


class Threshold(UnaryOperator):
	def __init__(self, threshold: float):
		self._threshold = threshold

	def kernel(self, data: np.ndarray):
		x = np.maximum(0, data - self._threshold)
		x[x > 0] += self._threshold
		data[:, :] = x

	def name(self, operand):
		return f'threshold({operand}, {self._threshold})'

	@property
	def sim_op(self):
		return VK_SIMOP_THRESHOLD, float(self._threshold)


class Kernel:
	def __init__(self, operators):
		self._operators = list(operators)

	@property
	def operators(self):
		return list(self._operators)

	def __call__(self, data: np.ndarray):
		for x in self._operators:
			x.kernel(data)

	def name(self, operand):
		name = operand
		for x in self._operators:
			name = x.name(name)
		return name
