"""CPU tier: the operator chain of a ModifiedVectorSim (vectorian_amd/csrc/vk_sim_ops_host.h).  The header is the one
definition the table kernels and the canonical restatement compile for the device; here a g++ driver (once plain, once under
AddressSanitizer and UBSan) holds it against the operators of vectorian_amd/kernel.py run in numpy float32: bit for bit for the chains
made of exactly rounded operations, within a few ulp for powf / expf.  Then the operator classes themselves: values at hand-computed
points, name() strings, in-place semantics."""

import os
import subprocess

import numpy as np
import pytest

import sim_ops_cases as sc
from test_devbuf import CSRC, ROOT

from vectorian_amd import kernel as K
from vectorian_amd.sim import CosineSim, ModifiedVectorSim

T = 0.6


def _build(tmp, name, extra):
	exe = str(tmp / name)
	subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-ffp-contract=off", *extra, "-I", CSRC,
		os.path.join(ROOT, "tests", "sim_ops_driver.cpp"), "-o", exe], check=True)
	return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
	extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
	exe = _build(tmp_path_factory.mktemp("sim_ops_" + request.param), "sim_ops_driver", extra)

	def run(what, text):
		return subprocess.run([exe, what], input=text, check=True, capture_output=True, text=True).stdout.split()
	return run


def _bits(x):
	return int(np.float32(x).view(np.uint32))


def _header(ops):
	return " ".join([str(len(ops))] + [f"{k} {_bits(a):x}" for k, a in ops])


def _apply(driver, ops, x):
	out = driver("apply", _header(sc.pairs(ops)) + "\n" + "\n".join(f"{int(u):x}" for u in x.view(np.uint32)) + "\n")
	return np.array([int(w, 16) for w in out], dtype=np.uint32).view(np.float32)


def _grid():
	t = np.float32(T)
	# what reaches the threshold of chain (b) at t: (x + 1) * 0.5 around t
	around = np.float32(2) * t - np.float32(1)
	points = [0.0, -0.0, 1.0, -1.0, t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf)),
		around, np.nextafter(around, np.float32(np.inf)), np.nextafter(around, np.float32(-np.inf))]
	return np.concatenate([np.linspace(-1.1, 1.1, 100000).astype(np.float32), np.array(points, dtype=np.float32)])


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_exactly_rounded_chains_are_numpy_bit_for_bit(driver, name):
	ops = sc.chain(name, T)
	x = _grid()
	got, ref = _apply(driver, ops, x), sc.apply_numpy(ops, x)
	assert got.shape == ref.shape
	differ = got.view(np.uint32) != ref.view(np.uint32)
	assert not differ.any(), (name, x[differ][:5], got[differ][:5], ref[differ][:5])


def test_threshold_is_two_roundings_not_a_select(driver):
	"""max(0, x - t) + t is not x: the cell just above the threshold comes back rounded twice, and the test must be able to tell"""
	t = 0.1   # (next to t the subtraction is exact; a cell several binades above t loses the low bits of t twice)
	ops = [K.Threshold(t)]
	x = np.linspace(0.05, 1.1, 20001).astype(np.float32)
	got, ref = _apply(driver, ops, x), sc.apply_numpy(ops, x)
	assert (got.view(np.uint32) == ref.view(np.uint32)).all()
	select = np.where(x > np.float32(t), x, np.float32(0))
	assert (ref != select).any()


@pytest.mark.parametrize("name", ["e", "f"])
def test_transcendental_chains_are_numpy_within_a_few_ulp(driver, name):
	ops = sc.chain(name)
	x = _grid()
	got, ref = _apply(driver, ops, x), sc.apply_numpy(ops, x)
	assert np.isfinite(got).all() and (np.abs(got - ref) <= 4 * np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)))).all()


def test_empty_chain_is_the_identity(driver):
	x = _grid()
	assert (_apply(driver, [], x).view(np.uint32) == x.view(np.uint32)).all()


def test_check_refuses_what_the_entry_point_refuses(driver):
	ok = [(K.VK_SIMOP_BIAS, 1.0), (K.VK_SIMOP_RADIAL_BASIS, 1.5)]
	assert driver("check", _header(ok)) == ["0", "-1"]
	assert driver("check", "0") == ["0", "-1"]
	assert driver("check", _header(ok * 4)) == ["0", "-1"]                                   # 8 operators: the most
	assert driver("check", _header(ok * 4 + [(K.VK_SIMOP_SCALE, 2.0)])) == ["1", "-1"]      # 9
	assert driver("check", "-1") == ["1", "-1"]
	assert driver("check", _header([ok[0], (6, 1.0)])) == ["1", "1"]                         # an unknown kind
	assert driver("check", _header([ok[0], (-1, 1.0)])) == ["1", "1"]
	for bad in (np.nan, np.inf, -np.inf):
		assert driver("check", _header([ok[0], ok[1], (K.VK_SIMOP_SCALE, bad)])) == ["1", "2"]


# ---- the operator classes (vectorian/sim/kernel.py)

def _run(op, values):
	m = np.array([values], dtype=np.float32)
	alias = m
	op.kernel(m)
	assert alias is m and m.dtype == np.float32   # in place, on the caller's float32 matrix
	return m[0]


def test_operator_values_at_hand_computed_points():
	assert list(_run(K.Bias(1), [-1, -0.5, 0, 0.25])) == [0, 0.5, 1, 1.25]
	assert list(_run(K.Scale(0.5), [-1, 0, 0.5, 1])) == [-0.5, 0, 0.25, 0.5]
	assert list(_run(K.DistanceToSimilarity(), [-1, 0, 0.25, 1, 2])) == [2, 1, 0.75, 0, 0]
	assert list(_run(K.Threshold(0.5), [-1, 0.25, 0.5, 0.75, 1])) == [0, 0, 0, 0.75, 1]
	assert list(_run(K.Power(2), [-1, 0, 0.5, 1, 2])) == [0, 0, 0.25, 1, 4]
	assert list(_run(K.Power(0.5), [0.25, 4])) == [0.5, 2]
	rb = _run(K.RadialBasis(1.5), [0, 1, -1])
	assert rb[0] == 1 and rb[1] == rb[2] and abs(float(rb[1]) - np.exp(-1.5)) < 1e-7
	m = np.array([[-1, -0.2], [0.2, 1]], dtype=np.float32)
	K.Kernel([K.Bias(1), K.Scale(0.5)])(m)
	np.testing.assert_array_equal(m, np.array([[0, 0.4], [0.6, 1]], dtype=np.float32))


def test_operator_kinds_and_names():
	assert K.Bias(1).sim_op == (K.VK_SIMOP_BIAS, 1.0) and K.Scale(0.5).sim_op == (K.VK_SIMOP_SCALE, 0.5)
	assert K.Threshold(0.3).sim_op == (K.VK_SIMOP_THRESHOLD, 0.3) and K.DistanceToSimilarity().sim_op == (K.VK_SIMOP_ONE_MINUS, 0.0)
	assert K.Power(2.5).sim_op == (K.VK_SIMOP_POWER, 2.5) and K.RadialBasis(1.5).sim_op == (K.VK_SIMOP_RADIAL_BASIS, 1.5)
	from vectorian_amd import core
	assert (K.VK_SIMOP_BIAS, K.VK_SIMOP_SCALE, K.VK_SIMOP_THRESHOLD, K.VK_SIMOP_ONE_MINUS, K.VK_SIMOP_POWER, K.VK_SIMOP_RADIAL_BASIS) == (
		core.VK_SIMOP_BIAS, core.VK_SIMOP_SCALE, core.VK_SIMOP_THRESHOLD, core.VK_SIMOP_ONE_MINUS, core.VK_SIMOP_POWER, core.VK_SIMOP_RADIAL_BASIS) == (0, 1, 2, 3, 4, 5)
	header = open(os.path.join(ROOT, "include", "vectorian_hip.h")).read()
	assert "VK_SIMOP_BIAS = 0, VK_SIMOP_SCALE = 1, VK_SIMOP_THRESHOLD = 2" in header and "VK_SIMOP_ONE_MINUS = 3, VK_SIMOP_POWER = 4, VK_SIMOP_RADIAL_BASIS = 5" in header
	# the reference's strings (vectorian/sim/kernel.py)
	assert K.Bias(1).name("x") == "(x + 1)" and K.Scale(0.5).name("x") == "(x * 0.5)" and K.Power(2).name("x") == "(x ** 2)"
	assert K.Threshold(0.2).name("x") == "threshold(x, 0.2)" and K.RadialBasis(1.5).name("x") == "radialbasis(x, 1.5)"
	assert K.DistanceToSimilarity().name("x") == "(1 - x)"
	assert K.Kernel([K.Bias(1), K.Scale(0.5)]).name("cosine") == "((cosine + 1) * 0.5)"
	sim = ModifiedVectorSim(CosineSim(), K.Bias(1), K.Scale(0.5), K.Threshold(0.2))
	assert sim.name == "threshold(((cosine + 1) * 0.5), 0.2)"
	with pytest.raises(NotImplementedError):
		K.UnaryOperator().kernel(np.zeros((1, 1), np.float32))


def test_modified_vector_sim_computes_source_then_chain():
	from vectorian_amd.embedding import Vectors
	rng = np.random.default_rng(0)
	a, b = Vectors(rng.standard_normal((5, 8)).astype(np.float32)), Vectors(rng.standard_normal((3, 8)).astype(np.float32))
	plain, out = np.empty((5, 3), np.float32), np.empty((5, 3), np.float32)
	CosineSim()(a, b, plain)
	ModifiedVectorSim(CosineSim(), K.Bias(1), K.Scale(0.5))(a, b, out)
	np.testing.assert_array_equal(out, (plain + np.float32(1)) * np.float32(0.5))
	assert (plain < 0).any() and (out > 0).all()
