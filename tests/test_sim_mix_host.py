"""CPU tier: the token similarity combinators (vectorian_amd/csrc/vk_sim_mix_host.h).  The header is the one definition
vk_table_mix_kernel compiles for the device; here a g++ driver (once plain, once under AddressSanitizer and UBSan) holds
sim_mix_cell against the reference's own numpy calls -- np.average(.., weights=w) assigned into a float32 array, np.maximum.reduce --
bit for bit, for 2, 3 and 4 operands, float weights, int weights and a weight of 0, over 10^5 clipped float32 cells with 0, 1 and
subnormal-sized cells among them."""

import os
import subprocess

import numpy as np
import pytest

from test_devbuf import CSRC, ROOT

from vectorian_amd import core

N = 100000


def _build(tmp, name, extra):
	exe = str(tmp / name)
	subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-ffp-contract=off", *extra, "-I", CSRC,
		os.path.join(ROOT, "tests", "sim_mix_driver.cpp"), "-o", exe], check=True)
	return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
	extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
	exe = _build(tmp_path_factory.mktemp("sim_mix_" + request.param), "sim_mix_driver", extra)

	def run(what, text):
		return subprocess.run([exe, what], input=text, check=True, capture_output=True, text=True).stdout.split()
	return run


def _cells(m, seed):
	"""[m x N] clipped float32 cells as a table holds them: values of [0, 1], with exact 0 and 1, subnormal-sized and tiny normal
	cells, and positions where the operands are equal"""
	rng = np.random.default_rng(seed)
	x = np.clip(rng.uniform(-0.3, 1.2, size=(m, N)), 0, 1).astype(np.float32)
	special = np.array([0.0, 1.0, 1e-45, 3e-42, 1.1754942e-38, 1.1754944e-38, 5e-30, np.nextafter(np.float32(1), np.float32(0))], dtype=np.float32)
	at = rng.integers(0, N, size=(m, 4000))
	for i in range(m):
		x[i, at[i]] = special[rng.integers(0, len(special), size=4000)]
	x[:, :500] = x[0, :500]   # equal operands
	assert (x == 0).any() and (x == 1).any() and ((x > 0) & (x < 1.17e-38)).any()
	return x


def _w64(w):
	return [f"{int(np.float64(v).view(np.uint64)):x}" for v in w]


def _cell(driver, kind, weights, x):
	m = x.shape[0]
	head = " ".join([str(kind), str(m)] + _w64(weights if weights is not None else [0] * m))
	lines = [" ".join(f"{int(u):x}" for u in col) for col in x.view(np.uint32).T]
	out = driver("cell", head + "\n" + "\n".join(lines) + "\n")
	return np.array([int(w, 16) for w in out], dtype=np.uint32).view(np.float32)


WEIGHTS = {
	2: [[0.3, 0.7], [2, 1], [0, 5], [1e-3, 123.456]],
	3: [[0.2, 0.5, 0.3], [1, 2, 3], [1.5, 0, 0.25]],
	4: [[0.1, 0.2, 0.3, 0.4], [4, 3, 2, 1], [0, 0.7, 0, 0.1]],
}


@pytest.mark.parametrize("m", [2, 3, 4])
def test_average_is_np_average_bit_for_bit(driver, m):
	x = _cells(m, seed=m)
	for w in WEIGHTS[m]:
		ref = np.empty(N, np.float32)
		ref[:] = np.average(list(x), axis=0, weights=w)   # as MixedTokenSimilarity.__call__: float64, rounded once on assignment
		got = _cell(driver, core.VK_SIMMIX_AVERAGE, w, x)
		assert got.shape == ref.shape
		differ = got.view(np.uint32) != ref.view(np.uint32)
		assert not differ.any(), (w, x[:, differ][:, :5], got[differ][:5], ref[differ][:5])


@pytest.mark.parametrize("m", [2, 3, 4])
def test_maximum_is_np_maximum_bit_for_bit(driver, m):
	x = _cells(m, seed=10 + m)
	ref = np.maximum.reduce(list(x))
	stack = np.array(list(x))
	assert (ref == np.take_along_axis(stack, np.argmax(stack, axis=0)[None], axis=0)[0]).all()   # the reference's own call
	got = _cell(driver, core.VK_SIMMIX_MAXIMUM, None, x)
	assert (got.view(np.uint32) == ref.view(np.uint32)).all()


def test_zeros_stay_zero_and_ones_stay_one(driver):
	"""the padding of the operands' tables needs no mask, and sim[id(t_j)][j] = 1 survives the combination"""
	x = np.array([[0, 1], [0, 1], [0, 1]], dtype=np.float32)
	for w in WEIGHTS[3]:
		assert list(_cell(driver, core.VK_SIMMIX_AVERAGE, w, x)) == [0, 1]
	assert list(_cell(driver, core.VK_SIMMIX_MAXIMUM, None, x)) == [0, 1]


def test_check_refuses_what_the_entry_point_refuses(driver):
	def check(kind, n, weights, has=True):
		return driver("check", " ".join([str(kind), str(n), str(int(has))] + _w64(weights)))[0]
	ok, bad = "0", str(core.VK_ERR_INVALID)
	assert check(core.VK_SIMMIX_AVERAGE, 2, [1, 2]) == ok and check(core.VK_SIMMIX_AVERAGE, 4, [0, 0, 0, 1e-300]) == ok
	assert check(core.VK_SIMMIX_MAXIMUM, 3, [], has=False) == ok
	assert check(core.VK_SIMMIX_NONE, 2, [1, 1]) == bad and check(3, 2, [1, 1]) == bad
	assert check(core.VK_SIMMIX_AVERAGE, 1, [1]) == bad and check(core.VK_SIMMIX_AVERAGE, 5, [1] * 5) == bad
	assert check(core.VK_SIMMIX_MAXIMUM, 5, [], has=False) == bad and check(core.VK_SIMMIX_AVERAGE, -1, []) == bad
	assert check(core.VK_SIMMIX_AVERAGE, 2, [], has=False) == bad   # no weights
	for w in ([1, -1e-9], [np.nan, 1], [np.inf, 1], [0, 0]):
		assert check(core.VK_SIMMIX_AVERAGE, 2, w) == bad, w
	header = open(os.path.join(ROOT, "include", "vectorian_hip.h")).read()
	assert "VK_SIMMIX_NONE = 0, VK_SIMMIX_AVERAGE = 1, VK_SIMMIX_MAXIMUM = 2" in header and "#define VK_MAX_SIM_OPERANDS 4" in header
	assert core.VK_MAX_SIM_OPERANDS == 4
