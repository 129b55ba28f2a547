"""CPU tier: the similarity cell of a contextual handle under an operator chain (vk_host::contextual_cell,
vectorian_amd/csrc/vk_sim_ops_host.h).  The function is the one statement of the cell that the scoring epilogues and the
restatement sites compile for the device; here a g++ driver with its own main (once plain, once under AddressSanitizer and UBSan) holds
it to numpy float32, bit for bit: clip(chain(x)) on the columns the query holds, 0 on the padding behind them, and the bare clip --
whatever the column -- without a chain."""

import os
import subprocess

import numpy as np
import pytest

import sim_ops_cases as sc
from test_devbuf import CSRC, ROOT

T = 0.6


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
	extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
	exe = str(tmp_path_factory.mktemp("contextual_cell_" + request.param) / "contextual_cell_driver")
	subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-ffp-contract=off", *extra, "-I", CSRC,
		os.path.join(ROOT, "tests", "contextual_cell_driver.cpp"), "-o", exe], check=True)

	def run(ops, x, in_query):
		head = " ".join([str(len(ops))] + [f"{k} {int(np.float32(a).view(np.uint32)):x}" for k, a in sc.pairs(ops)])
		text = head + "\n" + "\n".join(f"{int(q)} {int(u):x}" for q, u in zip(in_query, x.view(np.uint32))) + "\n"
		out = subprocess.run([exe, "cell"], input=text, check=True, capture_output=True, text=True).stdout.split()
		return np.array([int(w, 16) for w in out], dtype=np.uint32).view(np.float32)
	return run


def _grid():
	t = np.float32(T)
	around = np.float32(2) * t - np.float32(1)   # what reaches the threshold of chain (b) at t: (x + 1) * 0.5 around t
	points = [0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), t, around, np.nextafter(around, np.float32(np.inf)),
		np.nextafter(around, np.float32(-np.inf))]
	return np.concatenate([np.linspace(-1.1, 1.1, 100000).astype(np.float32), np.array(points, dtype=np.float32)])


def _clip(x):
	return np.clip(np.nan_to_num(np.asarray(x, dtype=np.float32), nan=0.0), np.float32(0), np.float32(1)).astype(np.float32)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_the_cell_is_numpy_bit_for_bit(driver, name):
	ops = sc.chain(name, T)
	x = _grid()
	got, ref = driver(ops, x, np.ones(len(x), bool)), _clip(sc.apply_numpy(ops, x))
	assert got.shape == ref.shape
	differ = got.view(np.uint32) != ref.view(np.uint32)
	assert not differ.any(), (name, x[differ][:5], got[differ][:5], ref[differ][:5])
	assert got.min() >= 0 and got.max() <= 1


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_padding_columns_stay_zero_under_a_chain(driver, name):
	"""chain(0) is no zero ((0 + 1) / 2 = 0.5; 1 - 0 = 1): the columns past the query are zeroed after the chain, before the clip"""
	ops = sc.chain(name, T)
	x = _grid()
	got = driver(ops, x, np.zeros(len(x), bool))
	assert (got.view(np.uint32) == 0).all()
	assert _clip(sc.apply_numpy(ops, np.zeros(1, np.float32)))[0] > 0 or name == "b"   # (b): 0.5 is below the threshold


def test_no_chain_is_the_clip_whatever_the_column(driver):
	x = np.concatenate([_grid(), np.array([np.nan, np.inf, -np.inf], dtype=np.float32)])
	ref = _clip(x)
	ref[-2] = 1.0
	for in_query in (np.ones(len(x), bool), np.zeros(len(x), bool)):
		got = driver([], x, in_query)
		assert (got == ref).all()   # (as values: which zero fmaxf(-0, 0) returns is the platform's choice, here and on the device)
