"""CPU tier: the cells of vectorian_amd/csrc/vk_saliency_host.h against numpy and scipy.  A g++ driver with its own main
(tests/saliency_driver.cpp), built plain and with AddressSanitizer / UBSan and run as a stand-alone program, computes the header's
keyword signal, filters and average for the cases of saliency_cases.py: counts and their clipping ==, the max filter == scipy's, the
`same` convolution within one float32 ulp of np.convolve's (numpy does not specify the order of its sum; the header does), the
pass-through ==, the average == np.average's.  The grids of the three kernels are walked on the host: every slice exactly once."""

import os
import re
import subprocess

import numpy as np
import pytest

import saliency_cases as sc
from test_devbuf import CSRC, ROOT

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
	work = tmp_path_factory.mktemp("saliency_" + request.param)
	exe = str(work / "saliency_driver")
	subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (SANITIZE if request.param == "sanitized" else []) +
		["-I", CSRC, os.path.join(ROOT, "tests", "saliency_driver.cpp"), "-o", exe], check=True)

	def run(cmd, args, arrays, n_out):
		src, dst = str(work / "in.bin"), str(work / "out.bin")
		with open(src, "wb") as f:
			for a in arrays:
				f.write(np.ascontiguousarray(a).tobytes())
		r = subprocess.run([exe, cmd, *[str(a) for a in args], src, dst], capture_output=True, text=True)
		assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-3000:])
		out = np.fromfile(dst, dtype=np.float32)
		assert out.shape == (n_out,)
		return out
	run.exe = exe
	return run


@pytest.mark.parametrize("max_count", [1, 3])
def test_counts_and_their_clipping(driver, max_count):
	"""slices of 0 .. 200 tokens, overlapping, over a vocabulary of 37; keywords that hit, one id used twice; tokens without an id (-1)
	and with an id beyond the vocabulary never count"""
	rng = np.random.default_rng(7)
	V = 37
	ids = rng.integers(0, V, 900).astype(np.int32)
	ids[rng.random(900) < 0.1] = -1
	ids[5], ids[6] = V, 2 ** 31 - 1
	ids[0], ids[1], ids[2] = 3, 3, 11   # one hit in the slice of one token, two in the slice of two
	lens = [0, 1, 2, 31, 32, 33, 63, 64, 65, 200, 0, 7]
	start = np.array([0, 0, 1, 3, 20, 40, 60, 100, 150, 210, 410, 893], dtype=np.int64)
	end = start + np.array(lens, dtype=np.int64)
	assert end.max() <= len(ids)
	kw = np.array([3, 11, 11, 36, 0], dtype=np.int32)
	got = driver("keywords", [V, max_count, len(ids), len(start), len(kw)], [ids, start, end, kw], len(start))
	want = sc.keyword_signal(ids, start, end, kw, max_count)
	assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
	assert got[0] == 0.0 and got.max() == 1.0   # an empty slice; a clipped one
	if max_count == 3:
		assert len(np.unique(got)) == 4   # 0, 1/3, 2/3, 1: the clip and the float32 division both show


@pytest.mark.parametrize("case", sc.filter_cases(), ids=lambda c: c[0])
def test_filters(driver, case):
	name, kind, width, pulse, off, x, want = case
	arrays = [x, off] + ([pulse] if kind == 1 else [])
	got = driver("filter", [kind, width, len(off) - 1, len(x)], arrays, len(x))
	sc.assert_filtered(got, case)


def test_the_cases_hold_what_the_issue_asks():
	cases = sc.filter_cases()
	assert sorted(c[2] for c in cases if c[1] == 0) == [1, 2, 3, 4, 5, 8]
	assert sorted({c[2] for c in cases if c[1] == 1}) == list(range(1, 10))
	for name, kind, width, pulse, off, x, want in cases:
		lens = set(np.diff(off).tolist())
		assert {1, 2, max(width - 1, 1), width, width + 1} <= lens, name
		if kind == 1 and width > 1:   # a document shorter than the pulse passes through, and the case shows it
			assert any(0 < b - a < width for a, b in zip(off[:-1], off[1:]))
		assert not np.array_equal(want, x) or width == 1, name   # the filter does something


@pytest.mark.parametrize("strength", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("m", range(0, 7))
def test_the_average_is_numpys(driver, m, strength):
	"""0 .. 6 signals (7 weights: below numpy's block of 8), unequal weights"""
	n = 501
	signals = [sc.signal_values(n, 300 + k) for k in range(m)]
	user = [1.0, 0.25, 3.0, 0.7, 2.0, 0.1][:m]
	w = sc.saliency_weights(user, strength)
	got = driver("average", [m, n], [np.asarray(w, dtype=np.float64)] + signals, n)
	want = sc.average(signals, w, n)
	assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (m, strength, np.flatnonzero(got != want)[:5])
	if m == 0:
		assert (got == 1.0).all()


@pytest.mark.parametrize("m", [7, 8])
def test_the_weights_sum_follows_numpys_block_of_eight(driver, m):
	"""8 and 9 weights: np.average's scale is numpy's unrolled sum, which sal_numpy_sum restates"""
	n = 257
	signals = [sc.signal_values(n, 400 + k) for k in range(m)]
	w = sc.saliency_weights([1.0, 0.25, 3.0, 0.7, 2.0, 0.1, 0.9, 1.3][:m], 0.37)
	got = driver("average", [m, n], [np.asarray(w, dtype=np.float64)] + signals, n)
	want = sc.average(signals, w, n)
	assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_every_slice_is_visited_once(driver):
	r = subprocess.run([driver.exe, "geometry"], capture_output=True, text=True)
	out = r.stdout.split("\n")[:-1]
	assert r.returncode == 0 and not [line for line in out if line.startswith("VIOLATED")], (out[:10], r.stderr[-2000:])
	points, violations = [int(x) for x in re.fullmatch(r"points (\d+) violations (\d+)", out[-1]).groups()]
	assert violations == 0 and points == 2 * 19


def test_the_kernels_and_the_entry_points_read_the_header():
	kernel, corpus = [open(os.path.join(CSRC, name)).read() for name in ("vk_saliency.hip", "vk_corpus.cpp")]
	assert '#include "vk_saliency_host.h"' in kernel and '#include "vk_saliency_host.h"' in corpus
	for name in ("sal_is_keyword(", "sal_signal_value(", "sal_filter_cell(", "sal_doc_of(", "sal_boost_cell(", "sal_boost_bounds_ok(",
			"sal_keyword_first(", "sal_keyword_stride(", "sal_keyword_grid(", "sal_cell_grid(", "sal_cell_of("):
		assert "vk_host::" + name in kernel, name
	for name in ("sal_bitmap_set(", "sal_numpy_sum(", "sal_check_docs("):
		assert "vk_host::" + name in corpus, name
