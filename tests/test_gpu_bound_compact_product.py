"""-m gpu: the product of the bound pass over a compact 6-bit tile with exact integers, as
tests/test_gpu_bound6_product.py holds MODE 8's.  vk_fp6c_bound_tile_probe packs 16 query rows whole and 16 token rows as a compact
tile of d features (vk_host::fp6c_put_row) and runs them through dot_tile_fp6<true>, MODE 9's loads: 64 x every cell must be the int64
product of the eighths over the features below d, whatever the query tile holds from d on (lanes 32 .. 63 of the last K-step and the
words 3 .. 5 of its quarter 1 feed zeros).  The bytes behind the tile's 3,712 are filled with 0x00 or with 0xff: a lane that read past
the tile -- a load of three words issued as four -- would move the product."""

import ctypes as C

import numpy as np
import pytest

from bound6_cases import EIGHTHS

pytestmark = pytest.mark.gpu

K = 384
WIDTHS = (289, 300, 304)


@pytest.fixture(scope="module")
def probe(hip):
	lib = hip.lib()
	lib.vk_fp6c_bound_tile_probe.restype = C.c_int
	lib.vk_fp6c_bound_tile_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]

	def run(q, x, d, fill=0xff):
		q, x = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(x, dtype=np.uint8)
		assert q.shape == (16, K) and x.shape == (16, K)
		out = np.full((16, 16), np.nan, dtype=np.float32)
		hip._check(lib.vk_fp6c_bound_tile_probe(q.ctypes.data, x.ctypes.data, d, fill, out.ctypes.data))
		return out.astype(np.float64) * 64
	return run


def expected(q, x, d):
	return EIGHTHS[q[:, :d]] @ EIGHTHS[x[:, :d]].T


def same(got, want):
	assert (got == want.astype(np.float64)).all(), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("d", WIDTHS)
def test_every_code_on_both_sides(probe, d):
	k, r = np.arange(K)[None, :], np.arange(16)[:, None]
	q = ((k * 5 + r * 11 + 3) % 64).astype(np.uint8)
	x = ((k * 7 + r * 13 + (k // 64) * 3 + 1) % 64).astype(np.uint8)
	want = expected(q, x, d)
	assert not (want == want.T).all() and (want != expected(q, x, K)).any()
	same(probe(q, x, d), want)


@pytest.mark.parametrize("side", ("token", "query"))
@pytest.mark.parametrize("d", WIDTHS)
def test_one_feature_at_a_time(probe, d, side):
	"""one operand holds a single nonzero feature k, the other random codes everywhere: the outer product of column k alone for k < d,
	zeros from d on -- which lane, which of parts P and Q and which bits a feature lives in, on either side"""
	rng = np.random.default_rng(6 + d)
	full = rng.integers(0, 64, size=(16, K)).astype(np.uint8)
	column = np.array([1, 9, 17, 25, 31, 33, 41, 49, 57, 63, 5, 37, 12, 44, 22, 54], dtype=np.uint8)
	for k in range(K):
		one = np.zeros((16, K), dtype=np.uint8)
		one[:, k] = np.roll(column, k)
		q, x = (full, one) if side == "token" else (one, full)
		want = np.outer(EIGHTHS[q[:, k]], EIGHTHS[x[:, k]]) if k < d else np.zeros((16, 16))
		same(probe(q, x, d), want)


@pytest.mark.parametrize("d", WIDTHS)
def test_the_bytes_behind_the_tile_do_not_reach_the_product(probe, d):
	rng = np.random.default_rng(60 + d)
	for _ in range(4):
		q = rng.integers(0, 64, size=(16, K)).astype(np.uint8)
		x = rng.integers(0, 64, size=(16, K)).astype(np.uint8)
		want = expected(q, x, d)
		zeros, ones = probe(q, x, d, fill=0x00), probe(q, x, d, fill=0xff)
		same(zeros, want)
		same(ones, want)


def test_the_largest_sums(probe):
	plus = np.full((16, K), 31, dtype=np.uint8)
	assert (probe(plus, plus, 304) == 64 * 304 * 56.25).all()
	k, r = np.arange(K)[None, :], np.arange(16)[:, None]
	signs_q = (31 + 32 * ((k + r) % 2)).astype(np.uint8)
	signs_x = (31 + 32 * ((k // 3 + r) % 2)).astype(np.uint8)
	same(probe(signs_q, signs_x, 300), expected(signs_q, signs_x, 300))
