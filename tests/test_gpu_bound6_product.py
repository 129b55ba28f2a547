"""-m gpu: the product of the 6-bit bound pass with exact integers.  vk_fp6_bound_tile_probe packs 16 query rows and 16
token rows of E2M3 codes as vk_pack_query and the shadow pack them and runs them through dot_tile_fp6, the bound kernel's own product
(the query tile in LDS, the token tile's last K-step with `live6` of its quarters, v_mfma_scale_f32_16x16x128_f8f6f4 with both scales
x 1).  Every grid value is a multiple of 1 / 8, so 64 x the result must be the int64 product of the eighths, cell for cell: the lane
map of the operands, the 16-byte / 8-byte split of a lane's 24 bytes, the order of the bits, and the exactness of the float sum."""

import ctypes as C

import numpy as np
import pytest

from bound6_cases import EIGHTHS

pytestmark = pytest.mark.gpu

K = 384


@pytest.fixture(scope="module")
def probe(hip):
	lib = hip.lib()
	lib.vk_fp6_bound_tile_probe.restype = C.c_int
	lib.vk_fp6_bound_tile_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]

	def run(q, x, live6):
		q, x = np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(x, dtype=np.uint8)
		assert q.shape == (16, K) and x.shape == (16, K)
		out = np.full((16, 16), np.nan, dtype=np.float32)
		hip._check(lib.vk_fp6_bound_tile_probe(q.ctypes.data, x.ctypes.data, live6, out.ctypes.data))
		return out.astype(np.float64) * 64
	return run


def expected(q, x, live6):
	"""64 x the product over the features the kernel reads: the token tile holds features below 256 + 32 live6"""
	n = 256 + 32 * live6
	return EIGHTHS[q[:, :n]] @ EIGHTHS[x[:, :n]].T


def same(got, want):
	assert (got == want.astype(np.float64)).all(), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("live6", (1, 2, 3, 4))
def test_every_code_on_both_sides(probe, live6):
	"""an asymmetric pattern that holds all 64 codes in every row of both operands"""
	k, r = np.arange(K)[None, :], np.arange(16)[:, None]
	q = ((k * 5 + r * 11 + 3) % 64).astype(np.uint8)
	x = ((k * 7 + r * 13 + (k // 64) * 3 + 1) % 64).astype(np.uint8)
	assert all(len(set(row)) == 64 for row in q) and all(len(set(row)) == 64 for row in x)
	want = expected(q, x, live6)
	assert not (want == want.T).all()
	same(probe(q, x, live6), want)


def test_the_largest_sums(probe):
	"""every element +-7.5: signs aligned (the largest sum the format can hold, 384 x 56.25) and alternating"""
	k, r = np.arange(K)[None, :], np.arange(16)[:, None]
	plus = np.full((16, K), 31, dtype=np.uint8)
	got = probe(plus, plus, 4)
	assert (got == 64 * 384 * 56.25).all()
	signs_q = (31 + 32 * ((k + r) % 2)).astype(np.uint8)
	signs_x = (31 + 32 * ((k // 3 + r) % 2)).astype(np.uint8)
	same(probe(signs_q, signs_q, 4), expected(signs_q, signs_q, 4))
	same(probe(signs_q, signs_x, 4), expected(signs_q, signs_x, 4))
	same(probe(signs_q, signs_x ^ 32, 2), expected(signs_q, signs_x ^ 32, 2))


@pytest.mark.parametrize("side", ("token", "query"))
def test_one_feature_at_a_time(probe, side):
	"""one operand holds a single nonzero feature k (sixteen distinct values down its rows: the sixteen lanes (g, i) of element j = k % 32
	at once), the other random codes everywhere: the result is the outer product of column k alone -- for every k, which pins which
	lane and which bits of its 24 bytes a feature lives in, on either side"""
	rng = np.random.default_rng(6)
	full = rng.integers(0, 64, size=(16, K)).astype(np.uint8)
	column = np.array([1, 9, 17, 25, 31, 33, 41, 49, 57, 63, 5, 37, 12, 44, 22, 54], dtype=np.uint8)
	for k in range(K):
		one = np.zeros((16, K), dtype=np.uint8)
		one[:, k] = np.roll(column, k)
		q, x = (full, one) if side == "token" else (one, full)
		want = np.outer(EIGHTHS[q[:, k]], EIGHTHS[x[:, k]])
		same(probe(q, x, 4), want)


@pytest.mark.parametrize("live6", (1, 2, 3, 4))
def test_dead_quarters_do_not_reach_the_product(probe, live6):
	"""random codes in every feature of both operands: the token tile stores (and the kernel fetches) features below 256 + 32 live6
	only, and what the query tile holds beyond them must not count"""
	rng = np.random.default_rng(60 + live6)
	for _ in range(4):
		q = rng.integers(0, 64, size=(16, K)).astype(np.uint8)
		x = rng.integers(0, 64, size=(16, K)).astype(np.uint8)
		want = expected(q, x, live6)
		if live6 < 4:
			assert (want != expected(q, x, 4)).any()
		same(probe(q, x, live6), want)
