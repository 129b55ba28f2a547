"""-m gpu: the bytes of the dead quarters of a shadow tile's last K-step do not reach the bound kernel's product.  One tile of
random int8 and one 8-bit query through vk_i8_bound_tile_probe, which runs the shipped product of MODE 7 (dot_tile_i8: the query tile in
LDS, `live` of the four 16-lane quarters of the last 1 KiB block feeding the MFMA, zero registers for the rest), for both compile-time
forms: five K-steps (289 .. 304 features) and twelve (753 .. 768).
The query's features past d are zero, as vk_pack_query leaves them; the tile's dead quarters are filled with non-zero garbage here
(the shadow holds zeros there: a kernel that used them would compute the same, so zeros could not tell the two kernels apart).
  live = 1, 2, 3: the product equals numpy's integer product over the live features exactly -- and, taken with a query that is NOT
zero past d, still does: the dead quarters' bytes never reach the MFMA.
  live = 4: the whole block is used, so with a non-zero query the garbage shows in the product -- the test can see those lanes.
What this proves is the arithmetic.  That the lanes issue no load (rather than load and discard) is a matter of the generated code and
of the fetch counter recorded in DESIGN 11.7, not of this test."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def probe(hip, q, x, nk, live):
	lib = hip.lib()
	lib.vk_i8_bound_tile_probe.restype = C.c_int
	lib.vk_i8_bound_tile_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
	q, x = np.ascontiguousarray(q), np.ascontiguousarray(x)
	assert q.shape == x.shape == (16, 64 * nk) and q.dtype == x.dtype == np.int8
	out = np.full((16, 16), -1, dtype=np.int32)
	hip._check(lib.vk_i8_bound_tile_probe(q.ctypes.data, x.ctypes.data, nk, live, out.ctypes.data))
	return out


@pytest.mark.parametrize("live", (1, 2, 3, 4))
@pytest.mark.parametrize("nk", (5, 12))
def test_dead_quarters_are_not_fetched(hip, nk, live):
	rng = np.random.default_rng(100 * nk + live)
	K = 64 * nk
	d = 64 * (nk - 1) + 16 * live                                   # the widest row with this many live quarters
	nz = lambda shape: (rng.integers(1, 128, size=shape) * rng.choice((-1, 1), size=shape)).astype(np.int8)   # never zero
	x = nz((16, K))                                                  # features >= d: garbage where the shadow holds zeros
	q_full = nz((16, K))
	q = q_full.copy()
	q[:, d:] = 0                                                     # what vk_pack_query leaves past d
	want = q[:, :d].astype(np.int32) @ x[:, :d].astype(np.int32).T   # out[j][i] = q[j] . x[i] over the live features
	assert (probe(hip, q, x, nk, live) == want).all()
	# a narrower row in the same quarter: the query's zeros inside the last live quarter do the rest
	q2 = q.copy()
	q2[:, d - 15:] = 0
	assert (probe(hip, q2, x, nk, live) == q2[:, :d].astype(np.int32) @ x[:, :d].astype(np.int32).T).all()
	got_full = probe(hip, q_full, x, nk, live)
	if live < 4:
		# a query that is not zero past d still sees nothing of the dead quarters: their bytes are replaced by zeros
		assert (got_full == q_full[:, :d].astype(np.int32) @ x[:, :d].astype(np.int32).T).all()
	else:
		assert d == K
		assert (got_full == q_full.astype(np.int32) @ x.astype(np.int32).T).all()


@pytest.mark.parametrize("nk", (5, 12))
def test_garbage_shows_when_every_quarter_is_live(hip, nk):
	"""the same garbage in the last quarter, live = 4 against live = 3: the live quarter's bytes change the product, the dead one's do not --
	the probe does see the lanes the other cases rely on not being read"""
	rng = np.random.default_rng(7 + nk)
	K = 64 * nk
	x = rng.integers(-127, 128, size=(16, K)).astype(np.int8)
	x[:, K - 16:] = rng.integers(1, 128, size=(16, 16)).astype(np.int8)      # the last quarter: positive garbage
	q = rng.integers(-127, 128, size=(16, K)).astype(np.int8)
	q[:, K - 16:] = rng.integers(1, 128, size=(16, 16)).astype(np.int8)      # positive too: every cell's share of the quarter is > 0
	with4, with3 = probe(hip, q, x, nk, 4), probe(hip, q, x, nk, 3)
	assert (with4 == q.astype(np.int32) @ x.astype(np.int32).T).all()
	assert (with3 == q[:, :K - 16].astype(np.int32) @ x[:, :K - 16].astype(np.int32).T).all()
	assert (with4 > with3).all()
