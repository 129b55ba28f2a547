"""-m gpu: every byte of a corpus's shadow, read back from the device, against the numpy restatements of the two
quantizers and of the two tile orders (tests/bound_cases.py, tests/bound6_cases.py) -- the same restatements the CPU tier holds the
host quantizers against, so that the query's side and the corpus's side of a bound are one function:
  * the codes of every row, byte for byte, in the tile's operand order;
  * s_x and e_x of every row, bit for bit (the double sums taken in k order, rounded up as up() does);
  * N and X of the corpus as the largest restated n and a, bit for bit;
  * zeros for every feature past d, for the rows past the corpus in the last tile and for the zero tile behind it;
  * the format the handle reports: bits, K-steps, live quarters of the last K-step, bytes per tile.
One corpus per case: 40 tokens in 3 slices (two whole tiles, one of 8 rows, the zero tile), at the widths where a format changes form
-- 289, 300 and 304 features in 8 and in 6 bits, 753 and 768 in 8 bits and with 6 asked for (the 8-bit form all the same).  Among
the rows: one of zeros, one whose largest element is negative, one on the midpoints of all three E2M3 steps (s = 1), one on .5 ties
of the int8 grid (s = 1; the two grids have no common scale in bf16, so each has its row, and each row is in every corpus), one of
magnitudes around 1e-20."""

import numpy as np
import pytest

import bound6_cases as b6
import bound_cases as bc
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

F = np.float32
N_ROWS, OFF = 40, np.array([0, 13, 14, 40], dtype=np.int64)
TIES6 = np.array([7.5, 0.0625, 0.1875, -0.3125, 1.9375, 2.125, 2.375, -3.875, 4.25, 4.75, 7.25, -7.5, 0.0, 3.75, -1.875, 0.125], dtype=F)
TIES8 = np.array([127, 0.5, 1.5, -2.5, 63.5, -126.5, 126.5, 3.5, -0.5, 100.5, -127, 0.0, 64.5, -1.5, 2.5, 1.0], dtype=F)
# (d, VK_BOUND_BITS) -> bits, K-steps, live quarters, bytes per tile
CASES = {
	(289, "8"): (8, 5, 3, 5248), (300, "8"): (8, 5, 3, 5248), (304, "8"): (8, 5, 3, 5248),
	(289, "6"): (6, 3, 2, 3968), (300, "6"): (6, 3, 2, 3968), (304, "6"): (6, 3, 2, 3968),
	(753, "8"): (8, 12, 4, 12416), (768, "8"): (8, 12, 4, 12416), (753, "6"): (8, 12, 4, 12416), (768, "6"): (8, 12, 4, 12416),
}


def rows_of(d):
	"""the rows as stored: every value a bf16 number"""
	rng = np.random.default_rng(d)
	x = b6.stored(rng.standard_normal((N_ROWS, d)).astype(F))
	x[5] = 0.0                                                   # a row of zeros
	x[9, d // 3] = -0.75                                         # the largest element is negative
	x[17] = 0.0; x[17, :8] = TIES6[:8]; x[17, d - 8:] = TIES6[8:]   # midpoints of the E2M3 steps, some in the last K-step
	x[18] = 0.0; x[18, :8] = TIES8[:8]; x[18, d - 8:] = TIES8[8:]   # .5 ties of the int8 grid
	x[33] = synth.bf16_bits_to_f32(synth.to_bf16_bits(F(1e-20) * x[33]))   # tiny throughout, in the partial tile
	assert (synth.bf16_bits_to_f32(synth.to_bf16_bits(x)) == x).all()
	assert np.abs(x[9]).argmax() == d // 3 and np.abs(x[33]).max() < 1e-20
	return x


def restated(x, bits, steps, live):
	"""(the tiles' bytes [tiles, tile_bytes], N, X) by the numpy restatements; rows past the corpus: zeros throughout"""
	tiles = (len(x) + 15) // 16 + 1
	width = 384 if bits == 6 else 64 * steps
	codes = np.zeros((16 * tiles, width), dtype=np.uint8 if bits == 6 else np.int8)
	meta = np.zeros((16 * tiles, 2), dtype=F)
	if bits == 6:
		c, s, e, n, a = b6.quantize6(x)
	else:
		c, s, e, n, a = (np.array(v) for v in zip(*[bc.quantize8(r) for r in x]))
	codes[:len(x), :x.shape[1]] = c
	meta[:len(x), 0], meta[:len(x), 1] = s, e
	out = []
	for t in range(tiles):
		rows = slice(16 * t, 16 * t + 16)
		body = b6.pack_tile(codes[rows], live) if bits == 6 else bc.pack_tile8(codes[rows])
		out.append(np.concatenate([body, meta[rows].reshape(-1).view(np.uint8)]))
	return np.stack(out), n.max(), a.max(), codes, meta


@pytest.mark.parametrize("d,asked", sorted(CASES))
def test_every_byte_of_the_shadow(hip, d, asked):
	bits, steps, live, tile_bytes = CASES[(d, asked)]
	x = rows_of(d)
	with bc.Env(VK_BOUND_PASS="force", VK_BOUND_BITS=asked):
		c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=d, n_tokens=N_ROWS, n_sentences=len(OFF) - 1)
		c.append_vectors(synth.to_bf16_bits(x), normalize=False)   # stored as given
		c.set_sentences(OFF)
		c.finalize()
	try:
		fmt, N, X, got = bc.shadow_of(hip, c)
		assert fmt == dict(bits=bits, steps=steps, live=live, tile_bytes=tile_bytes, tiles=4), fmt
		want, n_max, a_max, codes, meta = restated(x, bits, steps, live)
		assert got.shape == want.shape == (4, tile_bytes)
		# the inputs are what the module's text says: ties on the grid in use, a scale of exactly 1 on its tie row
		tie = 17 if bits == 6 else 18
		assert meta[tie, 0] == 1 and meta[5, 0] == 0 and meta[5, 1] == 0 and 0 < meta[33, 0] < 1e-20
		body = tile_bytes - 128
		for t in range(4):
			diff = np.flatnonzero(got[t, :body] != want[t, :body])
			assert len(diff) == 0, (t, diff[:8], got[t, diff[:8]], want[t, diff[:8]])          # the codes, in tile order
			g, w = got[t, body:].view(np.uint32).reshape(16, 2), want[t, body:].view(np.uint32).reshape(16, 2)
			assert (g == w).all(), (t, [(i, "%08x %08x" % tuple(g[i]), "%08x %08x" % tuple(w[i])) for i in np.flatnonzero((g != w).any(axis=1))])
		assert N.view(np.uint32) == F(n_max).view(np.uint32) and X.view(np.uint32) == F(a_max).view(np.uint32), (N, n_max, X, a_max)
		# zeros: features past d (restated() left them zero and the bytes agree), the rows past the corpus, the tile behind it
		assert (codes[:, d:] == 0).all() and (codes[N_ROWS:] == 0).all() and (meta[N_ROWS:] == 0).all() and not got[3].any()
		if bits == 8:
			lanes = got[2, :body].reshape(steps, 4, 16, 16)          # [block, quarter, row, byte]
			assert not lanes[:, :, N_ROWS - 32:].any()
		# a range of tiles is the same bytes
		_, _, _, part = bc.shadow_of(hip, c, 1, 2)
		assert (part == got[1:3]).all()
	finally:
		c.close()
