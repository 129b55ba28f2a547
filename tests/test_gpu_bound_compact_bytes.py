"""-m gpu: every byte of a corpus's compact 6-bit shadow (VK_BOUND_PASS=force VK_BOUND_BITS=6c), read back from the
device through vk_bound_pass_shadow, against the numpy statement the CPU tier holds the host's quantizer and packer against
(tests/bound6c_cases.py, tests/test_bound_compact_host.py): the codes in the tile's order -- two whole K-steps, part P, part Q --,
one word of (s_x, e_x) as two bf16 per row, N and X of the corpus, zeros for the rows past the corpus and for the tile behind it; the
handle reports 6 bits, three K-steps, two live quarters and 3,712 bytes a tile.  Corpora of 64 tokens (four whole tiles) and of 40
tokens in ragged slices (two whole tiles and one of eight rows), at 289, 300, 303 and 304 features; among the rows one of zeros, one
whose largest element is negative, one on the midpoints of the E2M3 steps with s = 1, one of magnitudes around 1e-20.
VK_BOUND_BITS=6 still builds the 3,968-byte tiles."""

import numpy as np
import pytest

import bound6_cases as b6
import bound6c_cases as b6c
import bound_cases as bc
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

F = np.float32
TIES6 = np.array([7.5, 0.0625, 0.1875, -0.3125, 1.9375, 2.125, 2.375, -3.875, 4.25, 4.75, 7.25, -7.5, 0.0, 3.75, -1.875, 0.125], dtype=F)
SHAPES = {"whole": (64, np.array([0, 16, 17, 48, 64], dtype=np.int64)), "ragged": (40, np.array([0, 13, 14, 40], dtype=np.int64))}


def rows_of(d, n):
	rng = np.random.default_rng(7 * d + n)
	x = b6.stored(rng.standard_normal((n, d)).astype(F))
	x[5] = 0.0
	x[9, d // 3] = -0.75
	x[17] = 0.0; x[17, :8] = TIES6[:8]; x[17, d - 8:] = TIES6[8:]
	x[33] = synth.bf16_bits_to_f32(synth.to_bf16_bits(F(1e-20) * x[33]))
	assert (synth.bf16_bits_to_f32(synth.to_bf16_bits(x)) == x).all()
	return x


def corpus_of(hip, x, off, bits):
	with bc.Env(VK_BOUND_PASS="force", VK_BOUND_BITS=bits):
		c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=x.shape[1], n_tokens=len(x), n_sentences=len(off) - 1)
		c.append_vectors(synth.to_bf16_bits(x), normalize=False)
		c.set_sentences(off)
		c.finalize()
	return c


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("d", (289, 300, 303, 304))
def test_every_byte_of_the_compact_shadow(hip, d, shape):
	n, off = SHAPES[shape]
	x = rows_of(d, n)
	c = corpus_of(hip, x, off, "6c")
	try:
		tiles = (n + 15) // 16 + 1
		fmt, N, X, got = bc.shadow_of(hip, c)
		assert fmt == dict(bits=6, steps=3, live=2, tile_bytes=b6c.TILE, tiles=tiles), fmt
		rc, rs, re, rn, ra = b6c.quantize6c(x)
		codes = np.zeros((16 * tiles, 384), dtype=np.uint8)
		s, e = np.zeros(16 * tiles, dtype=F), np.zeros(16 * tiles, dtype=F)
		codes[:n, :d], s[:n], e[:n] = rc, rs, re
		assert s[17] == 1 and s[5] == 0 and e[5] == 0 and 0 < s[33] < 1e-20
		assert got.shape == (tiles, b6c.TILE)
		for t in range(tiles):
			r = slice(16 * t, 16 * t + 16)
			want = b6c.pack_tile_c(codes[r], s[r], e[r])
			diff = np.flatnonzero(got[t] != want)
			assert len(diff) == 0, (t, diff[:8], got[t, diff[:8]], want[diff[:8]])
		assert N.view(np.uint32) == F(rn.max()).view(np.uint32) and X.view(np.uint32) == F(ra.max()).view(np.uint32), (N, rn.max(), X, ra.max())
		assert not got[tiles - 1].any()                              # the zero tile behind the corpus
		if n % 16:
			assert not codes[n:].any() and not got[tiles - 2, b6c.META + 4 * (n % 16):].any()   # the rows past the corpus
		_, _, _, part = bc.shadow_of(hip, c, 1, 2)
		assert (part == got[1:3]).all()
	finally:
		c.close()


def test_six_without_the_c_keeps_the_wide_tiles(hip):
	n, off = SHAPES["ragged"]
	x = rows_of(300, n)
	c = corpus_of(hip, x, off, "6")
	try:
		fmt, _, _, got = bc.shadow_of(hip, c)
		assert fmt == dict(bits=6, steps=3, live=2, tile_bytes=3968, tiles=4), fmt
		rc, rs, re, _, _ = b6.quantize6(x)
		codes = np.zeros((16, 384), dtype=np.uint8)
		codes[:, :300] = rc[:16]
		assert (got[0, :3840] == b6.pack_tile(codes, 2)).all()
		assert (got[0, 3840:].view(F).reshape(16, 2) == np.stack([rs[:16], re[:16]], axis=1)).all()
	finally:
		c.close()
