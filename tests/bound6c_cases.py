"""Shared by the tests of the compact 6-bit shadow: the quantizer of vk_host::quantize_row<grid_e2m3>(.., bf16_meta)
restated in numpy (s and e rounded UP to bf16, the codes computed with that s), the packing of a compact tile (3,712 bytes: two
whole K-steps, part P, part Q, sixteen words of (s, e)), and the terms of delta for the GPU tests.  The grid, up() and round2_limit are
tests/bound6_cases.py's."""

import numpy as np

import bound6_cases as b6

F = np.float32
TILE, META, STEP = 3712, 3648, 1536


def bf16_up(v):
	"""the least bf16 value >= v (v >= 0), as float32"""
	u = np.ascontiguousarray(v, dtype=F).view(np.uint32).astype(np.uint64)
	u = np.where(u & 0xffff, (u | 0xffff) + 1, u)
	return u.astype(np.uint32).view(F)


def quantize6c(x):
	"""x: float32 rows.  (codes uint8, s, e, n, a) per row as the library computes them under bf16_meta: s = bf16_up(max|x| / 7.5), the
	codes and the sums with that s, e = bf16_up(up(|x - s x^|))"""
	x = np.ascontiguousarray(x, dtype=F)
	m = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(len(x), dtype=F)
	s = bf16_up((m / F(7.5)).astype(F))
	safe = np.where(s > 0, s, F(1)).astype(F)
	t = np.minimum(F(7.5), np.abs((x / safe[:, None]).astype(F)))
	step = np.where(t < 2, F(0.125), np.where(t < 4, F(0.25), F(0.5))).astype(F)
	a = np.minimum(F(7.5), np.rint(t / step) * step).astype(F)
	a = a * (s > 0)[:, None]
	n8 = (a * 8).astype(np.int64)
	mag = np.where(n8 < 16, n8, np.where(n8 < 32, 16 + ((n8 - 16) >> 1), 24 + ((n8 - 32) >> 2)))
	codes = (mag | np.where((x < 0) & (mag != 0), 32, 0)).astype(np.uint8)
	v = np.where(x < 0, -a, a).astype(np.float64)
	xs = s.astype(np.float64)[:, None] * v
	dd = x.astype(np.float64) - xs
	seq = lambda t: np.cumsum(t, axis=1)[:, -1] if t.shape[1] else np.zeros(len(t))   # sequential, as the C loop
	return codes, s, bf16_up(b6.up(np.sqrt(seq(dd * dd)))), b6.up(np.sqrt(seq(xs * xs))), b6.up(np.sqrt(seq(x.astype(np.float64) ** 2)))


def lane_words(codes32):
	"""32 codes -> the lane's 24 bytes: code j at bits 6 j .. 6 j + 5"""
	word = 0
	for j in range(32):
		word |= int(codes32[j] & 63) << (6 * j)
	return np.frombuffer(word.to_bytes(24, "little"), dtype=np.uint8)


def pack_tile_c(codes, s, e):
	"""codes: 16 rows x 384 codes (zeros from 304 on), s / e: 16 bf16-valued floats -> the 3,712 bytes of a compact tile: K-steps 0 and
	1 as bound6_cases.pack_tile lays them out; the last one part P, 32 lanes x 12 bytes (lane 16 g + i: bytes 0 .. 11 of row i's quarter
	g, g = 0, 1), then part Q, 16 lanes x 12 bytes (bytes 12 .. 23 of quarter 0); then per row one word, s's bf16 in the low half"""
	assert codes.shape == (16, 384) and not codes[:, 304:].any()
	whole = b6.pack_tile(codes, 0)
	assert len(whole) == 2 * STEP
	P = np.zeros((32, 12), dtype=np.uint8)
	Q = np.zeros((16, 12), dtype=np.uint8)
	for g in range(2):
		for i in range(16):
			b = lane_words(codes[i, 256 + 32 * g:256 + 32 * g + 32])
			P[16 * g + i] = b[:12]
			if g == 0:
				Q[i] = b[12:]
			else:
				assert not b[12:].any()
	su, eu = np.ascontiguousarray(s, dtype=F).view(np.uint32), np.ascontiguousarray(e, dtype=F).view(np.uint32)
	assert not (su & 0xffff).any() and not (eu & 0xffff).any()
	meta = ((su >> 16) | eu).astype(np.uint32)
	out = np.concatenate([whole, P.reshape(-1), Q.reshape(-1), meta.view(np.uint8)])
	assert len(out) == TILE
	return out


def corpus_terms(X_stored):
	"""(the largest e_x, N, X) of a corpus under the compact quantizer, each with a relative 1e-5 on top (as bound6_cases.corpus_terms)"""
	_, _, e_x, n_x, a_x = quantize6c(X_stored)
	return float(e_x.max()) * (1 + 1e-5), float(n_x.max()) * (1 + 1e-5), float(a_x.max()) * (1 + 1e-5)
