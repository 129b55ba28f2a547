"""Shared by the tests of the 6-bit bound pass: the E2M3 grid and the quantizer of vk_host::quantize_row_e2m3 restated in
numpy, the packing of a tile, and the limits the GPU tests hold the pass against (delta_6 and round2_limit, from the restatement)."""

import numpy as np

from vectorian_amd import synth

F = np.float32

# the grid as DESIGN 11.8 states it: 0 .. 1.875 in steps of 0.125, 2 .. 3.75 in steps of 0.25, 4 .. 7.5 in steps of 0.5
GRID = np.concatenate([np.arange(0, 2, 0.125), np.arange(2, 4, 0.25), np.arange(4, 8, 0.5)])
assert len(GRID) == 32 and GRID[31] == 7.5
EIGHTHS = np.concatenate([(GRID * 8), -(GRID * 8)]).astype(np.int64)   # by code: bit 5 the sign


def up(v):
	"""non-negative doubles rounded UP to float32 (quant_up)"""
	v = np.asarray(v, dtype=np.float64)
	f = np.nextafter((v * (1.0 + 1e-6)).astype(F), F(np.inf))
	return np.where(v > 0, f, F(0)).astype(F)


def quantize6(x):
	"""x: float32 rows.  (codes uint8, s, e >= |x - s x^|, n >= |s x^|, a >= |x|) per row as the library computes them: float32
	where it uses floats, sums in double in k order, rounded up"""
	x = np.ascontiguousarray(x, dtype=F)
	m = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(len(x), dtype=F)
	s = (m / F(7.5)).astype(F)
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
	return codes, s, up(np.sqrt(seq(dd * dd))), up(np.sqrt(seq(xs * xs))), up(np.sqrt(seq(x.astype(np.float64) ** 2)))


def values(codes, s):
	"""the rows the codes stand for, s x^, in double"""
	return s.astype(np.float64)[:, None] * (EIGHTHS[codes] / 8.0)


def constants(s, e, a, N, X):
	"""cs, ca, cb of a query column (vk_host::bound_cell_constants with the exact kernel's d_pad = 320)"""
	gamma = 2.0 * 320 * 2.0 ** -24 * a.astype(np.float64) * float(X) + 2e-6
	return s, a, up(e.astype(np.float64) * float(N) + gamma)


def pack_tile(codes, live6):
	"""codes: 16 rows x 384 codes -> the bytes of the tile's K-steps as the issue lays them out: lane l = 16 g + i holds row i,
	features 128 t + 32 g + j at bits 6 j .. 6 j + 5 of 24 bytes; a K-step is its lanes' first 16 bytes, then their last 8; the last
	K-step holds live6 quarters only"""
	out = []
	for t in range(3):
		quarters = 4 if t < 2 else live6
		lo = np.zeros((16 * quarters, 16), dtype=np.uint8)
		hi = np.zeros((16 * quarters, 8), dtype=np.uint8)
		for g in range(quarters):
			for i in range(16):
				word = 0
				for j in range(32):
					word |= int(codes[i, 128 * t + 32 * g + j] & 63) << (6 * j)
				b = np.frombuffer(word.to_bytes(24, "little"), dtype=np.uint8)
				lo[16 * g + i], hi[16 * g + i] = b[:16], b[16:]
		out += [lo.reshape(-1), hi.reshape(-1)]
	return np.concatenate(out)


def stored(x):
	"""unit rows as the corpus stores them: normalised, rounded to bf16"""
	return synth.bf16_bits_to_f32(synth.to_bf16_bits(synth.normalize_rows(x)))


def corpus_terms(X_stored):
	"""(the largest e_x, N, X) of a corpus, each with a relative 1e-5 on top of the library's rounding up: compute once per corpus"""
	_, _, e_x, n_x, a_x = quantize6(X_stored)
	return float(e_x.max()) * (1 + 1e-5), float(n_x.max()) * (1 + 1e-5), float(a_x.max()) * (1 + 1e-5)


def delta6(terms, q_stored):
	"""The most a cell of the 6-bit bound exceeds the exact cosine (DESIGN 11.6 with this quantizer): 2 max (e_x a_q + e_q N) + gamma +
	2e-5, the terms at their largest over corpus (corpus_terms) and query"""
	e_x, N, X = terms
	_, _, e_q, _, a_q = quantize6(q_stored)
	e_q, a_q = e_q.astype(np.float64) * (1 + 1e-5), a_q.astype(np.float64) * (1 + 1e-5)
	gamma = 2 * 320 * 2.0 ** -24 * a_q * X + 2e-6
	return float((2 * (e_x * a_q + e_q * N) + gamma).max()) * (1 + 1e-5) + 2e-5


def round2_limit(delta, full, k, n, min_score):
	"""the most slices round 2 can hold, from the exact scores `full` and delta (as tests/test_gpu_bound_pass.py)"""
	floor = min_score - 1e-5 * max(1.0, abs(min_score))
	kk = min(k + 8, n)
	above = np.sort(full[full > floor])[::-1]
	if len(above) >= kk and above[kk - 1] - delta > floor:
		return int((full >= above[kk - 1] - 2 * delta).sum())
	return int((full > floor - delta).sum())
