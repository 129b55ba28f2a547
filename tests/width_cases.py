"""The width table of the width sweep (test_gpu_widths.py, test_widths_host.py) and the inputs both run on.

Every kernel family picks its form from (nk32, tail, prec) (vk_corpus.cpp): d_pad = ceil(d / 16) * 16; bf16 rows take
nk32 = ceil(d_pad / 32) K-steps of 32 features, the last one a half block (tail = 1) when d_pad % 32 == 16; fp32 rows take
nk32 = d_pad / 16 blocks of 16 features and no tail.  The static layout gathers from a similarity table over the vocabulary
(MODE 2), so only the table kernel and the canonical restatement see its width.

The rows are tail-heavy: the live features of the last block of 16 carry half of a row's squared norm, so a kernel that drops,
pads wrongly or counts twice anything of that block moves every cosine by far more than any tolerance
(test_widths_host.py proves that on the oracle alone)."""

import numpy as np

# width: (nk32, tail), the arm it is the edge of.  bf16 contextual rows:
BF16_WIDTHS = {
	5:    ((1, 1), "d < 16: the tile is a single half block (nfull == 0); vk_doc's register form loads block 0"),
	113:  ((4, 0), "d_pad 128 with 15 padded features: vk_rwmd_batch<4>, MODE 1, 113 % 4 == 1"),
	127:  ((4, 0), "d_pad 128 with one padded feature: vk_rwmd_batch<4>; below the stream_cap arm"),
	200:  ((7, 1), "upper edge of nk32 5..7 (stream_cap = 4 in launch_sized), MODE 1 with a half block"),
	225:  ((8, 1), "nk32 == 8 with a half block: lower edge of MODE 5, 8-deep loop of sim_tile_generic never entered"),
	288:  ((9, 0), "d_pad 288: MODE 5, must NOT take the (10,1) forms nor build a shadow"),
	289:  ((10, 1), "d_pad 304 with 15 padded features, 289 % 4 == 1: MODE 0 / MODE 3-300, <10,true> arms, shadow and bound pass"),
	303:  ((10, 1), "d_pad 304 with one padded feature: the (10,1) forms"),
	304:  ((10, 1), "d_pad 304 without padding in the half block: the (10,1) forms"),
	305:  ((10, 0), "d_pad 320: MODE 5, must NOT take the (10,1) forms nor build a shadow; shared pass at nk32 == 10"),
	368:  ((12, 1), "NKP = 12 with a half block: register forms of vk_doc / vk_docw / vk_flow; shared pass refuses nk32 > 10"),
	384:  ((12, 0), "NKP = 12 without a half block; launch_span<12>"),
	385:  ((13, 1), "nk32 == 13: the generic arm of vk_doc / vk_docw / vk_flow starts here"),
	512:  ((16, 0), "an encoder's width: MODE 5, 8-deep loop entered twice"),
	753:  ((24, 0), "d_pad 768 with 15 padded features: MODE 3, vk_rwmd_batch<24>, launch_span<24>, wide32"),
	767:  ((24, 0), "d_pad 768 with one padded feature: the (24,0) forms"),
	769:  ((25, 1), "just past the (24,0) forms: MODE 5 again"),
	1024: ((32, 0), "an encoder's width: launch_span<32>; beyond every measured tolerance"),
	# vk_query.cpp stages the query tile in LDS only if 2 * (smem + qb) <= 160 KiB, qb = ceil(32 d_pad / 1024) KiB: from d_pad = 2560 on
	# 2 * qb alone is 160 KiB, so with any strip at all (smem > 0) q_lds == 0 for every query; 2570 -> d_pad 2576, qb = 81 KiB
	2570: ((81, 1), "q_lds == 0 (the query tile is read through the caches), plan32.fits == false, with a half block"),
	8192: ((256, 0), "the API's maximum (corpus of 60 slices)"),
}
# fp32 rows (nk32 = d_pad / 16, no tail)
F32_WIDTHS = {
	5:    ((1, 0), "a single block of 16"),
	200:  ((13, 0), "MODE 6 with 8 padded features"),
	288:  ((18, 0), "MODE 6: must NOT take MODE 4"),
	289:  ((19, 0), "MODE 4 (nk32 == 19) with 15 padded features, sim_canon16's trailing loop"),
	304:  ((19, 0), "MODE 4 without padding"),
	305:  ((20, 0), "MODE 6: must NOT take MODE 4"),
	# (qb = 64 KiB: 2 * (smem + qb) <= 160 KiB holds only while the four waves' strips stay under 16 KiB -- the 1-token query (lt = 4);
	# the 7- and 16-token queries run with q_lds == 0)
	1024: ((64, 0), "an encoder's width; the query tile is staged in LDS for the 1-token query only"),
}
# static layout (bf16 vocabulary; the token pass is MODE 2 at every width)
STATIC_WIDTHS = {
	5:    ((1, 1), "table kernel over a single half block"),
	289:  ((10, 1), "table kernel at the (10,1) edge, 289 % 4 == 1"),
	385:  ((13, 1), "no GEMM form for the batch: the table kernel takes any width"),
	1024: ((32, 0), "an encoder's width"),
}
TABLES = {"bf16": BF16_WIDTHS, "f32": F32_WIDTHS, "static": STATIC_WIDTHS}
for _layout, _table in TABLES.items():
	for _d, ((_nk, _tail), _) in _table.items():
		_pad = (_d + 15) // 16 * 16
		assert (_nk, _tail) == ((_pad // 16, 0) if _layout == "f32" else ((_pad + 31) // 32, int(_pad % 32 != 0))), (_layout, _d)

# Widths that run on a small corpus of slices of at most 40 tokens.  60 slices and not fewer: with 20, the winners at k = 10 are half of
# the live slices, and whether counting the tail twice changes that set (test_widths_host.py demands it) was a coin toss per corpus
# (8 of 12 corpora tried); with 60, 22 of 24 -- it is never certain, the order of the slices can survive that mutation -- and the one
# committed here, seeded like every other width, meets it.
SMALL = {8192}
SMALL_SLICES = 60
VOCAB = 400             # static layout


def d_pad(d):
	return (d + 15) // 16 * 16


def tol(d, project):
	"""tolerance of last_scores() against the oracle: the project's value (1e-4 alignments, 2e-5 relaxed WMD; held by the suite up to
	768 features), and beyond 768 features, where neither was ever measured, 2 d_pad 2^-24 + 2e-5 if that is larger: DESIGN 11.6's
	gamma (fp32 accumulation of d_pad products of unit rows) plus the exact kernel's own rounding"""
	p = d_pad(d)
	return project if p <= 768 else max(project, 2 * p * 2.0 ** -24 + 2e-5)


def tail_start(d):
	"""first feature of the last block of 16"""
	return 16 * ((d - 1) // 16)


def tail_heavy(G):
	"""rows whose last block of 16 features carries half of the squared norm (d <= 16: the row is its last block), and in that block
	the last live feature as much as the others together: a cosine then moves by about a quarter when that one feature is lost,
	whatever the width and its tolerance, and by a sixtieth for any other feature of the block"""
	G = np.array(G, dtype=np.float64)
	d = G.shape[1]
	t0 = tail_start(d)
	if t0 > 0:
		head = (G[:, :t0] ** 2).sum(axis=1)
		tail = (G[:, t0:] ** 2).sum(axis=1)
		G[:, t0:] *= np.sqrt(head / np.maximum(tail, 1e-30))[:, None]
	if d - t0 > 1:
		rest = (G[:, t0:d - 1] ** 2).sum(axis=1)
		last = G[:, d - 1] ** 2
		G[:, t0:d - 1] *= np.sqrt((rest + last) / 2 / np.maximum(rest, 1e-30))[:, None]
		G[:, d - 1] *= np.sqrt((rest + last) / 2 / np.maximum(last, 1e-30))
	return G.astype(np.float32)


def with_common_direction(G, rng):
	"""standard normal rows plus, on the features before the last block, one common standard normal direction with a standard normal
	coefficient per row.  Without it the cosines of the heads shrink as 1 / sqrt(d) while those of the tails do not: the order of the
	slices is then the order of their tail cosines alone, and counting the tail twice (mutation 'double' of test_widths_host.py) scales
	every score without changing a winner.  With it head and tail cosines spread alike at every width, and every feature stays live."""
	t0 = tail_start(G.shape[1])
	if t0 > 0:
		G[:, :t0] += rng.standard_normal((G.shape[0], 1)) * rng.standard_normal((1, t0))
	return G


def slice_lengths(d, rng):
	"""about 240 slices of 0..40 tokens (empty ones among them), two of 65..200, one of about 700 as the LAST slice: the last tile of
	the buffer belongs to a long slice.  n_short: the leading slices of at most 40 tokens."""
	if d in SMALL:
		lens = rng.integers(0, 41, size=SMALL_SLICES)
		lens[[3, 11]] = (0, 40)
		return lens, SMALL_SLICES
	lens = rng.integers(0, 41, size=243)
	lens[[0, 7, 100, 239]] = 0
	lens[[1, 50]] = (40, 16)
	lens[240:] = (int(rng.integers(65, 201)), int(rng.integers(65, 201)), 697)
	return lens, 240


class Case:
	"""the inputs of one (layout, width): raw rows (tail-heavy, not normalised), slices, and planted queries"""

	def __init__(self, layout, d):
		self.layout, self.d = layout, d
		rng = np.random.default_rng(1000 * d + {"bf16": 0, "f32": 1, "static": 2}[layout])
		self.lens, self.n_short = slice_lengths(d, rng)
		self.off = np.concatenate(([0], np.cumsum(self.lens))).astype(np.int64)
		self.n = len(self.lens)
		T = int(self.off[-1])
		if layout == "static":
			self.raw = tail_heavy(with_common_direction(rng.standard_normal((VOCAB, d)), rng))       # the vocabulary
			self.tok_id = rng.integers(0, VOCAB, size=T).astype(np.int32)
		else:
			self.raw = tail_heavy(with_common_direction(rng.standard_normal((T, d)), rng))
			self.tok_id = None
		self.rng = rng

	def token_rows(self):
		return self.raw if self.tok_id is None else self.raw[self.tok_id]

	def place(self, len_t, seed=0, among_short=False):
		"""(first token, tokens) of the stretch a query copies: up to len_t tokens in the middle of a slice that holds as many (the
		seed-th such slice; among the leading short slices if asked: a corpus may end with them), else of the longest slice"""
		lens = self.lens[:self.n_short] if among_short else self.lens
		fit = np.flatnonzero(lens >= len_t)
		s = int(fit[seed % len(fit)]) if len(fit) else int(np.argmax(lens))
		m = min(len_t, int(lens[s]))
		return int(self.off[s]) + (int(lens[s]) - m) // 2, m

	def query(self, len_t, seed=0, among_short=False):
		"""a noisy copy of len_t consecutive tokens of a slice (place), padded with fresh rows when no slice holds as many.  Static
		layout: the vectors only (static_ids has the ids)."""
		rng = np.random.default_rng(7919 * self.d + 31 * len_t + seed)
		a, m = self.place(len_t, seed, among_short)
		q = noisy_copy(self.token_rows()[a:a + m], rng)
		if m < len_t:
			q = np.concatenate((q, tail_heavy(rng.standard_normal((len_t - m, self.d)))))
		return q

	def static_ids(self, len_t, seed=0):
		"""ids of a static query: the tokens query() copies, one id repeated, the last id -1 (a word the vocabulary does not hold)"""
		a, m = self.place(len_t, seed)
		assert m == len_t
		ids = self.tok_id[a:a + len_t].copy()
		if len_t > 3:
			ids[3] = ids[0]
		if len_t > 1:
			ids[-1] = -1
		return ids


def noisy_copy(src, rng, level=0.3):
	"""rows plus noise in the proportions of the rows themselves: standard normal rows made tail-heavy, at `level` of each row's norm"""
	src = np.asarray(src, dtype=np.float64)
	noise = tail_heavy(rng.standard_normal(src.shape)).astype(np.float64)
	noise *= (np.linalg.norm(src, axis=1) / np.linalg.norm(noise, axis=1))[:, None]
	return (src + level * noise).astype(np.float32)


def mutate(stored, d, kind):
	"""stored unit rows (bf16 bits or fp32) as a kernel with a tail bug would see them: 'zero' -- the last live feature dropped;
	'double' -- the live features of the last block of 16 counted twice (both exact in either format)"""
	is_bits = stored.dtype == np.uint16
	x = (stored.astype(np.uint32) << 16).view(np.float32).copy() if is_bits else stored.copy()
	if kind == "zero":
		x[:, d - 1] = 0.0
	elif kind == "double":
		x[:, tail_start(d):] *= 2.0
	else:
		raise ValueError(kind)
	return (x.view(np.uint32) >> 16).astype(np.uint16) if is_bits else x
