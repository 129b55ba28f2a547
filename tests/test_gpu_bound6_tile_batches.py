"""-m gpu: the 6-bit bound kernel's tile loop, several tiles per trip, on corpora laid out to reach every shape of a trip.
The kernel takes the tiles of a group of four slices VK_FP6_TILES at a time (two), all their loads ahead of the first MFMA, and what is
left of the group one tile per trip; the first tile of a group is carried over from the previous group of the wave's run when both
share it (ti0 = 1), which may leave no tile to compute at all.  Two corpora of fewer than 1,000 slices, built with VK_BOUND_PASS=force
VK_BOUND_BITS=6 at d = 300 -- below 1,024 slices round 2 cannot reach the fallback line max(n / 16, 1024), so every case asserts that
no fallback happened:
  `short`: slices of 0 .. 32 tokens (general gaps run the 32-row history, GAP 3), groups of 1 .. 9 tiles;
  `long`:  slices of 0 .. 64 tokens, some above 32 (the 64-row history, GAP 6, which keeps one tile per trip), groups of 1 .. 17 tiles;
both with empty slices and a last group of fewer than four.  groups_of() restates how the kernel walks the groups (runs of VK_RUN = 4
groups, the carried tile), and the fixtures assert from it that the layout holds every tile count, both parities of what is left after
the carried tile, with and without one, and a group whose only tile is the carried one.
Per query (4, 8, 10 and 16 tokens; linear, affine and general gaps; local and global alignment; k = 1 and 10) the claims (a), (b), (c),
(e) of tests/test_gpu_bound6_pass.py hold against a VK_BOUND_PASS=off handle of the same vectors.
Shift invariance: the same slices behind a prefix of 1, 7 and 15 tokens (one, two and three extra slices, copies of the corpus's own
first rows, so that the corpus-wide N and X are the same -- asserted) land at other rows of other tiles in other groups; the bound
of a slice depends on neither, so every shared slice's bound is the same bit pattern.  A tile written to the wrong strip rows, a
stale row or a dropped tile at the end of a group changes it."""

import numpy as np
import pytest

import bound_cases as bc
from bound_cases import case_queries, state
from test_gpu_bound6_pass import EXP5, GAPS, Pair, _Env, check
from vectorian_amd import synth

pytestmark = pytest.mark.gpu

D, V = 300, 5_000
RUN, T = 4, 2   # VK_RUN and VK_FP6_TILES of vk_common.hip.h


def lengths(top, seed):
	"""slice lengths of 0 .. top tokens: four equal slices of every length (groups of 4 .. 4 top tokens at whatever place in their first
	tile the layout before them leaves), two runs of one-token slices with empty ones (groups inside one tile), and drawn lengths"""
	rng = np.random.default_rng(seed)
	parts = [np.repeat(np.arange(1, top + 1), 4)]
	parts.append(np.array([1, 1, 0, 1] * 12 + [0, 0, 0, 0] + [1, 2, 1, 1] * 8))
	parts.append(rng.integers(0, top + 1, size=240))
	parts.append(np.full(37, top))                         # whole groups of the longest slices, then a last group of one
	parts.append(rng.integers(0, 4, size=64))
	lens = np.concatenate(parts)
	lens = np.concatenate([lens, [3] * ((5 - len(lens) % 4) % 4)])   # n % 4 == 1
	return lens.astype(np.int64)


def groups_of(off):
	"""[(tiles of the group, 1 if its first tile is carried over else 0)] as vk_score_kernel walks them: runs of RUN groups of four slices"""
	n = len(off) - 1
	out = []
	for g in range((n + 3) // 4):
		if g % RUN == 0:
			prev = -1
		g_a, g_b = int(off[min(4 * g, n)]), int(off[min(4 * g + 4, n)])
		tile0 = g_a >> 4
		ntiles = ((g_b + 15) >> 4) - tile0
		ti0 = int(ntiles > 0 and tile0 == prev)
		if ntiles > 0:
			prev = tile0 + ntiles - 1
		out.append((ntiles, ti0))
	return out


def layout(top, seed):
	lens = lengths(top, seed)
	off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
	n = len(lens)
	assert n < 1000 and n % 4 in (1, 2, 3) and (lens == 0).sum() >= 8 and lens.max() == top
	groups = groups_of(off)
	most = (4 * top + 15) // 16 + 1
	assert {nt for nt, _ in groups} >= set(range(1, most + 1)), sorted({nt for nt, _ in groups})
	left = {(ti0, (nt - ti0) % T) for nt, ti0 in groups if nt - ti0 > 0}
	assert left == {(c, r) for c in (0, 1) for r in range(T)}, left           # both parities of the remainder, with and without a carried tile
	assert (1, 1) in groups                                                    # the carried tile is the group's only one
	assert any(nt - ti0 >= 2 * T + 1 for nt, ti0 in groups)                    # several whole trips and a remainder
	return off


def corpus_with(off, seed):
	"""a contextual corpus of off[-1] token rows in the slices off (rows as synth draws them, one token per row)"""
	corpus = synth.make_contextual_corpus(int(off[-1]), 1, 1, V, D, seed=seed)
	corpus["sent_off"] = off
	return corpus


@pytest.fixture(scope="module")
def short(hip):
	p = Pair(hip, corpus_with(layout(32, 3), seed=61))
	yield p
	p.close()


@pytest.fixture(scope="module")
def long(hip):
	p = Pair(hip, corpus_with(layout(64, 4), seed=62))
	assert (np.diff(p.off) > 32).sum() > 100
	yield p
	p.close()


@pytest.mark.parametrize("gap", sorted(GAPS))
@pytest.mark.parametrize("shape", ("short", "long"))
def test_pruned_query_is_the_exact_query(hip, request, shape, gap):
	pair = request.getfixturevalue(shape)
	gs, gt = GAPS[gap]
	for len_t in (4, 8, 10, 16):
		for qv in case_queries(pair.corpus, len_t):
			for locality in (hip.Locality.LOCAL, hip.Locality.GLOBAL):
				for k in (1, 10):
					cnt = check(hip, pair, qv, strict=True, locality=int(locality), gap_s=gs, gap_t=gt, max_matches=k,
						min_score=0.0 if int(locality) == 0 else -1e9)
					assert cnt[3] == 0, cnt


def shifted(pair, p):
	"""the pair's slices behind p prefix tokens in one slice per started five (1 -> 1, 7 -> 3 + 4, 15 -> 5 + 5 + 5): (X, off, slices added)"""
	cuts = {1: [1], 7: [3, 7], 15: [5, 10, 15]}[p]
	X = np.concatenate([pair.X[:p], pair.X])
	off = np.concatenate([[0], cuts, pair.off[1:] + p]).astype(np.int64)
	return X, off, len(cuts)


def bounds_of(hip, c, qv, **kw):
	with _Env("force"):
		c.query(qv, **kw)
		ub, cnt = state(hip, c)
	assert cnt[0] == 1 and cnt[3] == 0, cnt
	return ub


@pytest.mark.parametrize("prefix", (1, 7, 15))
@pytest.mark.parametrize("shape", ("short", "long"))
def test_a_bound_does_not_depend_on_the_place_in_the_tile(hip, request, shape, prefix):
	pair = request.getfixturevalue(shape)
	X, off, added = shifted(pair, prefix)
	assert groups_of(off) != groups_of(pair.off)
	with _Env("force"):
		moved = bc.corpus_of(hip, X, off)
	try:
		_, N0, X0, _ = bc.shadow_of(hip, pair.forced, 0, 1)
		fmt, N1, X1, _ = bc.shadow_of(hip, moved, 0, 1)
		assert fmt["bits"] == 6
		assert np.float32(N0).view(np.uint32) == np.float32(N1).view(np.uint32) and np.float32(X0).view(np.uint32) == np.float32(X1).view(np.uint32)
		for len_t in (10, 16):
			qv = case_queries(pair.corpus, len_t)[0]
			for gap in sorted(GAPS):
				gs, gt = GAPS[gap]
				for locality in (hip.Locality.LOCAL, hip.Locality.GLOBAL):
					kw = dict(locality=int(locality), gap_s=gs, gap_t=gt, max_matches=10, min_score=0.0 if int(locality) == 0 else -1e9)
					here = bounds_of(hip, pair.forced, qv, **kw)
					there = bounds_of(hip, moved, qv, **kw)
					same = here.view(np.uint32) == there[added:].view(np.uint32)
					assert same.all(), (shape, prefix, len_t, gap, int(locality), np.flatnonzero(~same)[:8])
	finally:
		moved.close()
