"""The reader of test_gpu_batch_every_slice.py cannot hide a wrong cell: on a numpy stand-in for query_batch over a known matrix,
batch_windows.read_matrix returns that matrix bit for bit, and each way a batch kernel could be wrong in one cell -- off by twice the
tolerance, sign flipped, dropped, a slice leaked from outside the window, a live slice written as empty -- fails assert_matrix or the
reader's own assertions.  No GPU and no library: the same idea as test_widths_host.py."""

import types

import numpy as np
import pytest

import batch_windows as bw

TOL = 2e-5
N_Q = 7


class StandIn:
	"""query_batch as vk_batch.cpp answers it without flows: score = cell * boost (an empty slice stays -inf), admitted iff
	score > min_score, the 64 best by (score descending, index descending).  scores: what the 'kernel' wrote; the hooks change what
	the batch returns: drop = (query, slice) never returned, leak = (query, slice, value) returned from every window."""

	def __init__(self, scores, drop=None, leak=None):
		self.scores, self.drop, self.leak = np.asarray(scores, dtype=np.float32), drop, leak
		self.calls = 0

	def __call__(self, boost, min_score=0.0, k=64):
		self.calls += 1
		outs = []
		for i, row in enumerate(self.scores):
			with np.errstate(invalid="ignore"):
				val = np.where(np.isneginf(row), row, row * boost).astype(np.float32)
			idx = np.flatnonzero(val > min_score)
			if self.drop is not None and self.drop[0] == i:
				idx = idx[idx != self.drop[1]]
			idx = idx[np.lexsort((-idx, -val[idx]))][:k]
			score = val[idx]
			if self.leak is not None and self.leak[0] == i and boost[self.leak[1]] == 0:
				idx, score = np.append(idx[:k - 1], self.leak[1]), np.append(score[:k - 1], np.float32(self.leak[2]))
			outs.append(types.SimpleNamespace(n=len(idx), sentence=idx.astype(np.int64), score=score.astype(np.float32)))
		return outs


def known_matrix(n, signed, seed=0):
	"""cells of 1e-3 .. 1 in magnitude (both signs when signed), one exact zero per query (+0.0 or -0.0), three empty columns: the first
	slice, one inside a window and the last slice of the partial tail"""
	rng = np.random.default_rng(seed + n)
	S = rng.uniform(1e-3, 1.0, size=(N_Q, n)).astype(np.float32)
	if signed:
		S *= rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=S.shape)
	live = np.ones(n, dtype=bool)
	live[[0, n // 2, n - 1]] = False
	S[:, ~live] = -np.inf
	for i in range(N_Q):
		S[i, 1 + (29 * i) % (n - 3)] = 0.0 if i % 2 else -0.0
	return S, live


def same_bits(a, b):
	return (np.asarray(a, dtype=np.float32).view(np.uint32) == np.asarray(b, dtype=np.float32).view(np.uint32)).all()


@pytest.mark.parametrize("signed", (False, True))
@pytest.mark.parametrize("n", (1037, 191, 192, 193, 63, 64, 65))
def test_reader_returns_the_matrix_bit_for_bit(n, signed):
	S, live = known_matrix(n, signed)
	run = StandIn(S)
	M = bw.read_matrix(run, n, N_Q, signed)
	assert run.calls == (2 if signed else 1) * ((n + 63) // 64)
	nothing = (S == 0) | np.isneginf(S)
	assert (np.isnan(M) == nothing).all()
	assert same_bits(M[~nothing], S[~nothing])
	if n >= 191:      # (one zero per query is within the cap of 1 % from 100 live slices on)
		want = np.where(live[None, :], S, 0.0)
		bw.assert_oracle_cap(want, live, TOL)
		bw.assert_matrix(M, want, live, TOL)


def test_windows_cover_every_slice_once():
	for n in (1, 63, 64, 65, 1037):
		total = np.zeros(n)
		for window, boost in bw.window_boosts(n, -1.0):
			assert len(window) <= 64 and boost.dtype == np.float32
			assert (boost[window.start:window.stop] == -1.0).all() and np.count_nonzero(boost) == len(window)
			total += boost
		assert (total == -1.0).all()


# (query, slice) of the wrong cell: the third query slot at the last slice of a full window, the first slice of the partial tail,
# a cell in the middle
CELLS = ((2, 63), (5, 1024), (6, 500))


@pytest.mark.parametrize("signed", (False, True))
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("kind", ("off_by_2tol", "sign", "dropped", "leaked", "empty"))
def test_a_wrong_cell_fails(kind, cell, signed):
	n = 1037
	S, live = known_matrix(n, signed)
	want = np.where(live[None, :], S, 0.0)
	i, s = cell
	assert live[s] and abs(S[i, s]) > 10 * TOL
	bad = S.copy()
	hooks = {}
	if kind == "off_by_2tol":
		bad[i, s] += np.float32(2 * TOL)
		assert abs(float(bad[i, s]) - float(S[i, s])) > 1.9 * TOL
	elif kind == "sign":
		bad[i, s] = -bad[i, s]
	elif kind == "dropped":
		hooks["drop"] = (i, s)
	elif kind == "leaked":
		hooks["leak"] = (i, s, 0.5)       # comes back from every window that does not hold it
	else:
		bad[:, s] = -np.inf
	run = StandIn(bad, **hooks)
	if kind == "leaked":      # the reader's own assertion
		with pytest.raises(AssertionError, match="slice outside the window"):
			bw.read_matrix(run, n, N_Q, signed)
		return
	M = bw.read_matrix(run, n, N_Q, signed)
	# the comparison's, at that cell and no other (a cell that did not come back, a live column written as empty among them: an
	# unfilled cell where the oracle is not 0)
	column = N_Q if kind == "empty" else 1
	with pytest.raises(AssertionError, match=r"^%d cells beyond .*query %d slice %d: " % (column, 0 if kind == "empty" else i, s)):
		bw.assert_matrix(M, want, live, TOL)


def test_messages_name_the_cell():
	S, live = known_matrix(193, True)
	bad = S.copy()
	bad[4, 100] += np.float32(1e-3)
	M = bw.read_matrix(StandIn(bad), 193, N_Q, True)
	with pytest.raises(AssertionError, match=r"query 4 slice 100: .* slot 1 of tile 1"):
		bw.assert_matrix(M, np.where(live[None, :], S, 0.0), live, TOL, where=lambda i, s: "slot %d of tile %d" % (i % 3, i // 3))


def test_too_many_unreturned_slices_fail_the_cap():
	"""a pass that wrote 0 where the oracle has 0 within tol on more than 1 % of a query's live slices proves nothing about them"""
	n = 1037
	S, live = known_matrix(n, False)
	S[3, 100:120] = 0.0
	want = np.where(live[None, :], S, 0.0)
	with pytest.raises(AssertionError):
		bw.assert_oracle_cap(want, live, TOL)
	with pytest.raises(AssertionError):
		bw.assert_matrix(bw.read_matrix(StandIn(S), n, N_Q, False), want, live, TOL)
