"""The whole [queries x slices] score matrix of a batch, read through the public API.

Both batch routes multiply the caller's `boost` in as the last operation of a score and admit a slice iff score > min_score.
With boost = +1 on a window of 64 consecutive slices and 0 elsewhere, min_score = 0, max_matches = 64 and no flows, the result set
of every query is exactly the slices of the window whose score is positive, each with the pass's own float (x 1.0 is exact;
outside the window the product is +-0, an empty slice stays -inf: neither is > 0).  boost = -1 returns the negative cells as
-score, exact too.  A live slice that neither call returns scored exactly 0.

read_matrix: the matrix, NaN where nothing came back.  assert_matrix: the comparison with the oracle's score of every slice.
test_batch_windows_host.py shows on a numpy stand-in that no wrong cell gets through the two."""

import numpy as np

WINDOW = 64          # max_matches of a batch without flows (vk_batch.cpp)
ZERO_CAP = 0.01      # at most this part of a query's live slices may come back as "nothing returned" (a score of 0 within tol)


def window_boosts(n, sign):
	"""(window, boost) for every window of 64 consecutive slices of 0..n-1: boost is `sign` inside the window, 0.0 outside"""
	for a in range(0, n, WINDOW):
		window = range(a, min(a + WINDOW, n))
		boost = np.zeros(n, dtype=np.float32)
		boost[window.start:window.stop] = sign
		yield window, boost


def read_matrix(run_batch, n, n_queries, signed):
	"""run_batch(boost) -> one result per query (.n, .sentence, .score), the caller's closure around
	query_batch(..., boost=boost, min_score=0.0, max_matches=64, want_flow=False).
	signed: a second call per window with boost = -1 for the negative cells (global and semiglobal alignments)."""
	M = np.full((n_queries, n), np.nan, dtype=np.float32)
	seen = np.zeros((n_queries, n), dtype=bool)
	for sign in (1.0, -1.0) if signed else (1.0,):
		for window, boost in window_boosts(n, np.float32(sign)):
			outs = run_batch(boost)
			assert len(outs) == n_queries, (len(outs), n_queries)
			for i, got in enumerate(outs):
				assert 0 <= got.n <= WINDOW, ("result set beyond 64 entries", i, got.n)
				rows = np.asarray(got.sentence[:got.n], dtype=np.int64)
				vals = np.asarray(got.score[:got.n], dtype=np.float32)
				inside = (rows >= window.start) & (rows < window.stop)
				assert inside.all(), ("slice outside the window", i, window, sign, rows[~inside], vals[~inside])
				assert len(np.unique(rows)) == len(rows), ("slice twice in one result set", i, window, sign, rows)
				assert not seen[i, rows].any(), ("slice returned twice", i, window, sign, rows[seen[i, rows]])
				# what came back passed score > 0; an empty slice (-inf before the boost) never does
				assert (np.isfinite(vals) & (vals > 0)).all(), ("score not finite and positive", i, window, sign, rows, vals)
				seen[i, rows] = True
				M[i, rows] = vals if sign > 0 else -vals
	return M


def assert_oracle_cap(want, live, tol):
	"""the inputs' side of the cap: on the oracle alone, at most ZERO_CAP of a query's live slices score within tol of 0"""
	want = np.asarray(want)
	for i in range(want.shape[0]):
		near = int((np.abs(want[i, live]) <= tol).sum())
		assert near <= ZERO_CAP * int(live.sum()), ("the oracle scores too many slices at 0 for this check", i, near, int(live.sum()))


def assert_matrix(M, want, live, tol, where=None):
	"""M: read_matrix; want: the oracle's score of every slice [queries x n] (empty slices: anything); live: slices with tokens.
	where(query, slice) -> str: what the message says about a failing cell (slot, position, form)."""
	M, want, live = np.asarray(M), np.asarray(want), np.asarray(live, dtype=bool)
	assert M.shape == want.shape and live.shape == (M.shape[1],), (M.shape, want.shape, live.shape)
	filled = ~np.isnan(M)

	def cell(i, s):
		return "query %d slice %d: got %r, oracle %r%s" % (i, s, float(M[i, s]), float(want[i, s]), "" if where is None else " -- " + where(i, s))

	stray = filled & ~live[None, :]
	assert not stray.any(), "empty slice returned: " + "; ".join(cell(i, s) for i, s in np.argwhere(stray)[:8])
	with np.errstate(invalid="ignore"):
		diff = np.abs(M.astype(np.float64) - want.astype(np.float64))
		off = (filled & live[None, :] & ~(diff <= tol)) | (~filled & live[None, :] & ~(np.abs(want) <= tol))
	assert not off.any(), "%d cells beyond %g: " % (int(off.sum()), tol) + "; ".join(cell(i, s) for i, s in np.argwhere(off)[:8])
	missing = (~filled & live[None, :]).sum(axis=1)
	cap = ZERO_CAP * int(live.sum())
	assert (missing <= cap).all(), ("live slices that were not returned, per query (cap %g)" % cap, missing.tolist())
