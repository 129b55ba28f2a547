"""-m gpu: every cell of the [queries x slices] score matrix of vk_query_batch against the oracle's score of every slice, on every
form of the batched relaxed-WMD GEMM (vk_rwmd_batch.hip: the 16-row kernel, the 32x32x16 kernels with two or three queries per A
tile, the dense form, W64, wide32, the padded length buckets, the static table and gather pass) and of the shared pass
(vk_score_batch.hip).  The matrix is a workspace; batch_windows.read_matrix reads it through `boost`, 64 slices at a time (DESIGN 7.4;
test_batch_windows_host.py shows that the reader cannot hide a wrong cell).  Each case asserts the route and form it is about from
vk_batch_state, an internal export of the library as vk_bound_pass_state is.

Tolerances are the project's own: 2e-5 for the relaxed WMD (score_tol of every batch test), 1e-4 for alignments (last_scores()
everywhere).  The largest |batch cell - last_scores() of a single vk_query| per form is recorded, not asserted, and printed at the
end of the module (run with -s); DESIGN 7.4 holds the table."""

import concurrent.futures
import ctypes as C

import numpy as np
import pytest

from vectorian_amd import synth

import batch_windows as bw
from helpers import hip_static_corpus, prep_contextual, prep_query

pytestmark = pytest.mark.gpu

EXP5 = ("table", (1 - 2.0 ** (-np.arange(0, 65) / 5)).astype(np.float32))
AFF = ("affine", 0.2, 0.05)
GAPS = (("linear", (0.1, 0.1), 0), ("affine", (AFF, AFF), 1), ("exp5", (EXP5, EXP5), 2))    # (name, gaps, vk_host::classify_gaps)
RWMD_TOL, ALIGN_TOL = 2e-5, 1e-4
FLAGS = ((True, True, True), (True, False, True), (True, False, False))   # (injective, symmetric, normalize_bow); symmetric needs nbow
PER_QUERY, SHARED, GEMM = 1, 2, 3
STATE = ("route", "qb_max", "lt", "gap_mode", "stat", "stat_uniform32", "uniform16", "b32", "r32", "gran", "wide32", "dense", "qpt",
	"n_qtiles", "uniform_len", "late_mask")    # vk_corpus::batch_state

MAXIMA = {}      # form -> largest |batch cell - single-query cell| seen
WORLDS = {}      # contextual corpora several cases share: key -> (corpus, stored rows, slice starts, slice ends)
SIMS = {}        # (world, query set) -> the oracle's similarity rows of every token against each query (vko_sim_bf16), for every option set
ORACLE = {}      # (world, query set, options) -> the oracle's score of every slice, [queries x n]
SINGLE = {}      # ... -> last_scores() of a single vk_query per query (the single-query pass reads none of the batch switches)


@pytest.fixture(scope="module", autouse=True)
def report():
	yield
	print("\nlargest |batch cell - last_scores() of a single query| per form")
	for form in sorted(MAXIMA):
		print("  %-46s %.3g" % (form, MAXIMA[form]))
	WORLDS.clear(); SIMS.clear(); ORACLE.clear(); SINGLE.clear()


def batch_state(hip, c):
	lib = hip.lib()
	lib.vk_batch_state.restype = C.c_int
	lib.vk_batch_state.argtypes = [C.c_void_p, C.c_void_p]
	st = np.zeros(len(STATE), dtype=np.int64)
	with c.lock:
		hip._check(lib.vk_batch_state(c._h, st.ctypes.data))
	return dict(zip(STATE, st.tolist()))


def world(n, lo, hi, d, empty=()):
	"""synth.make_contextual_corpus(n, lo, hi, 2000, d) as the batch tests store it; `empty`: slices emptied afterwards"""
	key = (n, lo, hi, d, tuple(empty))
	if key not in WORLDS:
		corpus = synth.make_contextual_corpus(n, lo, hi, 2000, d)
		off = corpus["sent_off"]
		start, end = off[:-1].copy(), off[1:].copy()
		end[list(empty)] = start[list(empty)]
		WORLDS[key] = (corpus, prep_contextual(corpus), start, end)
	return (key,) + WORLDS[key]


def contextual_handle(hip, Xb, start, end):
	c = hip.Corpus(layout=hip.VK_LAYOUT_CONTEXTUAL, d=Xb.shape[1], n_tokens=Xb.shape[0], n_sentences=len(start))
	c.append_vectors(Xb, normalize=False)
	if (start[1:] == end[:-1]).all() and start[0] == 0:
		c.set_sentences(np.concatenate((start, end[-1:])))
	else:
		c.set_slices(start, end)
	c.finalize()
	return c


def queries_of(corpus, lengths, seed=None):
	"""one query per entry of `lengths`: synth.make_queries at the longest of them, each cut to its length"""
	made = synth.make_queries(corpus, len(lengths), max(lengths), **({} if seed is None else dict(seed=seed)))
	return [prep_query(q)[:m] for q, m in zip(made, lengths)]


def slot(st, i):
	"""where vk_batch.cpp's slot_of puts query i, for the message of a failing cell"""
	if st["route"] == SHARED:
		return "strip %d of pass %d" % (i % st["qb_max"], i // st["qb_max"])
	if st["dense"]:
		return "slot %d of super tile %d" % (i % 16, i // 16)
	if st["b32"]:
		return "slot %d of tile %d (qpt %d)" % (i % st["qpt"], i // st["qpt"], st["qpt"])
	return "row block %d" % i


def every_slice(hip, c, form, expect, want, single, live, lens, qs, tol, signed, run_batch, reads=1, record=None):
	"""the matrix of one option set against the oracle's (want), the route and form (expect) and the record against `single`"""
	bw.assert_oracle_cap(want, live, tol)          # the inputs, before anything of the library's is looked at
	for _ in range(reads):
		M = bw.read_matrix(run_batch, len(live), len(qs), signed)
		st = batch_state(hip, c)
		got = {k: st[k] for k in expect}
		assert got == expect, (form, got, expect, st)
		bw.assert_matrix(M, want, live, tol, where=lambda i, s: "%s: query of %d tokens in %s, slice of %d tokens" % (form, len(qs[i]), slot(st, i), lens[s]))
		filled = ~np.isnan(M)
		if filled.any():
			MAXIMA[record or form] = max(MAXIMA.get(record or form, 0.0), float(np.abs(M[filled].astype(np.float64) - single[filled]).max()))


def cached(store, key, make):
	if key not in store:
		store[key] = make()
	return store[key]


def sims(oracle, key, X, qs):
	"""the dot products are most of the oracle's time: once per query, a few queries at a time (the call leaves the interpreter)"""
	def make():
		with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
			return list(pool.map(lambda Q: oracle.sim_bf16(X, Q), qs))
	return cached(SIMS, key, make)


# ---- relaxed 1:1 WMD over the contextual layout -----------------------------------------------------------------------------

def rwmd_contextual(hip, oracle, wkey, lengths, form, expect, c=None, reads=1, flag_sets=FLAGS, seed=None):
	key, corpus, Xb, start, end = world(*wkey)
	n, d = len(start), Xb.shape[1]
	live, lens = end > start, end - start
	n_tok = int(max(start[-1], end[-1]))     # the tokens the oracle counts (the last slice may be an emptied one)
	qs = queries_of(corpus, lengths, seed)
	own = c is None
	c = contextual_handle(hip, Xb, start, end) if own else c
	try:
		for flags in flag_sets:
			okey = (key, tuple(lengths), seed, "rwmd", flags)

			def oracle_all():
				S = sims(oracle, (key, tuple(lengths), seed), Xb[:n_tok], qs)
				refs = oracle.find_many(layout=oracle.LAYOUT_CONTEXTUAL, d=d, sent_off=start, sent_end=end, X=Xb, Qs=qs, S_rows=S,
					algorithm=oracle.ALG_RWMD, rwmd=flags, max_matches=1, min_score=0.0, want_all_scores=True, n_threads=8)
				return np.stack([r["all_scores"] for r in refs])

			def single_all():
				rows = []
				for Q in qs:
					c.query(Q, algorithm=hip.VK_ALG_RWMD, rwmd=flags, q_normalize=False, max_matches=10, min_score=0.0, want_flow=False)
					rows.append(c.last_scores())
				return np.stack(rows).astype(np.float64)

			want = cached(ORACLE, okey, oracle_all)
			single = cached(SINGLE, okey, single_all)
			run = lambda boost: c.query_batch(qs, algorithm=hip.VK_ALG_RWMD, rwmd=flags, q_normalize=False, boost=boost, min_score=0.0,
				max_matches=64, want_flow=False)
			every_slice(hip, c, form, expect, want, single, live, lens, qs, RWMD_TOL, False, run, reads)
	finally:
		if own:
			c.close()


A32 = (1037, 32, 32, 300)
MIXED_10 = [1 + (3 * i) % 10 for i in range(10)]                                  # 1, 4, 7, 10, 3, 6, 9, 2, 5, 8
MIXED_53 = [10 if i % 3 != 1 else 1 + (7 * i) % 10 for i in range(53)]           # every length 1..10; ten-token queries in the split slots 5..7 of a half
RAGGED_300 = (700, 1, 64, 300, (5, 77, 699))
RAGGED_768 = (700, 8, 64, 768)
# over slices of 1..64 tokens a query of one or two tokens has no positive cosine with more than 1 % of the slices (the shortest ones):
# a score of exactly 0, which the reader sees as "nothing returned" -- the cap of batch_windows.  From three tokens on it holds.
RAGGED_19 = [10, 3, 10, 10, 7, 10, 4, 10, 10, 5, 10, 10, 9, 10, 6, 10, 10, 8, 3]


def test_three_queries_per_tile(hip, oracle):
	"""10 queries of 1..10 tokens: three per 32-row A tile, the third split over the lane halves; the last tile holds one"""
	assert sorted(MIXED_10) == list(range(1, 11))
	rwmd_contextual(hip, oracle, A32, MIXED_10, "b32 qpt 3", dict(route=GEMM, b32=1, r32=0, dense=0, qpt=3, n_qtiles=4, uniform_len=32, wide32=0))


def test_two_queries_per_tile(hip, oracle):
	"""a query of more than 10 tokens in the batch: two per tile"""
	rwmd_contextual(hip, oracle, A32, [10, 16, 7, 11, 3], "b32 qpt 2", dict(route=GEMM, b32=1, r32=0, dense=0, qpt=2, n_qtiles=3))


@pytest.mark.parametrize("switch,value,form,expect", [
	(None, None, "b32 dense", dict(dense=1, n_qtiles=20, late_mask=4)),                     # 53 = 3 x 16 + 5: the last super tile is partly empty
	("VK_BATCH32_NO_DENSE", "1", "b32 qpt 3, 53 queries", dict(dense=0, n_qtiles=18)),
	("VK_BATCH32_LATE_MASK", "0", "b32 dense, late_mask 0", dict(dense=1, n_qtiles=20, late_mask=0)),   # the other phase pattern of the waves
])
def test_53_queries(hip, oracle, monkeypatch, switch, value, form, expect):
	assert set(MIXED_53) == set(range(1, 11))
	if switch:
		monkeypatch.setenv(switch, value)
	rwmd_contextual(hip, oracle, A32, MIXED_53, form, dict(route=GEMM, b32=1, r32=0, qpt=3, uniform_len=32, **expect))


def test_one_sentence_per_wave(hip, oracle):
	"""64-token slices: W64"""
	rwmd_contextual(hip, oracle, (1037, 64, 64, 300), [10, 7, 10, 4, 10, 9, 10, 10, 1], "b32 W64", dict(route=GEMM, b32=1, r32=0, uniform16=1, uniform_len=64, qpt=3, dense=0))


@pytest.mark.parametrize("length", (16, 48))
@pytest.mark.parametrize("d", (300, 128))
def test_sixteen_row_kernel(hip, oracle, length, d):
	rwmd_contextual(hip, oracle, (1037, length, length, d), [12, 9, 16, 5, 12, 1, 14, 12, 3], "16-row, %d-d x %d" % (d, length),
		dict(route=GEMM, uniform16=1, b32=0, r32=0, uniform_len=length, stat=0))


def test_ragged_buckets(hip, oracle):
	"""slices of 1..64 tokens, three of them emptied: padded buckets of 32 and 64 tokens on the 32x32x16 kernels, scores back at the
	original indices; the matrix of the call that builds the layout and again on the layout it built"""
	rwmd_contextual(hip, oracle, RAGGED_300, RAGGED_19, "r32 gran 2", dict(route=GEMM, r32=1, b32=1, gran=2, uniform16=0, qpt=3, dense=0), reads=2)


def test_ragged_768(hip, oracle):
	rwmd_contextual(hip, oracle, RAGGED_768, [10] * 9 + [7, 1], "wide32 ragged", dict(route=GEMM, wide32=1, r32=1, gran=2, uniform16=0))


def test_ragged_768_on_the_sixteen_row_kernel(hip, oracle, monkeypatch):
	"""VK_BATCH_WIDE16=1 on a handle of its own (the bucket layout is built once per handle): buckets of 16 / 32 / 48 / 64 padded tokens"""
	monkeypatch.setenv("VK_BATCH_WIDE16", "1")
	rwmd_contextual(hip, oracle, RAGGED_768, [10] * 9 + [7, 1], "16-row ragged 768-d, gran 1", dict(route=GEMM, wide32=0, r32=0, b32=0, gran=1, uniform16=0))


def test_uniform_768(hip, oracle, monkeypatch):
	"""32-token slices at 768-d: wide32 (four waves per workgroup); then the 16-row kernel at 24 K-steps on the same handle (uniform
	slices run on the resident tiles: nothing is built per handle)"""
	wkey = (1037, 32, 32, 768)
	_, _, Xb, start, end = world(*wkey)
	c = contextual_handle(hip, Xb, start, end)
	try:
		lengths = [10, 7, 10, 10, 4, 1]
		rwmd_contextual(hip, oracle, wkey, lengths, "wide32 uniform", dict(route=GEMM, wide32=1, b32=1, r32=0, uniform16=1, qpt=3), c=c)
		monkeypatch.setenv("VK_BATCH_WIDE16", "1")
		rwmd_contextual(hip, oracle, wkey, lengths, "16-row, 768-d x 32", dict(route=GEMM, wide32=0, b32=0, r32=0, uniform16=1), c=c)
	finally:
		c.close()


# ---- relaxed 1:1 WMD over the static layout -----------------------------------------------------------------------------------

STATIC = {"ragged40": (1500, 0, 40, 400, 300), "uniform32": (1003, 32, 32, 300, 300), "ragged64": (900, 1, 64, 500, 128), "wide": (700, 2, 50, 350, 96)}


@pytest.mark.parametrize("shape,n_q,len_t,expect", [
	("uniform32", 40, 9, dict(stat_uniform32=1, dense=1, qpt=3)),
	("ragged40", 9, 6, dict(stat_uniform32=0, dense=0, qpt=3, n_qtiles=3)),        # both length buckets, empty slices
	("ragged40", 53, 10, dict(stat_uniform32=0, dense=1, qpt=3, n_qtiles=20)),
	("ragged64", 7, 16, dict(stat_uniform32=0, dense=0, qpt=2, n_qtiles=4)),
	("wide", 12, 8, dict(stat_uniform32=0, dense=0, qpt=3, n_qtiles=4)),           # 96-d rows: the table kernel takes any width
])
def test_static(hip, oracle, shape, n_q, len_t, expect):
	"""queries as test_static_rwmd_batch builds them: an id repeated, an id of -1, frequent words"""
	n, lo, hi, V, d = STATIC[shape]
	corpus = synth.make_static_corpus(n, lo, hi, V, d)
	c, Eb = hip_static_corpus(hip, corpus)
	off = corpus["sent_off"]
	lens = np.diff(off)
	live = lens > 0
	assert live.all() == (lo > 0)
	rng = np.random.default_rng(7)
	qids, qs = [], []
	for i in range(n_q):
		# (no one-token query: it has no positive cosine with more than 1 % of the slices -- exact zeros, beyond the cap of batch_windows)
		ids = rng.integers(0, 60 if i % 2 else V, size=max(2, 1 + (i * 3) % len_t) if i % 5 == 3 else len_t).astype(np.int32)
		if len(ids) > 3:
			ids[3] = ids[0]
		if i % 7 == 2:
			ids[-1] = -1
		qids.append(ids)
		qs.append(Eb[np.where(ids >= 0, ids, 5)])
	form = "static %s, %d queries" % (shape, n_q)
	try:
		for flags in FLAGS:
			refs = oracle.find_many(layout=oracle.LAYOUT_STATIC, d=d, sent_off=off, tok_id=corpus["tok_id"], E=Eb, Qs=qs, q_ids=qids,
				algorithm=oracle.ALG_RWMD, rwmd=flags, max_matches=1, min_score=0.0, want_all_scores=True, n_threads=8)
			want = np.stack([r["all_scores"] for r in refs])
			rows = []
			for Q, ids in zip(qs, qids):
				c.query(Q, q_token_ids=ids, algorithm=hip.VK_ALG_RWMD, rwmd=flags, q_normalize=False, max_matches=10, min_score=0.0, want_flow=False)
				rows.append(c.last_scores())
			run = lambda boost: c.query_batch(qs, token_ids=qids, algorithm=hip.VK_ALG_RWMD, rwmd=flags, q_normalize=False, boost=boost,
				min_score=0.0, max_matches=64, want_flow=False)
			every_slice(hip, c, form, dict(route=GEMM, stat=1, b32=1, **expect), want, np.stack(rows).astype(np.float64), live, lens, qs, RWMD_TOL, False, run)
	finally:
		c.close()


# ---- the shared pass ------------------------------------------------------------------------------------------------------------

SEVEN = [11, 3, 16, 1, 8, 12, 5]
# synth.make_queries' seed for the seven: chosen on the oracle alone.  A one-token query has no positive cosine with some 20 of the 901
# slices of 1..64 tokens at most seeds (the one- and two-token slices): a local score of exactly 0 on more than the 1 % that
# batch_windows lets come back as "nothing returned".  With this seed it is 7 slices; assert_oracle_cap states it before every read.
# 7 against a cap of 9 is a thin margin: after a change to synth.make_queries it is assert_oracle_cap that fails (the inputs, not a
# kernel), and the seed is chosen anew, on the oracle.
SEVEN_SEED = 10
SEVEN_RWMD = [11, 3, 16, 4, 8, 12, 5]      # relaxed WMD over ragged slices: no query below three tokens (RAGGED_19)


def batches_of(lengths):
	"""the batch and its sub-batches by their longest query: lt = 16, 12, 8, 4 (vk_score_batch_kernel<GAP, LT>)"""
	return [(lt, [m for m in lengths if m <= lt]) for lt in (16, 12, 8, 4)]


def shared_pass(hip, oracle, monkeypatch, wkey, qb, options, form_of, tol, lengths=SEVEN, seed=SEVEN_SEED):
	"""options: (name, signed, expected gap_mode, common options of the library's calls and the oracle's)"""
	key, corpus, Xb, start, end = world(*wkey)
	n, d = len(start), Xb.shape[1]
	live, lens = end > start, end - start
	n_tok = int(max(start[-1], end[-1]))     # the tokens the oracle counts (the last slice may be an emptied one)
	if qb:
		monkeypatch.setenv("VK_BATCH_QB", str(qb))
	seven = queries_of(corpus, lengths, seed)
	c = contextual_handle(hip, Xb, start, end)
	try:
		for name, signed, gap_mode, kw_hip, kw_oracle in options:
			okey = (key, tuple(lengths), seed, name)

			def oracle_all():
				S = sims(oracle, (key, tuple(lengths), seed), Xb[:n_tok], seven)
				refs = oracle.find_many(layout=oracle.LAYOUT_CONTEXTUAL, d=d, sent_off=start, sent_end=end, X=Xb, Qs=seven, S_rows=S,
					max_matches=1, min_score=-1e9, want_all_scores=True, n_threads=8, **kw_oracle)
				return np.stack([r["all_scores"] for r in refs])

			def single_all():
				rows = []
				for Q in seven:
					c.query(Q, q_normalize=False, max_matches=10, min_score=-1e9, want_flow=False, **kw_hip)
					rows.append(c.last_scores())
				return np.stack(rows).astype(np.float64)

			want7 = cached(ORACLE, okey, oracle_all)
			single7 = cached(SINGLE, okey, single_all)
			for lt, some in batches_of(lengths):
				assert len(some) >= 2 and max(some) > lt - 4
				pick = [lengths.index(m) for m in some]
				qs = [seven[i] for i in pick]
				run = lambda boost: c.query_batch(qs, q_normalize=False, boost=boost, min_score=0.0, max_matches=64, want_flow=False, **kw_hip)
				every_slice(hip, c, "%s, %s, lt %d" % (form_of(name), name, lt), dict(route=SHARED, qb_max=expected_qb(wkey, lt, qb), lt=lt, gap_mode=gap_mode),
					want7[pick], single7[pick], live, lens, qs, tol, signed, run, record=form_of(name))
	finally:
		c.close()


# queries per pass (qb_max): VK_BATCH_QB, 2 where it is unset, except where that many strips and query tiles do not fit the LDS
# (DESIGN 7.4): the most that fit, by (corpus, lt)
QB_FITS = {((1037, 32, 32, 300), 16): 3, ((901, 1, 64, 64), 16): 2, ((901, 1, 64, 64), 12): 3}


def expected_qb(wkey, lt, qb):
	return min(qb or 2, QB_FITS.get((wkey[:4], lt), 4))


def alignment_options(table_mode):
	out = []
	for loc in (0, 1, 2):
		for gname, (gs, gt), klass in GAPS:
			kw = dict(locality=loc, gap_s=gs, gap_t=gt)
			out.append(("loc %d %s" % (loc, gname), loc != 0, klass if klass < 2 else table_mode, kw, kw))
	return out


@pytest.mark.parametrize("qb", (None, 2, 3, 4))
@pytest.mark.parametrize("wkey,table_mode", [((1037, 32, 32, 300), 3), ((901, 1, 64, 64), 6)])
def test_shared_pass_alignments(hip, oracle, monkeypatch, wkey, table_mode, qb):
	"""seven queries of 1..16 tokens, two to four per pass (the last pass of the seven holds 1, 1 or 3), every locality and gap family;
	localities 1 and 2 score below 0 too: the signed reader.  Tables run on the register-history forms: gap_mode 3 over slices of at
	most 32 tokens, 6 up to 64"""
	shared_pass(hip, oracle, monkeypatch, wkey, qb, alignment_options(table_mode),
		lambda name: "shared %d-d, gap_mode %s" % (wkey[3], {"linear": "0", "affine": "1", "exp5": str(table_mode)}[name.split()[-1]]), ALIGN_TOL)


def rwmd_options(hip, oracle):
	return [("rwmd %s" % (flags,), False, 4, dict(algorithm=hip.VK_ALG_RWMD, rwmd=flags), dict(algorithm=oracle.ALG_RWMD, rwmd=flags)) for flags in FLAGS]


def test_shared_pass_rwmd_96(hip, oracle, monkeypatch):
	"""96-d rows: no GEMM form exists for that width; slices of 1..64 tokens, three of them emptied"""
	shared_pass(hip, oracle, monkeypatch, (700, 1, 64, 96, (5, 77, 699)), None, rwmd_options(hip, oracle), lambda name: "shared 96-d, rwmd", RWMD_TOL,
		lengths=SEVEN_RWMD, seed=None)


def test_shared_pass_rwmd_300_without_buckets(hip, oracle, monkeypatch):
	monkeypatch.setenv("VK_BATCH_NO_RAGGED", "1")
	shared_pass(hip, oracle, monkeypatch, RAGGED_300, None, rwmd_options(hip, oracle), lambda name: "shared 300-d, rwmd (VK_BATCH_NO_RAGGED)", RWMD_TOL,
		lengths=SEVEN_RWMD, seed=None)
