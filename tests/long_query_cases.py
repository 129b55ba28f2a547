"""The inputs of tests/test_gpu_long_query_gaps_and_ties.py (queries of 65 .. 512 tokens: vk_longq_kernel and vk_longq_blocks_kernel), and
what tests/test_long_query_cases_host.py proves about them on the oracle alone.  No GPU, no library of the product.

Exact corpora: one-hot embeddings, so every similarity is exactly 0 or 1 -- in bf16, in fp32, under MFMA and under the canonical sums --,
and gap costs that are multiples of 1/8: every value of the DP is a multiple of 1/8 below 2^10, exact in fp32 in whatever order it is
summed.  The scoring pass, whose MFMA cosines are otherwise held to 1e-4, can then be held to ==.  Two kinds of token streams: `planted`
(a 12-token phrase once in the query and twice in a slice: the maximum is attained twice, in two lanes, in two blocks) and `shared`
(six words on both sides: co-optimal alignments everywhere).

Float corpora: mixed_corpus / quoting_query of test_gpu_long_query_long_slices.py under tables of the same shapes that are no
multiples of anything."""

import collections

import numpy as np

from vectorian_amd import synth

from test_gpu_long_query_long_slices import EDGE_LENS, mixed_corpus, quoting_query   # noqa: F401  (every block edge; the float corpora)

V = 64                                   # the vocabulary: E = I
PHRASE = np.arange(20, 32, dtype=np.int32)   # the planted phrase
SLICE_FILLER = (0, 6)                    # ids of the slices' filler
QUERY_FILLER = (40, 50)                  # ... of the planted query's: disjoint from the slices'
EXACT_LENS = (65, 80, 129)               # query lengths of the exact corpora (160: the first whose matrix leaves the LDS, see exact_plan)
LOCAL, GLOBAL, SEMIGLOBAL = 0, 1, 2


def one_hot(d):
	"""E = I, V = 64 rows of d >= 64 columns"""
	E = np.zeros((V, d), dtype=np.float32)
	E[np.arange(V), np.arange(V)] = 1.0
	return E


# ---- token streams ---------------------------------------------------------------------------------------------------------------

# a triple of otherwise identical slices: the phrase at both places, at the first only, at the second only
#   name: (tokens, first place, second place)
TRIPLES = collections.OrderedDict([
	("t200", (200, 10, 140)),   # blocks 0 and 2
	("t70", (70, 5, 55)),       # one block ...
	("t75", (75, 5, 55)),       # ... different lanes (the second ends in block 1)
	("t130", (130, 52, 64)),    # adjacent blocks: ends at token 64, starts again at token 65
	("t64", (64, 5, 45)),       # a slice of at most 64 tokens: two lanes of one sweep
])
# ... of the corpora without a slice of more than 64 tokens: there vk_longq_kernel restates the winners itself (beside longer slices all
# winners go through the block form), and the first lane among equals is its __ballot / ctz
SHORT_TRIPLES = collections.OrderedDict([("t64", (64, 5, 45)), ("t40", (40, 2, 26))])
STREAMS = ("planted", "shared", "planted64", "shared64")   # ...64: no slice of more than 64 tokens


def _plant(ids, at):
	ids = ids.copy()
	ids[at:at + len(PHRASE)] = PHRASE
	return ids


def exact_corpus(stream, seed=11, n_short=40, max_len=512):
	"""stream "planted" or "shared".  Slices: EDGE_LENS up to max_len, n_short of 1 .. 64 tokens, and the triples (max_len = 64:
	SHORT_TRIPLES), shuffled.  Returns ids, sent_off,
	lens and triples = {name: (both, first_only, second_only)} (slice numbers).
	planted: filler of ids 0 .. 5; besides the triples, every other slice of 8 tokens or more holds a run of 3 .. 12 words of the
	phrase, so that the scores of the corpus differ.  shared: the same slices and triples over the same filler -- the query shares it"""
	assert stream in ("planted", "shared")
	rng = np.random.default_rng(seed)
	slices, label = [], []
	for n in [n for n in EDGE_LENS if n <= max_len] + [int(x) for x in rng.integers(1, 65, size=n_short)]:
		ids = rng.integers(*SLICE_FILLER, size=n).astype(np.int32)
		if n >= 8 and len(slices) % 2 == 0:
			run = int(rng.integers(3, min(12, n) + 1))
			a = int(rng.integers(0, len(PHRASE) - run + 1))
			at = int(rng.integers(0, n - run + 1))
			ids[at:at + run] = PHRASE[a:a + run]
		slices.append(ids)
		label.append(None)
	which_triples = TRIPLES if max_len > 64 else SHORT_TRIPLES
	for name, (n, p1, p2) in which_triples.items():
		base = rng.integers(*SLICE_FILLER, size=n).astype(np.int32)
		for which, ids in (("both", _plant(_plant(base, p1), p2)), ("first", _plant(base, p1)), ("second", _plant(base, p2))):
			slices.append(ids)
			label.append((name, which))
	order = rng.permutation(len(slices))
	slices = [slices[i] for i in order]
	label = [label[i] for i in order]
	lens = np.array([len(s) for s in slices], dtype=np.int64)
	triples = {name: tuple(label.index((name, w)) for w in ("both", "first", "second")) for name in which_triples}
	return dict(stream=stream, ids=np.concatenate(slices).astype(np.int32), sent_off=np.concatenate(([0], np.cumsum(lens))).astype(np.int64),
		lens=lens, triples=triples)


def exact_query(stream, len_t, at="mid", seed=5):
	"""planted: filler of ids 40 .. 49 (no slice holds them) and the phrase once -- from token 30 on ("mid"), or as the query's last
	12 tokens ("end": a SEMIGLOBAL alignment ends in the last row or column, so only there it scores the bare 12);
	shared: len_t words of the slices' filler"""
	rng = np.random.default_rng(seed + len_t)
	if stream.startswith("shared"):
		return rng.integers(*SLICE_FILLER, size=len_t).astype(np.int32)
	q = rng.integers(*QUERY_FILLER, size=len_t).astype(np.int32)
	return _plant(q, 30 if at == "mid" else len_t - len(PHRASE))


def sim01(slice_ids, q_ids):
	"""the 0 / 1 similarities of one slice, [len_s x len_t]"""
	return (np.asarray(slice_ids)[:, None] == np.asarray(q_ids)[None, :]).astype(np.float32)


# ---- gap settings ----------------------------------------------------------------------------------------------------------------

N_TABLE = 513


def _table(f):
	w = np.array([f(k) for k in range(N_TABLE)], dtype=np.float32)
	w[0] = 0.0
	return ("table", w)


def sat(c, unit=0.125):
	"""min(unit k, unit c): constant from k = c on"""
	return _table(lambda k: min(unit * k, unit * c))


def csat(c, unit=1.0 / 64):
	"""strictly concave up to k = c, constant from there on: steps of c, c - 1, ... 1 units.  One gap is strictly cheaper than any two
	that make up its length, which min(unit k, unit c) is not -- under that ramp a candidate the tail's running maximum misses is
	made up for, to the bit, by a gap of one token after a shorter gap.  (Multiples of 1/64: as exact in fp32 as those of 1/8.)"""
	return _table(lambda k: unit * sum(c + 1 - i for i in range(1, min(k, c) + 1)))


def const(x):
	return _table(lambda k: x)


def steps(unit=0.25):
	"""unit ceil(k / 3): not subadditive (three gaps of one token cost 3 units, one of three tokens 1)"""
	return _table(lambda k: unit * ((k + 2) // 3))


def zigzag():
	"""0.25 + 0.125 (k mod 3): not monotone, never constant"""
	return _table(lambda k: 0.25 + 0.125 * (k % 3))


def ramp(unit=0.125):
	return _table(lambda k: unit * k)


def last_differs(len_t):
	"""0.5 throughout, 0.75 at the query's length: constant but for its last entry"""
	kind, w = const(0.5)
	w = w.copy()
	w[len_t] = 0.75
	return (kind, w)


def cost(gap, k):
	"""vk_host::gap_cost"""
	if k <= 0:
		return np.float32(0.0)
	if isinstance(gap, (int, float)):
		gap = ("linear", gap)
	if gap[0] == "linear":
		return np.float32(gap[1]) * np.float32(k)
	if gap[0] == "affine":
		return np.float32(gap[1]) + np.float32(gap[2]) * np.float32(k)
	return np.float32(gap[1][k])


def kind_of(gap):
	return "linear" if isinstance(gap, (int, float)) else gap[0]


def gap_mode(gap_s, gap_t):
	"""vk_host::classify_gaps: 0 both linear, 1 linear / affine, 2 a table on either side"""
	kinds = {kind_of(gap_s), kind_of(gap_t)}
	return 2 if "table" in kinds else 1 if "affine" in kinds else 0


def wt_tail_rule(gap_s, gap_t, len_t):
	"""the host's rule for VkLongqParams.wt_tail, restated: under general gaps, the smallest k >= 1 from which w_t is constant up to
	the query's length; 0 (no tail branch) when that is the query's length itself, or under other gaps"""
	if gap_mode(gap_s, gap_t) != 2:
		return 0
	w = [cost(gap_t, k) for k in range(len_t + 1)]
	kt = len_t
	while kt > 1 and w[kt - 1] == w[len_t]:
		kt -= 1
	return kt if kt < len_t else 0


def steps_tail(len_t):
	"""`steps` is constant over k = 3 j + 1 .. 3 j + 3: the query's length shares its step with the one or two entries before it unless
	len_t = 3 j + 1 -- by the host's rule a tail of len_t - 1 or len_t - 2, and none only at such a length"""
	first = (len_t + 2) // 3 * 3 - 2
	return first if first < len_t else 0


Setting = collections.namedtuple("Setting", "name gap_s gap_t tail")

AFF_S, AFF_T = ("affine", 0.25, 0.25), ("affine", 0.5, 0.125)
LINEAR_SETTINGS = ("lin0", "lin_asym", "lin_big")
AFFINE_SETTINGS = ("aff", "aff0", "aff_lin")
TABLE_SETTINGS = ("sat1", "sat2", "sat8", "sat9", "sat10", "sat_last", "last_differs", "steps", "zigzag", "tab_lin", "aff_tab")
SETTINGS = LINEAR_SETTINGS + AFFINE_SETTINGS + TABLE_SETTINGS
CONCAVE_SETTINGS = ("csat2", "csat8", "csat9", "csat10")   # beside sat2 .. sat10: tails at the same places that no chain of shorter gaps hides
SYMMETRIC = ("lin0", "lin_big", "aff0")   # w_s(k) = w_t(k) for every k (aff0: 0.25 k both, one of them as an affine cost): swapping them changes nothing


def gap_settings(len_t):
	"""name -> Setting.  All costs multiples of 1/8 (csat: of 1/64); every table is w_t against a w_s of another shape.  `tail`: the wt_tail the
	setting is built to have at this query length (what the shape says; the host module holds it against wt_tail_rule)"""
	S = [
		Setting("lin0", 0.0, 0.0, 0),
		Setting("lin_asym", 0.125, 0.5, 0),
		Setting("lin_big", 2.0, 2.0, 0),
		Setting("aff", AFF_S, AFF_T, 0),
		Setting("aff0", 0.25, ("affine", 0.0, 0.25), 0),    # linear + affine with a zero opening: E and H tie on every extension
		Setting("aff_lin", AFF_T, 0.25, 0),
		Setting("sat1", ramp(), const(0.25), 1),            # empty scan
		Setting("sat2", zigzag(), sat(2), 2),               # one-entry scan
		Setting("sat8", sat(2), sat(8), 8),                 # the scan loads eight candidates per trip: 7 ...
		Setting("sat9", steps(), sat(9), 9),                # ... 8 ...
		Setting("sat10", const(0.25), sat(10), 10),         # ... and 9 of them
		Setting("sat_last", const(0.5), sat(len_t - 1), len_t - 1),
		Setting("last_differs", sat(8), last_differs(len_t), 0),
		Setting("steps", sat(10), steps(), steps_tail(len_t)),
		Setting("zigzag", ramp(), zigzag(), 0),
		Setting("tab_lin", sat(9), 0.25, 0),                # table + linear: general gaps, w_t linear
		Setting("aff_tab", ("affine", 0.25, 0.125), sat(9), 9),   # affine + table
		Setting("csat2", ramp(), csat(2), 2),
		Setting("csat8", sat(2), csat(8), 8),
		Setting("csat9", const(0.25), csat(9), 9),
		Setting("csat10", zigzag(), csat(10), 10),
	]
	assert tuple(s.name for s in S) == SETTINGS + CONCAVE_SETTINGS
	return collections.OrderedDict((s.name, s) for s in S)


def exact_plan():
	"""(setting, locality, len_t, stream) of the exact runs.  Every setting: the planted ties under LOCAL and SEMIGLOBAL (where they
	are ties), the shared filler under GLOBAL and under one of the other two, every third setting the planted stream under GLOBAL too;
	the query length in rotation, so that every setting meets all three.  Then queries of 160 tokens under tables -- the matrix of
	the scoring pass over slices of up to 64 tokens has left the LDS (vk_longq_hm_in_lds: 150 tokens is the last that fits), with
	and without a tail"""
	plan = []
	for i, name in enumerate(SETTINGS):
		runs = [(LOCAL, "planted"), (SEMIGLOBAL, "planted"), (GLOBAL, "shared"), (LOCAL if i % 2 == 0 else SEMIGLOBAL, "shared")]
		if i % 3 == 0:
			runs.append((GLOBAL, "planted"))
		for r, (loc, stream) in enumerate(runs):
			plan.append((name, loc, EXACT_LENS[(i + r) % 3], stream))
		# the same over the corpora without long slices, at other lengths
		for r, (loc, stream) in enumerate(runs[:4]):
			plan.append((name, loc, EXACT_LENS[(i + r + 1) % 3], stream + "64"))
	# (a tail of len_t - 1 or len_t - 2 decides a score only where nearly the whole query is one gap: the lengths at which it does)
	plan += [("sat_last", GLOBAL, 129, "shared"), ("steps", GLOBAL, 129, "shared")]
	# the concave tails: GLOBAL, where gaps of every length are forced
	for i, name in enumerate(CONCAVE_SETTINGS):
		plan += [(name, GLOBAL, EXACT_LENS[i % 3], "shared"), (name, GLOBAL, EXACT_LENS[(i + 1) % 3], "shared64"), (name, GLOBAL, EXACT_LENS[(i + 2) % 3], "planted")]
	plan += [("sat9", GLOBAL, 160, "shared64"), ("steps", LOCAL, 160, "shared64"), ("sat2", SEMIGLOBAL, 160, "planted64")]
	plan += [("zigzag", LOCAL, 160, "shared"), ("sat10", GLOBAL, 160, "shared"), ("last_differs", SEMIGLOBAL, 160, "planted"), ("sat_last", LOCAL, 160, "planted")]
	return plan


def query_place(stream, loc):
	return "end" if (stream.startswith("planted") and loc == SEMIGLOBAL) else "mid"


# planted ties: under every setting, LOCAL and SEMIGLOBAL, the oracle scores the three slices of every triple alike (12.0) and starts
# "both" where it starts "first only" (tests/test_long_query_cases_host.py asserts it for each).  Not under GLOBAL: the whole slice is
# aligned, and the place of the phrase in it moves the gaps.
PLANTED_TIES = tuple((name, loc) for name in SETTINGS for loc in (LOCAL, SEMIGLOBAL))


# ---- the oracle over an exact corpus -----------------------------------------------------------------------------------------------

EXACT_MATCHES = 24   # the 15 slices of the triples tie at the top of the planted runs: all of them among the winners
_corpora, _refs = {}, {}


def corpus_of(stream):
	if stream not in _corpora:
		_corpora[stream] = exact_corpus(stream[:-2], seed=12, max_len=64) if stream.endswith("64") else exact_corpus(stream)
	return _corpora[stream]


def min_score_of(loc):
	return 0.0 if loc == LOCAL else -1e9


def oracle_exact(oracle, stream, name, loc, len_t, layout="contextual", d=64, f32=False, gaps=None, cache=True):
	"""the oracle's answer to one run of exact_plan: EXACT_MATCHES matches and the score of every slice.  The similarities are 0 / 1 in every
	layout, so the answer is one and the same for all of them (the host module asserts that); computed once and shared, read-only.
	gaps: other costs than the setting's (the host module swaps and truncates them)"""
	key = (stream, name, loc, len_t)
	plain = layout == "contextual" and d == 64 and not f32 and gaps is None
	if plain and cache and key in _refs:
		return _refs[key]
	c = corpus_of(stream)
	s = gap_settings(len_t)[name]
	gs, gt = gaps or (s.gap_s, s.gap_t)
	q_ids = exact_query(stream, len_t, query_place(stream, loc))
	E = one_hot(d)
	rows = (lambda x: np.ascontiguousarray(x, dtype=np.float32)) if f32 else synth.to_bf16_bits
	kw = dict(d=d, sent_off=c["sent_off"], locality=loc, gap_s=gs, gap_t=gt, max_matches=EXACT_MATCHES, min_score=min_score_of(loc), want_all_scores=True, n_threads=8)
	if layout == "static":
		ref = oracle.find(layout=oracle.LAYOUT_STATIC, tok_id=c["ids"], E=rows(E), Q=rows(E[q_ids]), q_ids=q_ids, **kw)
	else:
		ref = oracle.find(layout=oracle.LAYOUT_CONTEXTUAL, X=rows(E[c["ids"]]), Q=rows(E[q_ids]), **kw)
	for a in ref.values():
		a.setflags(write=False)
	if plain and cache:
		_refs[key] = ref
	return ref


# ---- float corpora ---------------------------------------------------------------------------------------------------------------

def fsqrt():
	return ("table", (0.1 * np.sqrt(np.arange(N_TABLE))).astype(np.float32))


def fsat(c):
	return ("table", np.minimum(0.1 * np.arange(N_TABLE), 0.1 * c).astype(np.float32))


FLOAT_SETTINGS = ("fsqrt", "fsat2", "fsat8", "fsat9", "fsat10")


def float_settings():
	"""the non-dyadic tables: 0.1 sqrt(k) (no tail) and min(0.1 k, 0.1 c); w_t = fsat_c runs against w_s = sqrt"""
	S = [Setting("fsqrt", fsat(3), fsqrt(), 0)] + [Setting(f"fsat{c}", fsqrt(), fsat(c), c) for c in (2, 8, 9, 10)]
	return collections.OrderedDict((s.name, s) for s in S)


FLOAT_CASES = ((64, 80), (64, 200), (300, 80), (300, 200))   # (d, len_t); 200 tokens: the matrix of the scoring pass in scratch
FLOAT_SEEDS = {(64, 80): 80, (64, 200): 200, (300, 80): 80, (300, 200): 200}   # of quoting_query; kept where the host module's sensitivity holds

_float = {}


def float_case(d, len_t):
	"""(corpus, bf16 rows, bf16 query) of one float case, built once"""
	if (d, len_t) not in _float:
		if d not in _float:
			corpus = mixed_corpus(d)
			_float[d] = (corpus, synth.to_bf16_bits(synth.normalize_rows(corpus["X"])))
		corpus, Xb = _float[d]
		s0, Q = quoting_query(corpus, len_t, seed=FLOAT_SEEDS[(d, len_t)])
		_float[(d, len_t)] = (corpus, Xb, synth.to_bf16_bits(synth.normalize_rows(Q)))
	return _float[(d, len_t)]


def float_plan():
	"""(d, len_t, setting, locality): every float setting at every case, the locality in rotation (every setting meets all three)"""
	return [(d, len_t, name, (i + j) % 3) for i, (d, len_t) in enumerate(FLOAT_CASES) for j, name in enumerate(FLOAT_SETTINGS)]


def truncated(gap_t, tail):
	"""the table with its tail moved one entry early: w[k >= tail] = w[tail - 1]"""
	w = gap_t[1].copy()
	w[tail:] = w[tail - 1]
	return ("table", w)
